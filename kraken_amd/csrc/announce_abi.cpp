// announce_abi.cpp -- announce rounds: the tracker's announce (UpdatePeer, GetPeers, the origins,
// SortPeers; tracker/trackerserver/announce.go:75-115) for a batch of announces over bit-matrix
// peer stores.  The host forms (krk_announce_handout, krk_announce_round: announce_math.hpp on the
// calling thread, no device) and the device form (krk_announce_round_dev, announce_round.hip
// computing the same rows and handouts).
#include "announce_math.hpp"
#include "runtime.hpp"

using namespace krk;

static_assert(an::kMaxWindows == KRK_AN_MAX_WINDOWS && an::kMaxOrigins == KRK_AN_MAX_ORIGINS &&
                  an::kMaxLimit == KRK_AN_MAX_LIMIT && an::kDefault == KRK_AN_DEFAULT &&
                  an::kCompleteness == KRK_AN_COMPLETENESS && an::kComplete == KRK_AN_COMPLETE &&
                  an::kNone == KRK_AN_NONE && an::kOrigin == KRK_AN_ORIGIN && an::kCompleteBit == KRK_AN_COMPLETE_BIT,
              "announce_math.hpp and kraken_hip.h name the same values");
static_assert(sizeof(an::Torrent) == sizeof(krk_announce_torrent) &&
                  offsetof(an::Torrent, bits_off) == offsetof(krk_announce_torrent, bits_off) &&
                  sizeof(an::Announce) == sizeof(krk_announce) && offsetof(an::Announce, seed) == offsetof(krk_announce, seed),
              "an::Torrent is krk_announce_torrent, an::Announce is krk_announce: the same fields in the same order");

namespace {

const an::Torrent* tors(const krk_announce_torrent* t) { return reinterpret_cast<const an::Torrent*>(t); }
const an::Announce* anns(const krk_announce* a) { return reinterpret_cast<const an::Announce*>(a); }

// The checks every form shares; *bits_words the words of `bits` the torrents name (0: none).
int check_round(const char* who, const krk_announce_torrent* t, uint64_t n_torrents, const krk_announce* a,
                uint64_t n_announces, uint32_t limit, uint32_t policy, uint64_t* bits_words) {
    KRK_CHECK(!n_torrents || t, KRK_EINVAL, "%s: torrents is NULL", who);
    KRK_CHECK(!n_announces || a, KRK_EINVAL, "%s: announces is NULL", who);
    const char* why = an::scalars_error(limit, policy);
    KRK_CHECK(!why, KRK_EINVAL, "%s: %s (limit %u, policy %u)", who, why, limit, policy);
    *bits_words = 0;
    for (uint64_t k = 0; k < n_torrents; ++k) {
        why = an::torrent_error(tors(t)[k]);
        KRK_CHECK(!why, KRK_EINVAL, "%s: torrent %llu: %s", who, (unsigned long long)k, why);
        const uint64_t wp = pr::words(t[k].n_peers);
        if (wp) *bits_words = std::max(*bits_words, t[k].bits_off + 2 * (uint64_t)t[k].n_windows * wp);
    }
    for (uint64_t k = 0; k < n_announces; ++k) {
        why = an::announce_error(anns(a)[k], tors(t), n_torrents);
        KRK_CHECK(!why, KRK_EINVAL, "%s: announce %llu: %s", who, (unsigned long long)k, why);
    }
    return KRK_OK;
}

}  // namespace

extern "C" {

int krk_announce_handout(const krk_announce_torrent* torrents, uint64_t n_torrents, const uint64_t* bits,
                         const krk_announce* announce, uint32_t limit, uint32_t policy, uint32_t* handout_out,
                         uint32_t* n_out, uint32_t* label_counts_out) {
    KRK_CHECK(announce, KRK_EINVAL, "announce_handout: announce is NULL");
    uint64_t words = 0;
    int r = check_round("announce_handout", torrents, n_torrents, announce, 1, limit, policy, &words);
    if (r) return r;
    KRK_CHECK(bits && handout_out && n_out && label_counts_out, KRK_EINVAL, "announce_handout: null argument");
    const an::Torrent& T = tors(torrents)[announce->torrent];
    *n_out = an::handout(bits + T.bits_off, T, *anns(announce), limit, policy, handout_out, label_counts_out);
    return KRK_OK;
}

int krk_announce_round(const krk_announce_torrent* torrents, uint64_t n_torrents, uint64_t* bits,
                       const krk_announce* announces, uint64_t n_announces, uint32_t limit, uint32_t policy,
                       uint32_t* handout_out, uint32_t* n_out, uint32_t* label_counts_out) {
    uint64_t words = 0;
    int r = check_round("announce_round", torrents, n_torrents, announces, n_announces, limit, policy, &words);
    if (r) return r;
    if (!n_announces) return KRK_OK;
    KRK_CHECK(bits && handout_out && n_out && label_counts_out, KRK_EINVAL, "announce_round: null argument");
    for (uint64_t k = 0; k < n_announces; ++k) {
        const an::Torrent& T = tors(torrents)[announces[k].torrent];
        an::update(bits + T.bits_off, T, anns(announces)[k]);
    }
    const uint64_t cap = limit + an::kMaxOrigins;
    for (uint64_t k = 0; k < n_announces; ++k) {
        const an::Torrent& T = tors(torrents)[announces[k].torrent];
        n_out[k] = an::handout(bits + T.bits_off, T, anns(announces)[k], limit, policy, handout_out + k * cap,
                               label_counts_out + k * 3);
    }
    return KRK_OK;
}

int krk_announce_round_dev(const krk_announce_torrent* torrents_host, uint64_t n_torrents, uint64_t* bits_dev,
                           const krk_announce* announces_host, uint64_t n_announces, uint32_t limit,
                           uint32_t policy, uint32_t* handout_out, uint32_t* n_out, uint32_t* label_counts_out,
                           void* stream) {
    uint64_t words = 0;
    int r = check_round("announce_round_dev", torrents_host, n_torrents, announces_host, n_announces, limit, policy,
                        &words);
    if (r) return r;
    if (!n_announces) return KRK_OK;
    KRK_CHECK(bits_dev && handout_out && n_out && label_counts_out, KRK_EINVAL, "announce_round_dev: null argument");
    KRK_CHECK(n_announces <= 0x7FFFFFFFull, KRK_ERANGE, "announce_round_dev: %llu announces in one call",
              (unsigned long long)n_announces);
    KRK_DEVICE(D);
    KRK_CHECK(!((uintptr_t)bits_dev & 7) && !((uintptr_t)handout_out & 3) && !((uintptr_t)n_out & 3) &&
                  !((uintptr_t)label_counts_out & 3),
              KRK_EINVAL,
              "announce_round_dev: bits_dev must be 8-byte, handout_out, n_out and label_counts_out 4-byte aligned");
    const uint64_t cap = limit + an::kMaxOrigins;
    KRK_CHECK(device_writable(bits_dev, 8 * words) && device_writable(handout_out, 4 * cap * n_announces) &&
                  device_writable(n_out, 4 * n_announces) && device_writable(label_counts_out, 12 * n_announces),
              KRK_EINVAL,
              "announce_round_dev: bits_dev, handout_out, n_out and label_counts_out must be device memory or "
              "page-locked host memory");
    hipStream_t s = pick(D, stream);
    // One staged block: the torrents, then the announces.
    const size_t ann_at = n_torrents * sizeof(an::Torrent);
    std::vector<uint8_t> stage(ann_at + n_announces * sizeof(an::Announce));
    memcpy(stage.data(), torrents_host, ann_at);
    memcpy(stage.data() + ann_at, announces_host, n_announces * sizeof(an::Announce));
    void* d_stage = nullptr;  // copied into the library's pinned staging before this returns
    r = upload(D, stage.data(), stage.size(), &d_stage, s);
    if (r) return r;
    const hipError_t e = timed(K_ANNOUNCE, s, [&] {
        return launch_announce_round(static_cast<const an::Torrent*>(d_stage),
                                     reinterpret_cast<const an::Announce*>(static_cast<const uint8_t*>(d_stage) + ann_at),
                                     n_announces, bits_dev, limit, policy, handout_out, n_out, label_counts_out, s);
    });
    scratch_free(D, d_stage, s);
    KRK_CHECK(e == hipSuccess, KRK_EHIP, "announce_round launch: %s", launch_error_text(e));
    return KRK_OK;
}

}  // extern "C"
