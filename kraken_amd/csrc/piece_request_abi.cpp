// piece_request_abi.cpp -- piece request rounds: the availability counts and the rarest-first /
// sampled picks of piecerequest.Manager.ReservePieces (piecerequest/manager.go:101-137) for the
// peers of a batch of torrents.  The host forms (krk_piece_availability, krk_piece_select,
// krk_piece_request_round: piece_request_math.hpp on the calling thread, no device) and the
// device round (krk_piece_request_round_dev, piece_request.hip computing the same picks).
#include "piece_request_math.hpp"
#include "runtime.hpp"

using namespace krk;

static_assert(pr::kMaxLimit == KRK_PR_MAX_LIMIT && pr::kRarestFirst == KRK_PR_RAREST_FIRST &&
                  pr::kSample == KRK_PR_SAMPLE && pr::kAllowDuplicates == KRK_PR_ALLOW_DUPLICATES &&
                  pr::kNone == KRK_PR_NONE,
              "piece_request_math.hpp and kraken_hip.h name the same values");

namespace {

constexpr uint64_t kMaxOff = 1ull << 48;  // an offset past it is an error, and no sum below overflows

// What a round touches of each array, in elements; 0 when nothing is.
struct Extent {
    uint64_t bits = 0, peers = 0, pieces = 0, words = 0, units = 0;
    bool rarest = false;
};

// The checks both rounds share; *x the batch's extents.
int check_round(const char* who, const krk_request_torrent* t, uint64_t n, uint32_t limit, Extent* x) {
    KRK_CHECK(limit >= 1 && limit <= KRK_PR_MAX_LIMIT, KRK_EINVAL, "%s: limit %u outside [1, %u]", who, limit,
              KRK_PR_MAX_LIMIT);
    KRK_CHECK(!n || t, KRK_EINVAL, "%s: torrents is NULL", who);
    for (uint64_t k = 0; k < n; ++k) {
        KRK_CHECK(t[k].n_pieces < (1ull << 32), KRK_EINVAL, "%s: torrent %llu has %llu pieces (2^32 or more)", who,
                  (unsigned long long)k, (unsigned long long)t[k].n_pieces);
        KRK_CHECK(pr::flags_ok(t[k].flags), KRK_EINVAL, "%s: torrent %llu: invalid piece selection policy: %#x", who,
                  (unsigned long long)k, t[k].flags);
        KRK_CHECK(t[k].bits_off < kMaxOff && t[k].peer_off < kMaxOff && t[k].piece_off < kMaxOff, KRK_EINVAL,
                  "%s: torrent %llu: an offset of 2^48 or more", who, (unsigned long long)k);
        const uint64_t W = pr::words(t[k].n_pieces);
        if (W) x->bits = std::max(x->bits, t[k].bits_off + (1 + 2 * (uint64_t)t[k].n_peers) * W);
        if (t[k].n_peers) x->peers = std::max(x->peers, t[k].peer_off + t[k].n_peers);
        if (t[k].n_pieces) x->pieces = std::max(x->pieces, t[k].piece_off + t[k].n_pieces);
        x->words += W;
        x->units += (t[k].n_pieces + kPrG - 1) / kPrG;
        x->rarest |= (t[k].flags & pr::kPolicyMask) == pr::kRarestFirst && t[k].n_peers && t[k].n_pieces;
    }
    return KRK_OK;
}

}  // namespace

extern "C" {

int krk_piece_availability(const uint64_t* peer_bits, uint32_t n_peers, uint64_t n_pieces, uint32_t* counts_out) {
    KRK_CHECK(n_pieces < (1ull << 32), KRK_EINVAL, "piece_availability: %llu pieces (2^32 or more)",
              (unsigned long long)n_pieces);
    KRK_CHECK(!n_pieces || (counts_out && (peer_bits || !n_peers)), KRK_EINVAL, "piece_availability: null argument");
    pr::availability(peer_bits, pr::words(n_pieces), n_peers, n_pieces, counts_out);
    return KRK_OK;
}

int krk_piece_select(const uint64_t* cand, const uint64_t* blocked, const uint32_t* counts, uint64_t n_pieces, int32_t q,
                     uint32_t flags, uint64_t seed, uint32_t peer, uint32_t* picks_out, uint32_t* n_out) {
    KRK_CHECK(n_pieces < (1ull << 32), KRK_EINVAL, "piece_select: %llu pieces (2^32 or more)",
              (unsigned long long)n_pieces);
    KRK_CHECK(pr::flags_ok(flags), KRK_EINVAL, "piece_select: invalid piece selection policy: %#x", flags);
    KRK_CHECK(q <= (int32_t)KRK_PR_MAX_LIMIT, KRK_EINVAL, "piece_select: quota %d above the largest limit, %u", q,
              KRK_PR_MAX_LIMIT);
    const bool rarest = (flags & pr::kPolicyMask) == pr::kRarestFirst;
    KRK_CHECK(n_out && (q <= 0 || picks_out) && (!n_pieces || (cand && (counts || !rarest))), KRK_EINVAL,
              "piece_select: null argument");
    const uint32_t k = q <= 0 ? 0 : (uint32_t)q;
    const uint32_t m = pr::select(cand, blocked, nullptr, nullptr, counts, n_pieces, k, flags & pr::kPolicyMask, seed,
                                  peer, picks_out);
    for (uint32_t j = m; j < k; ++j) picks_out[j] = pr::kNone;
    *n_out = m;
    return KRK_OK;
}

int krk_piece_request_round(const krk_request_torrent* torrents, uint64_t n_torrents, const uint64_t* bits,
                            const int32_t* quota, uint32_t limit, uint32_t* counts_out, uint32_t* picks_out,
                            uint32_t* n_picked_out) {
    Extent x;
    int r = check_round("piece_request_round", torrents, n_torrents, limit, &x);
    if (r) return r;
    KRK_CHECK((bits || !x.bits) && (!x.peers || (quota && picks_out && n_picked_out)), KRK_EINVAL,
              "piece_request_round: null argument");
    for (uint64_t k = 0; k < n_torrents; ++k)
        for (uint32_t p = 0; p < torrents[k].n_peers; ++p)
            KRK_CHECK(quota[torrents[k].peer_off + p] <= (int32_t)limit, KRK_EINVAL,
                      "piece_request_round: torrent %llu peer %u: quota %d above the limit %u", (unsigned long long)k, p,
                      quota[torrents[k].peer_off + p], limit);
    std::vector<uint64_t> taken;
    std::vector<uint32_t> own;  // the counts when the caller does not ask for them
    for (uint64_t k = 0; k < n_torrents; ++k) {
        const krk_request_torrent& T = torrents[k];
        const uint64_t W = pr::words(T.n_pieces);
        const uint64_t* rows = W ? bits + T.bits_off : nullptr;
        const bool rarest = (T.flags & pr::kPolicyMask) == pr::kRarestFirst;
        uint32_t* counts = counts_out ? counts_out + T.piece_off : nullptr;
        if (!counts && rarest && T.n_peers) {
            own.resize(T.n_pieces);
            counts = own.data();
        }
        if (counts && T.n_pieces) pr::availability(rows + W, 2 * W, T.n_peers, T.n_pieces, counts);
        if (!T.n_peers) continue;
        taken.resize(W);
        pr::round_torrent(rows, T.n_pieces, T.n_peers, T.flags, T.seed, quota + T.peer_off, limit, counts, taken.data(),
                          picks_out + T.peer_off * limit, n_picked_out + T.peer_off);
    }
    return KRK_OK;
}

int krk_piece_request_round_dev(const krk_request_torrent* torrents_host, uint64_t n_torrents, const uint64_t* bits_dev,
                                const int32_t* quota_dev, uint32_t limit, uint32_t* counts_out, uint32_t* picks_out,
                                uint32_t* n_picked_out, void* stream) {
    Extent x;
    int r = check_round("piece_request_round_dev", torrents_host, n_torrents, limit, &x);
    if (r) return r;
    KRK_CHECK((bits_dev || !x.bits) && (!x.peers || (quota_dev && picks_out && n_picked_out)), KRK_EINVAL,
              "piece_request_round_dev: null argument");
    KRK_CHECK(n_torrents <= 0x7FFFFFFFull, KRK_ERANGE, "piece_request_round_dev: %llu torrents in one call",
              (unsigned long long)n_torrents);
    if (!n_torrents) return KRK_OK;
    KRK_DEVICE(D);
    KRK_CHECK(!((uintptr_t)bits_dev & 7) && !((uintptr_t)quota_dev & 3) && !((uintptr_t)counts_out & 3) &&
                  !((uintptr_t)picks_out & 3) && !((uintptr_t)n_picked_out & 3),
              KRK_EINVAL,
              "piece_request_round_dev: bits_dev must be 8-byte, quota_dev, counts_out, picks_out and n_picked_out "
              "4-byte aligned");
    KRK_CHECK((!x.bits || device_writable(bits_dev, 8 * x.bits)) &&
                  (!x.peers || (device_writable(quota_dev, 4 * x.peers) && device_writable(n_picked_out, 4 * x.peers) &&
                                device_writable(picks_out, 4 * x.peers * limit))) &&
                  (!counts_out || !x.pieces || device_writable(counts_out, 4 * x.pieces)),
              KRK_EINVAL,
              "piece_request_round_dev: bits_dev, quota_dev, counts_out, picks_out and n_picked_out must be device "
              "memory or page-locked host memory");
    hipStream_t s = pick(D, stream);
    // Counts nobody asked for live in scratch, packed torrent after torrent, and only when a
    // rarest-first torrent reads them.
    const bool own_counts = !counts_out && x.rarest;
    std::vector<PrTorrent> tors(n_torrents);
    uint64_t word = 0, unit = 0, piece = 0;
    for (uint64_t k = 0; k < n_torrents; ++k) {
        const krk_request_torrent& T = torrents_host[k];
        tors[k] = {T.n_pieces, T.bits_off, T.peer_off, own_counts ? piece : T.piece_off, T.seed, word, unit, T.n_peers,
                   T.flags};
        word += pr::words(T.n_pieces);
        unit += (T.n_pieces + kPrG - 1) / kPrG;
        piece += T.n_pieces;
    }
    void* d_tors = nullptr;  // copied into the library's pinned staging before this returns
    r = upload(D, tors.data(), tors.size() * sizeof(PrTorrent), &d_tors, s);
    if (r) return r;
    uint8_t* d_scratch = nullptr;  // [taken: a word a bitset word][counts: own_counts only]
    if (scratch_alloc(D, &d_scratch, 8 * word + (own_counts ? 4 * piece : 0) + 8, s) != hipSuccess) {
        scratch_free(D, d_tors, s);
        set_error(KRK_ENOMEM, "piece_request_round_dev: taken and counts scratch");
        return KRK_ENOMEM;
    }
    uint32_t* counts = own_counts ? reinterpret_cast<uint32_t*>(d_scratch + 8 * word) : counts_out;
    const hipError_t e = timed(K_PIECEREQ, s, [&] {
        return launch_piece_request(static_cast<const PrTorrent*>(d_tors), n_torrents, unit, bits_dev, quota_dev, limit,
                                    counts, reinterpret_cast<uint64_t*>(d_scratch), picks_out, n_picked_out, s);
    });
    scratch_free(D, d_scratch, s);
    scratch_free(D, d_tors, s);
    KRK_CHECK(e == hipSuccess, KRK_EHIP, "piece_request launch: %s", launch_error_text(e));
    return KRK_OK;
}

int krk_piece_request_geometry(uint64_t* pieces_per_pass, uint64_t* thread_stride, uint64_t* max_count_workgroups) {
    KRK_CHECK(pieces_per_pass && thread_stride && max_count_workgroups, KRK_EINVAL,
              "piece_request_geometry: null argument");
    *pieces_per_pass = kPrPass;
    *thread_stride = kPrG;
    *max_count_workgroups = kPrMaxBlocks;
    return KRK_OK;
}

}  // extern "C"
