// piece_resend_abi.cpp -- resend rounds: the failed piece requests of a batch of torrents placed
// on other peers (Dispatcher.resendFailedPieceRequests, dispatch/dispatcher.go:401-434).  The
// host form (krk_piece_resend_round: piece_resend_math.hpp on the calling thread, no device) and
// the device form (krk_piece_resend_round_dev, piece_resend.hip computing the same targets).
#include "piece_resend_math.hpp"
#include "runtime.hpp"

using namespace krk;

static_assert(rs::kExpired == KRK_PR_EXPIRED && rs::kUnsent == KRK_PR_UNSENT && rs::kInvalid == KRK_PR_INVALID,
              "piece_resend_math.hpp and kraken_hip.h name the same values");
static_assert(sizeof(rs::Failed) == sizeof(krk_failed_request) &&
                  offsetof(rs::Failed, piece) == offsetof(krk_failed_request, piece) &&
                  offsetof(rs::Failed, peer) == offsetof(krk_failed_request, peer) &&
                  offsetof(rs::Failed, status) == offsetof(krk_failed_request, status),
              "rs::Failed is krk_failed_request");

namespace {

constexpr uint64_t kMaxOff = 1ull << 48;  // an offset past it is an error, and no sum below overflows

// What a round touches of each array, in elements; 0 when nothing is.
struct Extent {
    uint64_t bits = 0, peers = 0, failed = 0, n_failed = 0;  // n_failed: the lists' lengths added up
};

const rs::Failed* entries(const krk_failed_request* f) { return reinterpret_cast<const rs::Failed*>(f); }

// The checks both forms share, the lists included; *x the batch's extents.
int check_round(const char* who, const krk_request_torrent* t, const krk_resend_torrent* r, uint64_t n,
                const krk_failed_request* failed, Extent* x) {
    KRK_CHECK(!n || (t && r), KRK_EINVAL, "%s: torrents or resends is NULL", who);
    for (uint64_t k = 0; k < n; ++k) {
        KRK_CHECK(t[k].n_pieces < (1ull << 32), KRK_EINVAL, "%s: torrent %llu has %llu pieces (2^32 or more)", who,
                  (unsigned long long)k, (unsigned long long)t[k].n_pieces);
        KRK_CHECK(rs::flags_ok(t[k].flags), KRK_EINVAL, "%s: torrent %llu: unknown flag bit: %#x", who,
                  (unsigned long long)k, t[k].flags);
        KRK_CHECK(t[k].bits_off < kMaxOff && t[k].peer_off < kMaxOff && r[k].failed_off < kMaxOff, KRK_EINVAL,
                  "%s: torrent %llu: an offset of 2^48 or more", who, (unsigned long long)k);
        KRK_CHECK(r[k].n_failed < (1ull << 32), KRK_ERANGE, "%s: torrent %llu: %llu failed requests (2^32 or more)", who,
                  (unsigned long long)k, (unsigned long long)r[k].n_failed);
        const uint64_t W = pr::words(t[k].n_pieces);
        if (W) x->bits = std::max(x->bits, t[k].bits_off + (1 + 2 * (uint64_t)t[k].n_peers) * W);
        if (t[k].n_peers) x->peers = std::max(x->peers, t[k].peer_off + t[k].n_peers);
        if (r[k].n_failed) x->failed = std::max(x->failed, r[k].failed_off + r[k].n_failed);
        x->n_failed += r[k].n_failed;
    }
    KRK_CHECK(failed || !x->failed, KRK_EINVAL, "%s: failed is NULL", who);
    for (uint64_t k = 0; k < n; ++k) {
        if (!r[k].n_failed) continue;
        uint64_t at = 0;
        const char* why = rs::list_error(entries(failed) + r[k].failed_off, r[k].n_failed, t[k].n_pieces, t[k].n_peers, &at);
        KRK_CHECK(!why, KRK_EINVAL, "%s: torrent %llu, failed request %llu: %s", who, (unsigned long long)k,
                  (unsigned long long)at, why);
    }
    return KRK_OK;
}

}  // namespace

extern "C" {

int krk_piece_resend_round(const krk_request_torrent* torrents, const krk_resend_torrent* resends, uint64_t n_torrents,
                           const uint64_t* bits, const int32_t* quota, const krk_failed_request* failed,
                           uint32_t* target_out, int32_t* quota_left_out, uint32_t* n_resent_out) {
    Extent x;
    int r = check_round("piece_resend_round", torrents, resends, n_torrents, failed, &x);
    if (r) return r;
    KRK_CHECK((bits || !x.bits) && (quota || !x.peers) && (target_out || !x.failed) && (n_resent_out || !n_torrents),
              KRK_EINVAL, "piece_resend_round: null argument");
    std::vector<int32_t> own;  // the quota left when the caller does not ask for it
    std::vector<uint32_t> mark;
    for (uint64_t k = 0; k < n_torrents; ++k) {
        const krk_request_torrent& T = torrents[k];
        const krk_resend_torrent& R = resends[k];
        int32_t* left = quota_left_out ? quota_left_out + T.peer_off : nullptr;
        if (!left) {
            own.resize(T.n_peers);
            left = own.data();
        }
        if (T.flags & pr::kAllowDuplicates) mark.resize(T.n_peers);
        n_resent_out[k] = rs::resend_torrent(x.bits ? bits + T.bits_off : nullptr, T.n_pieces, T.n_peers, T.flags,
                                             T.n_peers ? quota + T.peer_off : nullptr,
                                             R.n_failed ? entries(failed) + R.failed_off : nullptr, R.n_failed,
                                             mark.data(), R.n_failed ? target_out + R.failed_off : nullptr, left);
    }
    return KRK_OK;
}

int krk_piece_resend_round_dev(const krk_request_torrent* torrents_host, const krk_resend_torrent* resends_host,
                               uint64_t n_torrents, const uint64_t* bits_dev, const int32_t* quota_dev,
                               const krk_failed_request* failed_host, uint32_t* target_out, int32_t* quota_left_out,
                               uint32_t* n_resent_out, void* stream) {
    Extent x;
    int r = check_round("piece_resend_round_dev", torrents_host, resends_host, n_torrents, failed_host, &x);
    if (r) return r;
    KRK_CHECK((bits_dev || !x.bits) && (quota_dev || !x.peers) && (target_out || !x.failed) &&
                  (n_resent_out || !n_torrents),
              KRK_EINVAL, "piece_resend_round_dev: null argument");
    KRK_CHECK(n_torrents <= 0x7FFFFFFFull, KRK_ERANGE, "piece_resend_round_dev: %llu torrents in one call",
              (unsigned long long)n_torrents);
    if (!n_torrents) return KRK_OK;
    KRK_DEVICE(D);
    KRK_CHECK(!((uintptr_t)bits_dev & 7) && !((uintptr_t)quota_dev & 3) && !((uintptr_t)target_out & 3) &&
                  !((uintptr_t)quota_left_out & 3) && !((uintptr_t)n_resent_out & 3),
              KRK_EINVAL,
              "piece_resend_round_dev: bits_dev must be 8-byte, quota_dev, target_out, quota_left_out and n_resent_out "
              "4-byte aligned");
    KRK_CHECK((!x.bits || device_writable(bits_dev, 8 * x.bits)) &&
                  (!x.peers || (device_writable(quota_dev, 4 * x.peers) &&
                                (!quota_left_out || device_writable(quota_left_out, 4 * x.peers)))) &&
                  (!x.failed || device_writable(target_out, 4 * x.failed)) && device_writable(n_resent_out, 4 * n_torrents),
              KRK_EINVAL,
              "piece_resend_round_dev: bits_dev, quota_dev, target_out, quota_left_out and n_resent_out must be device "
              "memory or page-locked host memory");
    hipStream_t s = pick(D, stream);
    // One staged block: the torrents, then their lists packed torrent after torrent.  The quota
    // left nobody asked for and the marks live in scratch, packed the same way.
    const size_t list_at = n_torrents * sizeof(RsTorrent);
    std::vector<uint8_t> stage(list_at + x.n_failed * sizeof(rs::Failed));
    RsTorrent* tors = reinterpret_cast<RsTorrent*>(stage.data());
    rs::Failed* lists = reinterpret_cast<rs::Failed*>(stage.data() + list_at);
    uint64_t peer = 0, entry = 0;
    for (uint64_t k = 0; k < n_torrents; ++k) {
        const krk_request_torrent& T = torrents_host[k];
        const krk_resend_torrent& R = resends_host[k];
        tors[k] = {T.n_pieces, T.bits_off, T.peer_off, quota_left_out ? T.peer_off : peer, peer, entry, R.failed_off,
                   R.n_failed, T.n_peers, T.flags, 0};
        if (R.n_failed) memcpy(lists + entry, failed_host + R.failed_off, R.n_failed * sizeof(rs::Failed));
        peer += T.n_peers;
        entry += R.n_failed;
    }
    void* d_stage = nullptr;  // copied into the library's pinned staging before this returns
    r = upload(D, stage.data(), stage.size(), &d_stage, s);
    if (r) return r;
    uint8_t* d_scratch = nullptr;  // [mark: a word a peer][left: the same, unless quota_left_out]
    if (scratch_alloc(D, &d_scratch, 4 * peer * (quota_left_out ? 1 : 2) + 8, s) != hipSuccess) {
        scratch_free(D, d_stage, s);
        set_error(KRK_ENOMEM, "piece_resend_round_dev: mark and quota scratch");
        return KRK_ENOMEM;
    }
    uint32_t* mark = reinterpret_cast<uint32_t*>(d_scratch);
    int32_t* left = quota_left_out ? quota_left_out : reinterpret_cast<int32_t*>(d_scratch + 4 * peer);
    const hipError_t e = timed(K_PIECERESEND, s, [&] {
        return launch_piece_resend(static_cast<const RsTorrent*>(d_stage), n_torrents, bits_dev, quota_dev,
                                   reinterpret_cast<const rs::Failed*>(static_cast<const uint8_t*>(d_stage) + list_at), left,
                                   mark, target_out, n_resent_out, s);
    });
    scratch_free(D, d_scratch, s);
    scratch_free(D, d_stage, s);
    KRK_CHECK(e == hipSuccess, KRK_EHIP, "piece_resend launch: %s", launch_error_text(e));
    return KRK_OK;
}

int krk_piece_resend_geometry(uint64_t* peers_per_pass) {
    KRK_CHECK(peers_per_pass, KRK_EINVAL, "piece_resend_geometry: null argument");
    *peers_per_pass = kRsS;
    return KRK_OK;
}

}  // extern "C"
