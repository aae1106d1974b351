// receive_round_abi.cpp -- receive rounds: the download side's arrival step on the resident rows,
// every queued piece payload of a batch of torrents judged in arrival order.  The host form
// (krk_receive_round: receive_round_math.hpp on the calling thread, no device) and the device form
// (krk_receive_round_dev, receive_round.hip computing the same state and outputs).
#include "receive_round_math.hpp"
#include "runtime.hpp"

using namespace krk;

static_assert(sizeof(krk_receive_torrent) == 40, "krk_receive_torrent layout");
static_assert(sizeof(rv::Mark) == sizeof(krk_failed_request) && offsetof(rv::Mark, piece) == offsetof(krk_failed_request, piece) &&
                  offsetof(rv::Mark, peer) == offsetof(krk_failed_request, peer) &&
                  offsetof(rv::Mark, status) == offsetof(krk_failed_request, status),
              "rv::Mark is krk_failed_request");
static_assert(rv::kOk == KRK_RV_OK && rv::kChunk == KRK_RV_CHUNK && rv::kIndex == KRK_RV_INDEX &&
                  rv::kDuplicate == KRK_RV_DUPLICATE && rv::kBadSum == KRK_RV_BAD_SUM && rv::kComplete == KRK_RV_COMPLETE &&
                  rv::kCompletedNow == KRK_RV_COMPLETED_NOW && rv::kMaxPayloads == KRK_RV_MAX_PAYLOADS &&
                  kRvTile == KRK_RV_MAX_PAYLOADS && rv::kNone == KRK_PR_NONE && rv::kInvalid == KRK_PR_INVALID,
              "receive_round_math.hpp, kernels.hpp and kraken_hip.h name the same values");

namespace {

constexpr uint64_t kMaxOff = 1ull << 48;  // an offset past it is an error, and no sum below overflows

// What a round touches of each array, in elements (0 when nothing is), and the lists' lengths added up.
struct Extent {
    uint64_t bits = 0, peers = 0, sums = 0, pays = 0;  // extents of the callers' arrays
    uint64_t n_pays = 0;                               // sum
};

// The checks both forms share, the payload lists included; *x the batch's extents.
int check_round(const char* who, const krk_request_torrent* t, const krk_receive_torrent* b, uint64_t n,
                const krk_serve_request* pays, int64_t now, Extent* x) {
    KRK_CHECK(!n || (t && b), KRK_EINVAL, "%s: torrents or receives is NULL", who);
    KRK_CHECK(now >= 0, KRK_EINVAL, "%s: a negative now", who);
    for (uint64_t k = 0; k < n; ++k) {
        const unsigned long long kk = k;
        const char* why = rv::torrent_error(t[k].n_pieces, t[k].n_peers, b[k].length, b[k].piece_length, b[k].n_pays);
        KRK_CHECK(!why, KRK_EINVAL, "%s: torrent %llu: %s", who, kk, why);
        KRK_CHECK(!b[k].reserved, KRK_EINVAL, "%s: torrent %llu: a non-zero reserved field", who, kk);
        KRK_CHECK(t[k].bits_off < kMaxOff && t[k].peer_off < kMaxOff && b[k].sum_off < kMaxOff && b[k].pay_off < kMaxOff,
                  KRK_EINVAL, "%s: torrent %llu: an offset of 2^48 or more", who, kk);
        const uint64_t W = pr::words(t[k].n_pieces), P = t[k].n_peers;
        if (W) x->bits = std::max(x->bits, t[k].bits_off + W), x->sums = std::max(x->sums, b[k].sum_off + t[k].n_pieces);
        if (P) x->peers = std::max(x->peers, t[k].peer_off + P);
        if (b[k].n_pays) x->pays = std::max(x->pays, b[k].pay_off + b[k].n_pays);
        x->n_pays += b[k].n_pays;
    }
    KRK_CHECK(x->n_pays < (1ull << 32), KRK_EINVAL, "%s: %llu payloads in one call (2^32 or more)", who,
              (unsigned long long)x->n_pays);
    KRK_CHECK(pays || !x->pays, KRK_EINVAL, "%s: payloads is NULL", who);
    for (uint64_t k = 0; k < n; ++k)
        for (uint32_t r = 0; r < b[k].n_pays; ++r) {
            const uint32_t p = pays[b[k].pay_off + r].peer;
            KRK_CHECK(p < t[k].n_peers || p == KRK_PR_NONE, KRK_EINVAL,
                      "%s: torrent %llu, payload %u: a peer that is neither one of the torrent's slots nor 0xFFFFFFFF (left)", who,
                      (unsigned long long)k, r);
        }
    return KRK_OK;
}

// The NULL rules of the arrays both forms share; o: the thirteen outputs in the call's order.
bool nulls_ok(const Extent& x, uint64_t n, const void* bits, const void* sums, const void* expected, void* const o[13]) {
    return (bits || !x.bits) && (expected || !x.sums) && (!x.pays || (sums && o[0] && o[1] && o[2] && o[3] && o[4])) &&
           (!x.peers || (o[5] && o[6] && o[7])) && (!n || (o[8] && o[9] && o[10] && o[11] && o[12]));
}

}  // namespace

extern "C" {

int krk_receive_round(const krk_request_torrent* torrents, const krk_receive_torrent* receives, uint64_t n_torrents,
                      uint64_t* bits, const krk_serve_request* payloads, const uint32_t* sums, const uint32_t* expected,
                      int64_t now, uint32_t* status_out, int64_t* file_off_out, uint32_t* arrived_out,
                      uint32_t* arrived_from_out, krk_failed_request* marks_out, uint32_t* n_good_out,
                      uint32_t* n_duplicate_out, int64_t* received, uint32_t* n_arrived_out, uint32_t* n_marks_out,
                      uint32_t* n_complete_out, uint64_t* bytes_out, uint32_t* flags_out) {
    Extent x;
    const int r = check_round("receive_round", torrents, receives, n_torrents, payloads, now, &x);
    if (r) return r;
    void* const outs[13] = {status_out, file_off_out,  arrived_out, arrived_from_out, marks_out,      n_good_out, n_duplicate_out,
                            received,   n_arrived_out, n_marks_out, n_complete_out,   bytes_out,      flags_out};
    KRK_CHECK(nulls_ok(x, n_torrents, bits, sums, expected, outs), KRK_EINVAL, "receive_round: null argument");
    for (uint64_t k = 0; k < n_torrents; ++k) {
        const krk_request_torrent& T = torrents[k];
        const krk_receive_torrent& S = receives[k];
        const bool P = T.n_peers != 0, R = S.n_pays != 0;
        const rv::Totals o = rv::round_torrent(
            T.n_pieces ? bits + T.bits_off : nullptr, T.n_pieces, T.n_peers, S.length, S.piece_length,
            R ? reinterpret_cast<const sv::Request*>(payloads) + S.pay_off : nullptr, R ? sums + S.pay_off : nullptr,
            T.n_pieces ? expected + S.sum_off : nullptr, S.n_pays, now, R ? status_out + S.pay_off : nullptr,
            R ? file_off_out + S.pay_off : nullptr, R ? arrived_out + S.pay_off : nullptr,
            R ? arrived_from_out + S.pay_off : nullptr, R ? reinterpret_cast<rv::Mark*>(marks_out) + S.pay_off : nullptr,
            P ? n_good_out + T.peer_off : nullptr, P ? n_duplicate_out + T.peer_off : nullptr, P ? received + T.peer_off : nullptr);
        n_arrived_out[k] = o.n_arrived, n_marks_out[k] = o.n_marks, n_complete_out[k] = o.n_complete;
        bytes_out[k] = o.bytes, flags_out[k] = o.flags;
    }
    return KRK_OK;
}

int krk_receive_round_dev(const krk_request_torrent* torrents_host, const krk_receive_torrent* receives_host,
                          uint64_t n_torrents, uint64_t* bits_dev, const krk_serve_request* payloads_host,
                          const uint32_t* sums_dev, const uint32_t* expected_dev, int64_t now, uint32_t* status_out,
                          int64_t* file_off_out, uint32_t* arrived_out, uint32_t* arrived_from_out,
                          krk_failed_request* marks_out, uint32_t* n_good_out, uint32_t* n_duplicate_out,
                          int64_t* received_dev, uint32_t* n_arrived_out, uint32_t* n_marks_out, uint32_t* n_complete_out,
                          uint64_t* bytes_out, uint32_t* flags_out, void* stream) {
    Extent x;
    int r = check_round("receive_round_dev", torrents_host, receives_host, n_torrents, payloads_host, now, &x);
    if (r) return r;
    void* const outs[13] = {status_out,   file_off_out,  arrived_out, arrived_from_out, marks_out, n_good_out, n_duplicate_out,
                            received_dev, n_arrived_out, n_marks_out, n_complete_out,   bytes_out, flags_out};
    KRK_CHECK(nulls_ok(x, n_torrents, bits_dev, sums_dev, expected_dev, outs), KRK_EINVAL, "receive_round_dev: null argument");
    KRK_CHECK(n_torrents <= 0x7FFFFFFFull, KRK_ERANGE, "receive_round_dev: %llu torrents in one call",
              (unsigned long long)n_torrents);
    if (!n_torrents) return KRK_OK;
    KRK_DEVICE(D);
    KRK_CHECK(!(((uintptr_t)bits_dev | (uintptr_t)file_off_out | (uintptr_t)received_dev | (uintptr_t)bytes_out) & 7) &&
                  !(((uintptr_t)sums_dev | (uintptr_t)expected_dev | (uintptr_t)status_out | (uintptr_t)arrived_out |
                     (uintptr_t)arrived_from_out | (uintptr_t)marks_out | (uintptr_t)n_good_out | (uintptr_t)n_duplicate_out |
                     (uintptr_t)n_arrived_out | (uintptr_t)n_marks_out | (uintptr_t)n_complete_out | (uintptr_t)flags_out) &
                    3),
              KRK_EINVAL,
              "receive_round_dev: bits_dev, received_dev and the 64-bit outputs must be 8-byte, the uint32 arrays 4-byte aligned");
    KRK_CHECK((!x.bits || device_writable(bits_dev, 8 * x.bits)) && (!x.sums || device_writable(expected_dev, 4 * x.sums)) &&
                  (!x.pays || (device_writable(sums_dev, 4 * x.pays) && device_writable(status_out, 4 * x.pays) &&
                               device_writable(file_off_out, 8 * x.pays) && device_writable(arrived_out, 4 * x.pays) &&
                               device_writable(arrived_from_out, 4 * x.pays) && device_writable(marks_out, 12 * x.pays))) &&
                  (!x.peers || (device_writable(n_good_out, 4 * x.peers) && device_writable(n_duplicate_out, 4 * x.peers) &&
                                device_writable(received_dev, 8 * x.peers))) &&
                  device_writable(n_arrived_out, 4 * n_torrents) && device_writable(n_marks_out, 4 * n_torrents) &&
                  device_writable(n_complete_out, 4 * n_torrents) && device_writable(bytes_out, 8 * n_torrents) &&
                  device_writable(flags_out, 4 * n_torrents),
              KRK_EINVAL,
              "receive_round_dev: bits_dev, sums_dev, expected_dev, received_dev and the outputs must be device memory or "
              "page-locked host memory");
    hipStream_t s = pick(D, stream);
    // One staged block: the torrents, then the payloads (16-byte aligned behind them), packed torrent
    // after torrent.
    static_assert(sizeof(RvTorrent) % 16 == 0, "the payloads stay 16-byte aligned");
    const size_t pay_at = n_torrents * sizeof(RvTorrent);
    std::vector<uint8_t> stage(pay_at + sizeof(sv::Request) * x.n_pays);
    RvTorrent* tors = reinterpret_cast<RvTorrent*>(stage.data());
    uint64_t q = 0;
    for (uint64_t k = 0; k < n_torrents; ++k) {
        const krk_request_torrent& T = torrents_host[k];
        const krk_receive_torrent& S = receives_host[k];
        tors[k] = {T.n_pieces, T.bits_off, T.peer_off, S.pay_off, S.sum_off, S.length, S.piece_length, q, T.n_peers, S.n_pays};
        if (S.n_pays) memcpy(stage.data() + pay_at + sizeof(sv::Request) * q, payloads_host + S.pay_off, sizeof(sv::Request) * S.n_pays);
        q += S.n_pays;
    }
    void* d_stage = nullptr;  // copied into the library's pinned staging before this returns
    r = upload(D, stage.data(), stage.size(), &d_stage, s);
    if (r) return r;
    const uint8_t* ds = static_cast<const uint8_t*>(d_stage);
    const RvArrays A = {bits_dev,    sums_dev,         expected_dev,                       received_dev, status_out,
                        file_off_out, arrived_out,     arrived_from_out,                   reinterpret_cast<rv::Mark*>(marks_out),
                        n_good_out,  n_duplicate_out,  n_arrived_out,                      n_marks_out,  n_complete_out,
                        bytes_out,   flags_out};
    const hipError_t e = timed(K_RECEIVEROUND, s, [&] {
        return launch_receive_round(reinterpret_cast<const RvTorrent*>(ds), n_torrents,
                                    reinterpret_cast<const sv::Request*>(ds + pay_at), now, A, s);
    });
    scratch_free(D, d_stage, s);
    KRK_CHECK(e == hipSuccess, KRK_EHIP, "receive_round launch: %s", launch_error_text(e));
    return KRK_OK;
}

int krk_receive_round_geometry(uint64_t* chunk, uint64_t* tile) {
    KRK_CHECK(chunk && tile, KRK_EINVAL, "receive_round_geometry: null argument");
    *chunk = kRvChunk;
    *tile = kRvTile;
    return KRK_OK;
}

}  // extern "C"
