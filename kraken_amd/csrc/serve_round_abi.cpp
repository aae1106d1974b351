// serve_round_abi.cpp -- serve rounds: the seeder's side of the resident rows, every queued piece
// request of a batch of torrents answered in arrival order.  The host form (krk_serve_round:
// serve_round_math.hpp on the calling thread, no device) and the device form (krk_serve_round_dev,
// serve_round.hip computing the same state and outputs).
#include "serve_round_math.hpp"
#include "runtime.hpp"

using namespace krk;

static_assert(sizeof(sv::Request) == sizeof(krk_serve_request) && offsetof(sv::Request, peer) == offsetof(krk_serve_request, peer) &&
                  offsetof(sv::Request, index) == offsetof(krk_serve_request, index) &&
                  offsetof(sv::Request, offset) == offsetof(krk_serve_request, offset) &&
                  offsetof(sv::Request, length) == offsetof(krk_serve_request, length),
              "sv::Request is krk_serve_request");
static_assert(sizeof(krk_serve_torrent) == 40, "krk_serve_torrent layout");
static_assert(sv::kOk == KRK_SV_OK && sv::kChunk == KRK_SV_CHUNK && sv::kIndex == KRK_SV_INDEX &&
                  sv::kIncomplete == KRK_SV_INCOMPLETE && sv::kGone == KRK_SV_GONE && sv::kMaxRequests == KRK_SV_MAX_REQUESTS &&
                  kSvTile == KRK_SV_MAX_REQUESTS,
              "serve_round_math.hpp, kernels.hpp and kraken_hip.h name the same values");

namespace {

constexpr uint64_t kMaxOff = 1ull << 48;  // an offset past it is an error, and no sum below overflows

// What a round touches of each array, in elements (0 when nothing is), and the lists' lengths added up.
struct Extent {
    uint64_t bits = 0, peers = 0, live = 0, reqs = 0;  // extents of the callers' arrays
    uint64_t n_live = 0, n_reqs = 0;                   // sums
};

// The checks both forms share, the request lists included; *x the batch's extents.
int check_round(const char* who, const krk_request_torrent* t, const krk_serve_torrent* b, uint64_t n, const uint64_t* live,
                const krk_serve_request* reqs, int64_t now, Extent* x) {
    KRK_CHECK(!n || (t && b), KRK_EINVAL, "%s: torrents or serves is NULL", who);
    KRK_CHECK(now >= 0, KRK_EINVAL, "%s: a negative now", who);
    for (uint64_t k = 0; k < n; ++k) {
        const unsigned long long kk = k;
        const char* why = sv::torrent_error(t[k].n_pieces, t[k].n_peers, b[k].length, b[k].piece_length, b[k].n_reqs);
        KRK_CHECK(!why, KRK_EINVAL, "%s: torrent %llu: %s", who, kk, why);
        KRK_CHECK(!b[k].reserved, KRK_EINVAL, "%s: torrent %llu: a non-zero reserved field", who, kk);
        KRK_CHECK(t[k].bits_off < kMaxOff && t[k].peer_off < kMaxOff && b[k].live_off < kMaxOff && b[k].req_off < kMaxOff,
                  KRK_EINVAL, "%s: torrent %llu: an offset of 2^48 or more", who, kk);
        const uint64_t W = pr::words(t[k].n_pieces), P = t[k].n_peers, L = (P + 63) / 64;
        if (W) x->bits = std::max(x->bits, t[k].bits_off + (1 + 2 * P) * W);
        if (P) x->peers = std::max(x->peers, t[k].peer_off + P), x->live = std::max(x->live, b[k].live_off + L);
        if (b[k].n_reqs) x->reqs = std::max(x->reqs, b[k].req_off + b[k].n_reqs);
        x->n_live += L, x->n_reqs += b[k].n_reqs;
    }
    KRK_CHECK(x->n_reqs < (1ull << 32), KRK_EINVAL, "%s: %llu requests in one call (2^32 or more)", who,
              (unsigned long long)x->n_reqs);
    KRK_CHECK((live || !x->live) && (reqs || !x->reqs), KRK_EINVAL, "%s: live or requests is NULL", who);
    for (uint64_t k = 0; k < n; ++k)
        for (uint32_t r = 0; r < b[k].n_reqs; ++r)
            KRK_CHECK(reqs[b[k].req_off + r].peer < t[k].n_peers, KRK_EINVAL,
                      "%s: torrent %llu, request %u: a peer that is not one of the torrent's slots", who, (unsigned long long)k, r);
    return KRK_OK;
}

// The NULL rules of the arrays both forms share.
bool nulls_ok(const Extent& x, uint64_t n, uint64_t token_size, const void* bits, const void* status, const void* file_off,
              const void* len, const void* send_off, const void* token_off, const void* n_received, const void* n_sent,
              const void* sent, const void* n_ok, const void* bytes, const void* tokens) {
    return (bits || !x.bits) && (!x.reqs || (status && file_off && len && send_off && (token_off || !token_size))) &&
           (!x.peers || (n_received && n_sent && sent)) && (!n || (n_ok && bytes && (tokens || !token_size)));
}

}  // namespace

extern "C" {

int krk_serve_round(const krk_request_torrent* torrents, const krk_serve_torrent* serves, uint64_t n_torrents, uint64_t* bits,
                    const uint64_t* live, const krk_serve_request* requests, int64_t now, uint64_t token_size,
                    uint32_t* status_out, int64_t* file_off_out, uint32_t* len_out, uint64_t* send_off_out,
                    uint64_t* token_off_out, uint32_t* n_received_out, uint32_t* n_sent_out, int64_t* sent,
                    uint32_t* n_ok_out, uint64_t* bytes_out, uint64_t* tokens_out) {
    Extent x;
    const int r = check_round("serve_round", torrents, serves, n_torrents, live, requests, now, &x);
    if (r) return r;
    KRK_CHECK(nulls_ok(x, n_torrents, token_size, bits, status_out, file_off_out, len_out, send_off_out, token_off_out,
                       n_received_out, n_sent_out, sent, n_ok_out, bytes_out, tokens_out),
              KRK_EINVAL, "serve_round: null argument");
    for (uint64_t k = 0; k < n_torrents; ++k) {
        const krk_request_torrent& T = torrents[k];
        const krk_serve_torrent& S = serves[k];
        const bool P = T.n_peers != 0, R = S.n_reqs != 0;
        const sv::Totals o = sv::round_torrent(
            x.bits ? bits + T.bits_off : nullptr, T.n_pieces, T.n_peers, P ? live + S.live_off : nullptr, S.length, S.piece_length,
            R ? reinterpret_cast<const sv::Request*>(requests) + S.req_off : nullptr, S.n_reqs, now, token_size,
            R ? status_out + S.req_off : nullptr, R ? file_off_out + S.req_off : nullptr, R ? len_out + S.req_off : nullptr,
            R ? send_off_out + S.req_off : nullptr, R && token_size ? token_off_out + S.req_off : nullptr,
            P ? n_received_out + T.peer_off : nullptr, P ? n_sent_out + T.peer_off : nullptr, P ? sent + T.peer_off : nullptr);
        n_ok_out[k] = o.n_ok, bytes_out[k] = o.bytes;
        if (token_size) tokens_out[k] = o.tokens;
    }
    return KRK_OK;
}

int krk_serve_round_dev(const krk_request_torrent* torrents_host, const krk_serve_torrent* serves_host, uint64_t n_torrents,
                        uint64_t* bits_dev, const uint64_t* live_host, const krk_serve_request* requests_host, int64_t now,
                        uint64_t token_size, uint32_t* status_out, int64_t* file_off_out, uint32_t* len_out,
                        uint64_t* send_off_out, uint64_t* token_off_out, uint32_t* n_received_out, uint32_t* n_sent_out,
                        int64_t* sent_dev, uint32_t* n_ok_out, uint64_t* bytes_out, uint64_t* tokens_out, void* stream) {
    Extent x;
    int r = check_round("serve_round_dev", torrents_host, serves_host, n_torrents, live_host, requests_host, now, &x);
    if (r) return r;
    KRK_CHECK(nulls_ok(x, n_torrents, token_size, bits_dev, status_out, file_off_out, len_out, send_off_out, token_off_out,
                       n_received_out, n_sent_out, sent_dev, n_ok_out, bytes_out, tokens_out),
              KRK_EINVAL, "serve_round_dev: null argument");
    KRK_CHECK(n_torrents <= 0x7FFFFFFFull, KRK_ERANGE, "serve_round_dev: %llu torrents in one call",
              (unsigned long long)n_torrents);
    if (!n_torrents) return KRK_OK;
    KRK_DEVICE(D);
    if (!token_size) token_off_out = nullptr, tokens_out = nullptr;  // not asked for: never read
    KRK_CHECK(!(((uintptr_t)bits_dev | (uintptr_t)file_off_out | (uintptr_t)send_off_out | (uintptr_t)token_off_out |
                 (uintptr_t)sent_dev | (uintptr_t)bytes_out | (uintptr_t)tokens_out) &
                7) &&
                  !(((uintptr_t)status_out | (uintptr_t)len_out | (uintptr_t)n_received_out | (uintptr_t)n_sent_out |
                     (uintptr_t)n_ok_out) &
                    3),
              KRK_EINVAL, "serve_round_dev: bits_dev, sent_dev and the 64-bit outputs must be 8-byte, the uint32 outputs 4-byte aligned");
    KRK_CHECK((!x.bits || device_writable(bits_dev, 8 * x.bits)) &&
                  (!x.reqs || (device_writable(status_out, 4 * x.reqs) && device_writable(file_off_out, 8 * x.reqs) &&
                               device_writable(len_out, 4 * x.reqs) && device_writable(send_off_out, 8 * x.reqs) &&
                               (!token_size || device_writable(token_off_out, 8 * x.reqs)))) &&
                  (!x.peers || (device_writable(n_received_out, 4 * x.peers) && device_writable(n_sent_out, 4 * x.peers) &&
                                device_writable(sent_dev, 8 * x.peers))) &&
                  device_writable(n_ok_out, 4 * n_torrents) && device_writable(bytes_out, 8 * n_torrents) &&
                  (!token_size || device_writable(tokens_out, 8 * n_torrents)),
              KRK_EINVAL, "serve_round_dev: bits_dev, sent_dev and the outputs must be device memory or page-locked host memory");
    hipStream_t s = pick(D, stream);
    // One staged block: the torrents, the requests (16-byte aligned behind them), the live words, each
    // packed torrent after torrent.
    static_assert(sizeof(SvTorrent) % 16 == 0, "the requests stay 16-byte aligned");
    const size_t req_at = n_torrents * sizeof(SvTorrent), live_at = req_at + sizeof(sv::Request) * x.n_reqs;
    std::vector<uint8_t> stage(live_at + 8 * x.n_live);
    SvTorrent* tors = reinterpret_cast<SvTorrent*>(stage.data());
    uint64_t q = 0, l = 0;
    for (uint64_t k = 0; k < n_torrents; ++k) {
        const krk_request_torrent& T = torrents_host[k];
        const krk_serve_torrent& S = serves_host[k];
        const uint64_t L = ((uint64_t)T.n_peers + 63) / 64;
        tors[k] = {T.n_pieces, T.bits_off, T.peer_off, S.req_off, S.length, S.piece_length, q, l, T.n_peers, S.n_reqs, 0};
        if (S.n_reqs) memcpy(stage.data() + req_at + sizeof(sv::Request) * q, requests_host + S.req_off, sizeof(sv::Request) * S.n_reqs);
        if (L) memcpy(stage.data() + live_at + 8 * l, live_host + S.live_off, 8 * L);
        q += S.n_reqs, l += L;
    }
    void* d_stage = nullptr;  // copied into the library's pinned staging before this returns
    r = upload(D, stage.data(), stage.size(), &d_stage, s);
    if (r) return r;
    const uint8_t* ds = static_cast<const uint8_t*>(d_stage);
    const SvArrays A = {bits_dev,       status_out, file_off_out, len_out,  send_off_out, token_off_out,
                        n_received_out, n_sent_out, sent_dev,     n_ok_out, bytes_out,    tokens_out};
    const hipError_t e = timed(K_SERVEROUND, s, [&] {
        return launch_serve_round(reinterpret_cast<const SvTorrent*>(ds), n_torrents, reinterpret_cast<const sv::Request*>(ds + req_at),
                                  reinterpret_cast<const uint64_t*>(ds + live_at), now, token_size, A, s);
    });
    scratch_free(D, d_stage, s);
    KRK_CHECK(e == hipSuccess, KRK_EHIP, "serve_round launch: %s", launch_error_text(e));
    return KRK_OK;
}

int krk_serve_round_geometry(uint64_t* chunk, uint64_t* tile) {
    KRK_CHECK(chunk && tile, KRK_EINVAL, "serve_round_geometry: null argument");
    *chunk = kSvChunk;
    *tile = kSvTile;
    return KRK_OK;
}

}  // extern "C"
