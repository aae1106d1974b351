// serve_round_math.hpp -- one serve round over the rows of a request round (krk_serve_round): the
// upload side of the resident state, Dispatcher.handlePieceRequest
// (lib/torrent/scheduler/dispatch/dispatcher.go:504-530) for every queued PieceRequestMessage of a
// torrent, in arrival order.  With plen(i) = MetaInfo.GetPieceLength(i) (core/metainfo.go:109-118:
// 0 outside [0, n), the remainder for the last piece), request r takes the first status that applies:
//   kChunk       offset != 0 or (int64)length != plen(index)              (isFullPiece, :500-502)
//   kIndex       index < 0 or index >= n -- reached only with offset == length == 0
//                (GetPieceReader's "invalid piece index", agentstorage/torrent.go:260-269; for a
//                negative index the reference indexes out of range and panics: here it is a status)
//   kIncomplete  bit index of have is clear                               ("piece not complete")
//   kGone        the slot's live bit is clear: the send fails, nothing is touched
//   kOk          the payload is sent: file offset piece_length * index (getFileOffset, :293-295),
//                the slot's LastPieceSent touched, bit index of bits_p set ("Assume that the peer
//                successfully received the piece"), max(len * 8 / token_size, 1) egress tokens
//                reserved (conn/conn.go:254-261, utils/bandwidth/limiter.go:100-117).
// The OK payloads lie end to end in arrival order: send_off and token_off are the running sums
// before the request.  numPeersByPiece is the rows' column sum here, so a served bit counts in the
// next request round, where the reference never bumps it.  Header-only and free of the runtime;
// serve_round.hip computes the same state and outputs.
#pragma once
#include <stdint.h>

#include "piece_request_math.hpp"

namespace krk {
namespace sv {

constexpr uint32_t kOk = 0, kChunk = 1, kIndex = 2, kIncomplete = 3, kGone = 4;  // KRK_SV_*
constexpr uint32_t kMaxRequests = 4096;                                          // KRK_SV_MAX_REQUESTS
constexpr uint32_t kMaxPeers = 1u << 30;  // a slot and the pad key both fit the sort key

struct Request {  // krk_serve_request
    uint32_t peer;
    int32_t index, offset, length;
};

// GetPieceLength(index) of a torrent of n pieces.
KRK_PR_HD inline int64_t piece_len(int32_t index, uint64_t n, int64_t length, int64_t piece_length) {
    if (index < 0 || (uint64_t)index >= n) return 0;
    return (uint64_t)index + 1 == n ? length - piece_length * (int64_t)index : piece_length;
}
// What the request's three fields decide alone: kChunk, kIndex or kOk (the rows decide the rest).
KRK_PR_HD inline uint32_t shape_status(const Request& q, uint64_t n, int64_t length, int64_t piece_length) {
    if (q.offset != 0 || (int64_t)q.length != piece_len(q.index, n, length, piece_length)) return kChunk;
    if (q.index < 0 || (uint64_t)q.index >= n) return kIndex;
    return kOk;
}
KRK_PR_HD inline uint32_t status(uint32_t shape, bool have, bool live) {
    return shape ? shape : !have ? kIncomplete : !live ? kGone : kOk;
}
// The egress tokens of a payload of len bytes; token_size > 0.
KRK_PR_HD inline uint64_t tokens(uint32_t len, uint64_t token_size) {
    const uint64_t t = (uint64_t)len * 8 / token_size;
    return t ? t : 1;
}

// What is wrong with a torrent's shape, or nullptr.
inline const char* torrent_error(uint64_t n, uint32_t n_peers, int64_t length, int64_t piece_length, uint64_t n_reqs) {
    if (n >= (1ull << 32)) return "2^32 pieces or more";
    if (n_peers > kMaxPeers) return "more than 2^30 peer slots";
    if (piece_length <= 0) return "piece length must be positive";
    if (length < 0) return "a negative length";
    if (n != ((uint64_t)length + (uint64_t)piece_length - 1) / (uint64_t)piece_length)
        return "n_pieces is not krk_num_pieces(length, piece_length)";
    if (n_reqs > kMaxRequests) return "more than 4,096 requests";
    return nullptr;
}

struct Totals {
    uint32_t n_ok;
    uint64_t bytes, tokens;
};

// One torrent's round: rows as a request round's (nullptr when W is 0), live its live words, reqs
// valid (every peer < n_peers).  The per-request outputs start at the torrent's first request, the
// per-slot ones at its first slot; token_off is written iff token_size > 0.
inline Totals round_torrent(uint64_t* rows, uint64_t n, uint32_t n_peers, const uint64_t* live, int64_t length,
                            int64_t piece_length, const Request* reqs, uint32_t n_reqs, int64_t now, uint64_t token_size,
                            uint32_t* status_out, int64_t* file_off, uint32_t* len_out, uint64_t* send_off,
                            uint64_t* token_off, uint32_t* n_received, uint32_t* n_sent, int64_t* sent) {
    const uint64_t W = pr::words(n);
    Totals t = {0, 0, 0};
    for (uint32_t p = 0; p < n_peers; ++p) n_received[p] = n_sent[p] = 0;
    for (uint32_t r = 0; r < n_reqs; ++r) {
        const Request& q = reqs[r];
        const uint32_t shape = shape_status(q, n, length, piece_length);
        const bool have = !shape && ((rows[(uint32_t)q.index >> 6] >> (q.index & 63)) & 1);
        const uint32_t st = status(shape, have, (live[q.peer >> 6] >> (q.peer & 63)) & 1);
        const bool ok = st == kOk;
        const uint32_t len = ok ? (uint32_t)q.length : 0;
        status_out[r] = st;
        file_off[r] = ok ? piece_length * (int64_t)q.index : 0;
        len_out[r] = len;
        send_off[r] = ok ? t.bytes : 0;
        if (token_size) token_off[r] = ok ? t.tokens : 0;
        ++n_received[q.peer];
        if (!ok) continue;
        ++t.n_ok, t.bytes += len;
        if (token_size) t.tokens += tokens(len, token_size);
        ++n_sent[q.peer];
        sent[q.peer] = now;
        rows[(1 + 2 * (uint64_t)q.peer) * W + ((uint32_t)q.index >> 6)] |= 1ull << (q.index & 63);
    }
    return t;
}

}  // namespace sv
}  // namespace krk
