// receive_round_math.hpp -- one receive round over the rows of a request round (krk_receive_round):
// the download side's arrival step, Dispatcher.handlePiecePayload
// (lib/torrent/scheduler/dispatch/dispatcher.go:532-577) with Torrent.WritePiece
// (agentstorage/torrent.go:202-248) for every queued PiecePayloadMessage of a torrent, in arrival
// order at one clock instant.  sums[r] is the CRC-32 of payload r's bytes, expected[i] the
// MetaInfo's sum of piece i.  With plen(i) as in serve_round_math.hpp, payload r takes the first
// status that applies:
//   kChunk      offset != 0 or (int64)length != plen(index)   (isFullPiece; MarkInvalid(peer, index)
//               follows: a mark iff 0 <= index < n and the sender is known -- outside the range no
//               table entry can exist)
//   kIndex      index outside [0, n), reached only with offset == length == 0 (getPiece's "invalid
//               piece index"; a negative index is a status here, not a panic).  No mark.
//   kDuplicate  bit index of have was set when the round began, or an earlier payload of the round
//               was kOk for the piece (ErrPieceComplete, tested before the sum is looked at:
//               incrementDuplicatePiecesReceived).  No mark.
//   kBadSum     sums[r] != expected[index] ("invalid piece sum").  A mark unless the sender is
//               kNone; the piece stays empty, so a later payload of it can still be kOk.
//   kOk         the piece is written: incrementGoodPiecesReceived, touchLastGoodPieceReceived, the
//               bit set in have, Clear(index) (the arrived list of the next table round).
// A sender of kNone has left since: its piece is still judged and written, attributed to nobody and
// marked against nobody.  The live bit is not read: the reference's feed loop dispatches every
// message that arrived before the close.  errWritePieceConflict cannot arise: a round is one
// instant and its writes are serial, so no piece is ever dirty when the next payload looks at it.
// Header-only and free of the runtime; receive_round.hip computes the same state and outputs.
#pragma once
#include <stdint.h>

#include "have_round_math.hpp"
#include "serve_round_math.hpp"

namespace krk {
namespace rv {

constexpr uint32_t kOk = 0, kChunk = 1, kIndex = 2, kDuplicate = 3, kBadSum = 4;  // KRK_RV_*
constexpr uint32_t kComplete = 1, kCompletedNow = 2;                              // flags_out
constexpr uint32_t kMaxPayloads = 4096;                                           // KRK_RV_MAX_PAYLOADS
constexpr uint32_t kNone = 0xFFFFFFFFu;                                           // KRK_PR_NONE
constexpr uint32_t kInvalid = 3;                                                  // KRK_PR_INVALID

struct Mark {  // krk_failed_request
    uint32_t piece, peer, status;
};

// What the payload's three fields decide alone: kChunk, kIndex or kOk (full-shaped, index in [0, n)).
KRK_PR_HD inline uint32_t shape(const sv::Request& q, uint64_t n, int64_t length, int64_t piece_length) {
    const uint32_t s = sv::shape_status(q, n, length, piece_length);
    return s == sv::kChunk ? kChunk : s == sv::kIndex ? kIndex : kOk;
}
// A full-shaped payload r of a piece not held when the round began; `first` is the arrival index of
// the piece's first good-summed payload of that kind, read only when there is one (any_good).
KRK_PR_HD inline uint32_t resolve(uint32_t r, bool any_good, uint32_t first) {
    return !any_good || r < first ? kBadSum : r == first ? kOk : kDuplicate;
}
// MarkInvalid follows the payload and a table round would take the mark.
KRK_PR_HD inline bool marks(uint32_t st, const sv::Request& q, uint64_t n) {
    if (q.peer == kNone) return false;
    return st == kBadSum || (st == kChunk && q.index >= 0 && (uint64_t)q.index < n);
}
KRK_PR_HD inline uint32_t flags(uint64_t before, uint64_t after, uint64_t n) {
    return after == n ? kComplete | (before != n ? kCompletedNow : 0) : 0;
}

// What is wrong with a torrent's shape, or nullptr.
inline const char* torrent_error(uint64_t n, uint32_t n_peers, int64_t length, int64_t piece_length, uint64_t n_pays) {
    if (n_pays > kMaxPayloads) return "more than 4,096 payloads";
    return sv::torrent_error(n, n_peers, length, piece_length, 0);
}

struct Totals {
    uint32_t n_arrived, n_marks, n_complete, flags;
    uint64_t bytes;
};

// One torrent's round: have its row (W words, nullptr when W is 0), pays valid (every peer
// < n_peers or kNone), sums parallel to pays, expected the torrent's n sums.  The per-payload
// outputs and both lists start at the torrent's first payload, the per-slot ones at its first
// slot.  Of the lists only the first n_arrived / n_marks elements are stored.
inline Totals round_torrent(uint64_t* have, uint64_t n, uint32_t n_peers, int64_t length, int64_t piece_length,
                            const sv::Request* pays, const uint32_t* sums, const uint32_t* expected, uint32_t n_pays,
                            int64_t now, uint32_t* status_out, int64_t* file_off, uint32_t* arrived, uint32_t* arrived_from,
                            Mark* marks_out, uint32_t* n_good, uint32_t* n_duplicate, int64_t* received) {
    const uint64_t W = pr::words(n);
    uint64_t before = 0;
    for (uint64_t w = 0; w < W; ++w) before += (uint64_t)__builtin_popcountll(have[w] & pe::word_mask(n, w, W));
    Totals t = {0, 0, 0, 0, 0};
    for (uint32_t p = 0; p < n_peers; ++p) n_good[p] = n_duplicate[p] = 0;
    for (uint32_t r = 0; r < n_pays; ++r) {
        const sv::Request& q = pays[r];
        uint32_t st = shape(q, n, length, piece_length);
        if (st == kOk) {
            uint64_t& word = have[(uint32_t)q.index >> 6];
            const uint64_t bit = 1ull << (q.index & 63);
            if (word & bit) st = kDuplicate;
            else if (sums[r] != expected[q.index]) st = kBadSum;
            else word |= bit;
        }
        status_out[r] = st;
        file_off[r] = st == kOk ? piece_length * (int64_t)q.index : 0;
        if (marks(st, q, n)) marks_out[t.n_marks++] = {(uint32_t)q.index, q.peer, kInvalid};
        if (st == kDuplicate && q.peer != kNone) ++n_duplicate[q.peer];
        if (st != kOk) continue;
        if (q.peer != kNone) ++n_good[q.peer], received[q.peer] = now;
        uint32_t at = t.n_arrived++;  // kept ascending by piece: a piece is written once a round
        for (; at && arrived[at - 1] > (uint32_t)q.index; --at) arrived[at] = arrived[at - 1], arrived_from[at] = arrived_from[at - 1];
        arrived[at] = (uint32_t)q.index, arrived_from[at] = q.peer;
    }
    t.n_complete = (uint32_t)(before + t.n_arrived);
    t.flags = flags(before, before + t.n_arrived, n);
    t.bytes = hv::bytes_downloaded(before + t.n_arrived, piece_length, length);
    return t;
}

}  // namespace rv
}  // namespace krk
