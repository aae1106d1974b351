// request_table_math.hpp -- the piece request table of a torrent and one round over it
// (krk_request_table_round): piecerequest.Manager's `requests` and `requestsByPeer`
// (lib/torrent/scheduler/dispatch/piecerequest/manager.go) as one compact array of entries in
// recording order, beside the rows of a request round (piece_request_math.hpp).  Table order
// restricted to one piece is the order of requests[piece].  A round runs, in this order:
//   1 arrived  pieces, strictly ascending: the bit is set in have, every entry of the piece is
//              dropped (Manager.Clear, :163-178)
//   2 gone     peers, strictly ascending: every entry of the peer is dropped, its bits_p row zeroed
//   3 marks    (piece, peer, UNSENT | INVALID): every entry with that pair takes the status
//              (markStatus, :198-210); of two marks that hit one entry the later one stays
//   4 holds    (piece, peer), strictly ascending by (peer, piece): bit piece of bits_p is set
//              (handleAnnouncePiece, dispatch/dispatcher.go:488-496)
//   5 records  appended as pending with sent_at = now (ReservePieces' tail, :128-135): the explicit
//              pairs in order, then the picks of a request round, peer after peer; what does not
//              fit `cap`, and a pick >= n, is dropped and counted
//   6 derive   live(e) = pending && !(now > sent_at + timeout)              (expired, :212-215)
//              quota_p   = max(limit - #live entries of p, 0)               (requestQuota, :110-122)
//              blocked_p = the pieces with a live entry to p (allow-duplicates) or to anybody
//                          (validRequest, :224-236); every word of every blocked row is stored
//              failed    = every entry that is not live, a pending one as EXPIRED, ascending by
//                          piece and in table order inside a piece (GetFailedRequests, :139-161);
//                          they stay in the table
// One deliberate difference: ClearPeer (:180-196) ejects only the FIRST entry a piece and leaves
// the rest to block their pieces under a PeerID that no longer connects; `gone` drops them all.
// An entry nobody valid wrote -- piece >= n, peer >= n_peers, status > 3 -- is dropped with the
// removed, so no later step indexes with it.  Removal is stable.  Header-only and free of the
// runtime, so that tests/native/request_table_main.cpp builds it stand-alone under
// AddressSanitizer and UndefinedBehaviorSanitizer; request_table.hip computes the same state.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "piece_resend_math.hpp"

namespace krk {
namespace rt {

constexpr uint32_t kMaxEntries = 4096;  // KRK_RT_MAX_ENTRIES
constexpr uint32_t kPending = 0;

struct Entry {  // krk_request_entry
    uint32_t piece, peer, status, reserved;
    int64_t sent_at;
};
struct Pair {  // krk_request_pair
    uint32_t piece, peer;
};
struct Round {
    int64_t now, timeout;
    uint32_t limit;
};

// What is wrong with the round's scalars, or nullptr.
inline const char* round_error(const Round& r) {
    if (r.now < 0 || r.timeout < 0) return "a negative now or timeout";
    if (r.now > INT64_MAX - r.timeout) return "now + timeout past INT64_MAX";
    if (r.limit < 1 || r.limit > pr::kMaxLimit) return "a limit outside [1, 16]";
    return nullptr;
}
// live's clock test without the sum: now > sent_at + timeout, for any sent_at.
KRK_PR_HD inline bool expired(const Round& r, int64_t sent_at) { return sent_at < r.now - r.timeout; }
KRK_PR_HD inline bool live(const Round& r, uint32_t status, int64_t sent_at) {
    return status == kPending && !expired(r, sent_at);
}
// What the failed list reports of an entry that is not live.
KRK_PR_HD inline uint32_t failed_status(uint32_t status) { return status == kPending ? rs::kExpired : status; }
KRK_PR_HD inline bool entry_ok(uint32_t piece, uint32_t peer, uint32_t status, uint64_t n, uint32_t n_peers) {
    return piece < n && peer < n_peers && status <= rs::kInvalid;
}
// x is in the ascending list a[0, n).
KRK_PR_HD inline bool contains(const uint32_t* a, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && a[lo] == x;
}
// The status the marks leave on an entry (piece, peer) that had `status`.
KRK_PR_HD inline uint32_t marked(const rs::Failed* marks, uint32_t n_marks, uint32_t piece, uint32_t peer,
                                 uint32_t status) {
    for (uint32_t k = 0; k < n_marks; ++k)
        if (marks[k].piece == piece && marks[k].peer == peer) status = marks[k].status;
    return status;
}

// One torrent's five lists (n pieces, n_peers peers).
struct Lists {
    const uint32_t* arrived;
    const uint32_t* gone;
    const rs::Failed* marks;
    const Pair* holds;
    const Pair* records;
    uint32_t n_arrived, n_gone, n_marks, n_holds, n_records;
};
// What is wrong with them, or nullptr: *at is the element.
inline const char* lists_error(const Lists& l, uint64_t n, uint32_t n_peers, uint64_t* at) {
    for (uint32_t k = 0; k < l.n_arrived; ++k) {
        *at = k;
        if (l.arrived[k] >= n) return "an arrived piece past the torrent's last";
        if (k && l.arrived[k] <= l.arrived[k - 1]) return "arrived pieces that do not strictly ascend";
    }
    for (uint32_t k = 0; k < l.n_gone; ++k) {
        *at = k;
        if (l.gone[k] >= n_peers) return "a gone peer that is not one of the torrent's";
        if (k && l.gone[k] <= l.gone[k - 1]) return "gone peers that do not strictly ascend";
    }
    for (uint32_t k = 0; k < l.n_marks; ++k) {
        *at = k;
        if (l.marks[k].piece >= n || l.marks[k].peer >= n_peers) return "a mark's piece or peer out of range";
        if (l.marks[k].status != rs::kUnsent && l.marks[k].status != rs::kInvalid) return "a mark that is neither unsent nor invalid";
    }
    for (uint32_t k = 0; k < l.n_holds; ++k) {
        *at = k;
        const Pair a = l.holds[k];
        if (a.piece >= n || a.peer >= n_peers) return "a hold's piece or peer out of range";
        if (k) {
            const Pair b = l.holds[k - 1];
            if (a.peer < b.peer || (a.peer == b.peer && a.piece <= b.piece)) return "holds that do not strictly ascend by (peer, piece)";
        }
    }
    for (uint32_t k = 0; k < l.n_records; ++k) {
        *at = k;
        if (l.records[k].piece >= n || l.records[k].peer >= n_peers) return "a record's piece or peer out of range";
    }
    return nullptr;
}

// One torrent's round: rows = have, then (bits_p, blocked_p) a peer, W = words(n) words each;
// table: cap entries, *n_entries of them in use (<= cap); picks (rows of `limit`), n_picked and
// quota start at the torrent's first peer, picks and n_picked nullable together; failed (cap
// entries) and n_failed nullable together; keys: cap words of scratch.  The lists and the round
// are valid.  An n_picked above `limit` is read as `limit`.
inline void round_torrent(uint64_t* rows, uint64_t n, uint32_t n_peers, uint32_t flags, Entry* table,
                          uint32_t* n_entries, uint32_t cap, const Lists& l, const uint32_t* picks,
                          const uint32_t* n_picked, const Round& r, uint64_t* keys, int32_t* quota, rs::Failed* failed,
                          uint32_t* n_failed, uint32_t* n_dropped) {
    const uint64_t W = pr::words(n);
    const bool dup = (flags & pr::kAllowDuplicates) != 0;
    for (uint32_t k = 0; k < l.n_arrived; ++k) rows[l.arrived[k] >> 6] |= 1ull << (l.arrived[k] & 63);
    for (uint32_t k = 0; k < l.n_gone; ++k) {
        uint64_t* row = rows + (1 + 2 * (uint64_t)l.gone[k]) * W;
        for (uint64_t w = 0; w < W; ++w) row[w] = 0;
    }
    uint32_t m = 0;
    for (uint32_t e = 0; e < *n_entries; ++e) {
        Entry x = table[e];
        if (!entry_ok(x.piece, x.peer, x.status, n, n_peers) || contains(l.arrived, l.n_arrived, x.piece) ||
            contains(l.gone, l.n_gone, x.peer))
            continue;
        x.status = marked(l.marks, l.n_marks, x.piece, x.peer, x.status);
        table[m++] = x;
    }
    for (uint32_t k = 0; k < l.n_holds; ++k)
        rows[(1 + 2 * (uint64_t)l.holds[k].peer) * W + (l.holds[k].piece >> 6)] |= 1ull << (l.holds[k].piece & 63);
    uint32_t dropped = 0;
    auto record = [&](uint32_t piece, uint32_t peer) {
        if (m < cap) table[m++] = {piece, peer, kPending, 0, r.now};
        else ++dropped;
    };
    for (uint32_t k = 0; k < l.n_records; ++k) record(l.records[k].piece, l.records[k].peer);
    if (picks)
        for (uint32_t p = 0; p < n_peers; ++p)
            for (uint32_t j = 0; j < std::min(n_picked[p], r.limit); ++j) {
                const uint32_t i = picks[(uint64_t)p * r.limit + j];
                if (i < n) record(i, p);
                else ++dropped;
            }
    *n_entries = m;
    *n_dropped = dropped;
    // derive
    for (uint32_t p = 0; p < n_peers; ++p) {
        quota[p] = 0;  // the live entries, for now
        uint64_t* blocked = rows + (2 + 2 * (uint64_t)p) * W;
        for (uint64_t w = 0; w < W; ++w) blocked[w] = 0;
    }
    uint32_t nf = 0;
    for (uint32_t e = 0; e < m; ++e) {
        const Entry& x = table[e];
        if (live(r, x.status, x.sent_at)) {
            ++quota[x.peer];
            rows[(2 + 2 * (uint64_t)(dup ? x.peer : 0)) * W + (x.piece >> 6)] |= 1ull << (x.piece & 63);
        } else {
            keys[nf++] = (uint64_t)x.piece << 32 | e;
        }
    }
    if (!dup)
        for (uint32_t p = 1; p < n_peers; ++p) std::copy(rows + 2 * W, rows + 3 * W, rows + (2 + 2 * (uint64_t)p) * W);
    for (uint32_t p = 0; p < n_peers; ++p) quota[p] = (uint32_t)quota[p] >= r.limit ? 0 : (int32_t)(r.limit - quota[p]);
    if (failed) {
        std::sort(keys, keys + nf);
        for (uint32_t f = 0; f < nf; ++f) {
            const Entry& x = table[(uint32_t)keys[f]];
            failed[f] = {x.piece, x.peer, failed_status(x.status)};
        }
        *n_failed = nf;
    }
}

}  // namespace rt
}  // namespace krk
