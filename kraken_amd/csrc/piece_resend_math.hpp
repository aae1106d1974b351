// piece_resend_math.hpp -- where a failed piece request goes next (krk_piece_resend_round):
// Dispatcher.resendFailedPieceRequests (lib/torrent/scheduler/dispatch/dispatcher.go:401-434) over
// the rows of a request round (piece_request_math.hpp).  The reference answers "does peer p hold
// piece i, do we lack it, may we ask p for it" by building p.bitfield & ~have over the whole
// torrent, a one-bit bitset beside it, and ReservePieces over both; here it is bit i of three rows
// and a find-first over the peers in index order.  The pending set that grows inside the call
// (ReservePieces(p, {i}) blocks p itself, and outside endgame everybody, for piece i from then on)
// needs no row of its own: a torrent's entries ascend by piece, so "an earlier entry of this call
// with the same piece" lies in the run of equal pieces that ends at the current entry, and the
// state is the piece last resent (without duplicates) or the piece last resent to each peer
// (`mark`, with them).  Header-only and free of the runtime, so that
// tests/native/piece_resend_main.cpp builds it stand-alone under AddressSanitizer and
// UndefinedBehaviorSanitizer; piece_resend.hip computes the same targets.
#pragma once
#include <stdint.h>

#include "piece_request_math.hpp"

namespace krk {
namespace rs {

constexpr uint32_t kExpired = 1;  // KRK_PR_EXPIRED
constexpr uint32_t kUnsent = 2;   // KRK_PR_UNSENT
constexpr uint32_t kInvalid = 3;  // KRK_PR_INVALID

struct Failed {  // krk_failed_request
    uint32_t piece, peer, status;
};

inline bool flags_ok(uint32_t flags) { return !(flags & ~(pr::kPolicyMask | pr::kAllowDuplicates)); }
// Expired and invalid requests do not go back to their own peer (dispatcher.go:412-416).
KRK_PR_HD inline bool excludes_own_peer(uint32_t status) { return status != kUnsent; }
KRK_PR_HD inline int32_t quota_left(int32_t q) { return q < 0 ? 0 : q; }

// What is wrong with one torrent's list (n pieces, n_peers peers), or nullptr: *at is the entry.
inline const char* list_error(const Failed* f, uint64_t n_failed, uint64_t n, uint32_t n_peers, uint64_t* at) {
    for (uint64_t k = 0; k < n_failed; ++k) {
        *at = k;
        if (f[k].piece >= n) return "a piece past the torrent's last";
        if (f[k].peer >= n_peers && f[k].peer != pr::kNone) return "a peer that is neither one of the torrent's nor 0xFFFFFFFF";
        if (f[k].status < kExpired || f[k].status > kInvalid) return "a status outside 1..3";
        if (k && f[k].piece < f[k - 1].piece) return "pieces that do not ascend";
    }
    return nullptr;
}

// One torrent's resend: rows = have, then (bits_p, blocked_p) a peer, W = words(n) words each;
// quota and left (n_peers entries each) start at the torrent's first peer, target has n_failed
// entries.  mark: n_peers words of scratch (unused without kAllowDuplicates).  The list is valid
// (list_error).  Every left[p] and target[f] is stored; returns the entries resent.
inline uint32_t resend_torrent(const uint64_t* rows, uint64_t n, uint32_t n_peers, uint32_t flags, const int32_t* quota,
                               const Failed* failed, uint64_t n_failed, uint32_t* mark, uint32_t* target,
                               int32_t* left) {
    const uint64_t W = pr::words(n);
    const bool dup = (flags & pr::kAllowDuplicates) != 0;
    for (uint32_t p = 0; p < n_peers; ++p) left[p] = quota_left(quota[p]);
    if (dup)
        for (uint32_t p = 0; p < n_peers; ++p) mark[p] = pr::kNone;  // no piece has this index: n < 2^32
    uint32_t last = pr::kNone, resent = 0;  // the piece last resent to anybody
    for (uint64_t f = 0; f < n_failed; ++f) {
        const uint32_t i = failed[f].piece;
        const uint64_t w = i >> 6, b = 1ull << (i & 63);
        target[f] = pr::kNone;
        if ((rows[w] & b) || (!dup && last == i)) continue;
        const bool excl = excludes_own_peer(failed[f].status);
        for (uint32_t p = 0; p < n_peers; ++p) {
            const uint64_t* row = rows + (1 + 2 * (uint64_t)p) * W;
            if (excl && p == failed[f].peer) continue;
            if (!(row[w] & b) || left[p] == 0 || (row[W + w] & b)) continue;
            if (dup && mark[p] == i) continue;
            target[f] = p;
            --left[p];
            if (dup) mark[p] = i;
            last = i;
            ++resent;
            break;
        }
    }
    return resent;
}

}  // namespace rs
}  // namespace krk
