// peer_round_math.hpp -- one peer round over the rows of a request round (krk_peer_round): the
// peer set of the resident state and what the dispatcher derives from it.  The rows are have, then
// (bits_p, blocked_p) a peer slot, W = words(n) words each; a live row beside them holds bit p when
// slot p holds a connection.  A round runs, in this order:
//   1 joins   Dispatcher.AddPeer (lib/torrent/scheduler/dispatch/dispatcher.go:243-274) from the
//             wire bytes of the handshake's BitfieldMessage (conn/handshaker.go:63-131): slots,
//             strictly ascending, each with a span of `wire` holding a willf/bitset MarshalBinary --
//             a uint64 big-endian bit length, then ceil(length / 64) words, each uint64 big-endian,
//             word k holding bits 64k .. 64k + 63.  (The format of the willf/bitset commit the
//             reference's glide.lock names; its source is not part of this tree, so this is the
//             format assumed, pinned by the vector bits {0, 9} of 10 =
//             00 00 00 00 00 00 00 0A  00 00 00 00 00 00 02 01.)  Well formed iff wire_len >= 8, the
//             length field equals n and wire_len == 8 + 8 W: bits_p becomes the decoded words, the
//             tail bits past n cleared (kJoined).  Otherwise kBadBitfield and the row keeps every
//             bit: the bytes come from a remote peer, so this is a status and not an error.  No
//             byte outside the span is read, and the span starts at any byte.
//   2 fulls   handleComplete (dispatcher.go:589-597): slots, strictly ascending; bits_p becomes all
//             ones below n (kSetFull).  A slot joined and filled in one round ends up full.
//   3 derive  mask = the bits below n:
//             remaining = n - popcount(have & mask); kTorrentComplete iff it is 0, kEndgame iff
//             endgame is not disabled and remaining <= threshold                   (:366-372)
//             held_p = popcount(bits_p & mask), wanted_p = popcount(bits_p & ~have & mask) (the
//             candidate set of maybeRequestMorePieces); for a live slot kPeerComplete iff
//             held_p == n, and under a complete torrent kClose for a complete peer, kNotify for
//             any other (complete(), :321-338).
// blocked_p is not touched.  Header-only and free of the runtime, so that
// tests/native/peer_round_main.cpp builds it stand-alone under AddressSanitizer and
// UndefinedBehaviorSanitizer; peer_round.hip computes the same state and outputs.
#pragma once
#include <stdint.h>

#include "piece_request_math.hpp"

namespace krk {
namespace pe {

constexpr uint32_t kDisableEndgame = 1;                        // KRK_PE_DISABLE_ENDGAME
constexpr uint32_t kTorrentComplete = 1, kEndgame = 2;         // torrent_flags_out
constexpr uint32_t kJoined = 0x01, kBadBitfield = 0x02, kSetFull = 0x04, kPeerComplete = 0x08, kClose = 0x10,
                   kNotify = 0x20;                             // status_out

struct Join {  // krk_peer_join
    uint32_t peer, reserved;
    uint64_t wire_off, wire_len;
};

// The big-endian uint64 at p[0, 8).
inline uint64_t be64(const uint8_t* p) {
    uint64_t x = 0;
    for (int k = 0; k < 8; ++k) x = x << 8 | p[k];
    return x;
}
// A span of wire_len bytes whose first eight (when it has them) read `length` is the bitfield of a
// torrent of n pieces, n < 2^32.
KRK_PR_HD inline bool wire_ok(uint64_t wire_len, uint64_t length, uint64_t n) {
    return wire_len >= 8 && length == n && wire_len == 8 + 8 * ((n + 63) >> 6);
}
// The bits of word w (of W) that are pieces: the last word's tail is clear.
KRK_PR_HD inline uint64_t word_mask(uint64_t n, uint64_t w, uint64_t W) {
    return w + 1 == W && (n & 63) ? (1ull << (n & 63)) - 1 : ~0ull;
}
KRK_PR_HD inline uint32_t torrent_flags(uint64_t remaining, uint32_t threshold, uint32_t flags) {
    return (remaining == 0 ? kTorrentComplete : 0) | (!(flags & kDisableEndgame) && remaining <= threshold ? kEndgame : 0);
}
// What derive adds to a slot's status.
KRK_PR_HD inline uint32_t peer_flags(bool live, uint64_t held, uint64_t n, uint64_t remaining) {
    if (!live) return 0;
    const bool full = held == n;
    return (full ? kPeerComplete : 0) | (remaining ? 0 : full ? kClose : kNotify);
}

// What is wrong with a torrent's lists (n_peers slots), or nullptr: *at is the element.
inline const char* lists_error(const Join* joins, uint64_t n_joins, const uint32_t* fulls, uint64_t n_fulls,
                               uint32_t n_peers, uint64_t* at) {
    for (uint64_t k = 0; k < n_joins; ++k) {
        *at = k;
        if (joins[k].peer >= n_peers) return "a join's peer that is not one of the torrent's slots";
        if (k && joins[k].peer <= joins[k - 1].peer) return "joins that do not strictly ascend";
        if (joins[k].reserved) return "a join with a non-zero reserved field";
        if (joins[k].wire_off + joins[k].wire_len < joins[k].wire_off) return "a join whose wire span overflows";
    }
    for (uint64_t k = 0; k < n_fulls; ++k) {
        *at = k;
        if (fulls[k] >= n_peers) return "a full's peer that is not one of the torrent's slots";
        if (k && fulls[k] <= fulls[k - 1]) return "fulls that do not strictly ascend";
    }
    return nullptr;
}

// One torrent's round: rows as above (nullptr when W is 0), live its live words, the lists valid;
// held, wanted and status start at the torrent's first slot.
inline void round_torrent(uint64_t* rows, uint64_t n, uint32_t n_peers, const uint64_t* live, const Join* joins,
                          uint32_t n_joins, const uint32_t* fulls, uint32_t n_fulls, const uint8_t* wire,
                          uint32_t threshold, uint32_t flags, uint32_t* remaining_out, uint32_t* flags_out, uint32_t* held,
                          uint32_t* wanted, uint32_t* status) {
    const uint64_t W = pr::words(n);
    for (uint32_t p = 0; p < n_peers; ++p) status[p] = 0;
    for (uint32_t k = 0; k < n_joins; ++k) {
        const Join& j = joins[k];
        const uint8_t* span = wire + j.wire_off;
        if (!wire_ok(j.wire_len, j.wire_len >= 8 ? be64(span) : 0, n)) {
            status[j.peer] = kBadBitfield;
            continue;
        }
        uint64_t* row = rows + (1 + 2 * (uint64_t)j.peer) * W;
        for (uint64_t w = 0; w < W; ++w) row[w] = be64(span + 8 + 8 * w) & word_mask(n, w, W);
        status[j.peer] = kJoined;
    }
    for (uint32_t k = 0; k < n_fulls; ++k) {
        uint64_t* row = rows + (1 + 2 * (uint64_t)fulls[k]) * W;
        for (uint64_t w = 0; w < W; ++w) row[w] = word_mask(n, w, W);
        status[fulls[k]] |= kSetFull;
    }
    uint64_t have = 0;
    for (uint64_t w = 0; w < W; ++w) have += (uint64_t)__builtin_popcountll(rows[w] & word_mask(n, w, W));
    const uint64_t remaining = n - have;
    *remaining_out = (uint32_t)remaining;
    *flags_out = torrent_flags(remaining, threshold, flags);
    for (uint32_t p = 0; p < n_peers; ++p) {
        const uint64_t* row = rows + (1 + 2 * (uint64_t)p) * W;
        uint64_t h = 0, x = 0;
        for (uint64_t w = 0; w < W; ++w) {
            const uint64_t b = row[w] & word_mask(n, w, W);
            h += (uint64_t)__builtin_popcountll(b);
            x += (uint64_t)__builtin_popcountll(b & ~rows[w]);
        }
        held[p] = (uint32_t)h;
        wanted[p] = (uint32_t)x;
        status[p] |= peer_flags((live[p >> 6] >> (p & 63)) & 1, h, n, remaining);
    }
}

}  // namespace pe
}  // namespace krk
