// have_round_math.hpp -- one have round over the torrent's own row of a request round
// (krk_have_round): `have`, row 0 of the rows, W = words(n) words, loaded from the piece status
// sidecar, checked against a verify result, persisted and advertised where it lies.  With mask =
// the bits below n, a round runs, in this order:
//   1 restore  kRestore: restorePieces / pieceStatusMetadata.Deserialize
//              (lib/torrent/storage/agentstorage/pieces.go:71-82,130-159) from the `_status`
//              sidecar, one byte a piece.  Well formed iff status_len == n: bit i = (byte i == 1),
//              every byte that is neither 0 nor 1 reads as empty and is counted (n_unexpected;
//              _dirty = 2 is one).  Otherwise kBadStatus and the row keeps every bit: a status,
//              not an error.  kInCache: have = mask (pieces.go:144-149).
//   2 merge    ok = W words in the layout krk_piece_bitfield writes.  kMergeOr (pieces verified
//              this round): changed = ok & ~have & mask, have |= ok & mask.  kMergeAnd (a recheck):
//              changed = have & ~ok & mask, have &= ok.  n_changed = popcount(changed); the first
//              min(n_changed, changed_cap) changed indices, ascending, are stored.
//   3 derive   n_complete = popcount(have & mask); bytes = BytesDownloaded() =
//              min(n_complete * piece_length, length) (torrent.go:126-128) without the product.
//      emit    kEmitStatus: Serialize (pieces.go:63-69), n bytes, 1 iff the bit is set.
//              kEmitWire: Bitfield() as willf/bitset MarshalBinary (peer_round_math.hpp, step 1):
//              the uint64 big-endian n, then each word big-endian -- 8 + 8 W bytes.
//              kEmitMissing: MissingPieces() (torrent.go:281-291): the first min(n - n_complete,
//              missing_cap) clear indices, ascending.
// A step that wrote the row leaves the tail bits of its last word clear.  Header-only and free of
// the runtime, so that tests/native/have_round_main.cpp builds it stand-alone under
// AddressSanitizer and UndefinedBehaviorSanitizer; have_round.hip computes the same state and
// outputs.
#pragma once
#include <stdint.h>

#include "peer_round_math.hpp"

namespace krk {
namespace hv {

constexpr uint32_t kRestore = 0x01, kInCache = 0x02, kMergeOr = 0x04, kMergeAnd = 0x08, kEmitStatus = 0x10,
                   kEmitWire = 0x20, kEmitMissing = 0x40, kAllFlags = 0x7F;  // KRK_HV_*
constexpr uint32_t kBadStatus = 1;                                           // flags_out

// What is wrong with a torrent's flags, or nullptr.
inline const char* flags_error(uint32_t flags) {
    if (flags & ~kAllFlags) return "unknown flag bit";
    if ((flags & kRestore) && (flags & kInCache)) return "both the sidecar restore and the cache restore";
    if ((flags & kMergeOr) && (flags & kMergeAnd)) return "both the OR merge and the AND merge";
    return nullptr;
}
// The round rewrites the row: a restore that is well formed, the cache, or a merge.
KRK_PR_HD inline bool writes_row(uint32_t flags, bool bad_status) {
    return ((flags & kRestore) && !bad_status) || (flags & (kInCache | kMergeOr | kMergeAnd));
}
// Word w of the round: `old` from the row, `st` the restored word (kRestore, well formed), ok the
// verify word.  *now the word after the round (masked when the round writes the row), *changed
// what the merge reports.
KRK_PR_HD inline void word_round(uint32_t flags, bool bad_status, uint64_t old, uint64_t st, uint64_t ok, uint64_t m,
                                 uint64_t* now, uint64_t* changed) {
    uint64_t h = old;
    if ((flags & kRestore) && !bad_status) h = st;
    if (flags & kInCache) h = m;
    *changed = 0;
    if (flags & kMergeOr) *changed = ok & ~h & m, h |= ok;
    if (flags & kMergeAnd) *changed = h & ~ok & m, h &= ok;
    *now = writes_row(flags, bad_status) ? h & m : h;
}
// BytesDownloaded(): min(n_complete * piece_length, length), both >= 0, without the product.
KRK_PR_HD inline uint64_t bytes_downloaded(uint64_t n_complete, int64_t piece_length, int64_t length) {
    const uint64_t pl = (uint64_t)piece_length, len = (uint64_t)length;
    return pl == 0 || n_complete > len / pl ? len : n_complete * pl;
}

struct Torrent {           // one torrent's spans as pointers (nullptr when its flag is not set)
    uint32_t flags;
    int64_t piece_length, length;
    const uint8_t* status;  // kRestore: the span's first byte ...
    uint64_t status_len;    // ... and its length
    const uint64_t* ok;     // kMergeOr / kMergeAnd: W words
    uint32_t* changed;
    uint64_t changed_cap;
    uint32_t* missing;
    uint64_t missing_cap;
    uint8_t* status_out;    // kEmitStatus: n bytes
    uint8_t* wire_out;      // kEmitWire: 8 + 8 W bytes
};
struct Out {
    uint32_t flags, n_unexpected, n_changed, n_complete;
    uint64_t bytes;
};

inline void put_be64(uint8_t* p, uint64_t x) {
    for (int k = 7; k >= 0; --k) p[k] = (uint8_t)x, x >>= 8;
}

// One torrent's round over its `have` row (nullptr when W is 0).
inline Out round_torrent(uint64_t* have, uint64_t n, const Torrent& t) {
    const uint64_t W = pr::words(n);
    Out o = {};
    const bool bad = (t.flags & kRestore) && t.status_len != n;
    if (bad) o.flags = kBadStatus;
    uint64_t n_changed = 0, n_complete = 0, n_missing = 0;
    if (t.flags & kEmitWire) put_be64(t.wire_out, n);
    for (uint64_t w = 0; w < W; ++w) {
        const uint64_t m = pe::word_mask(n, w, W);
        uint64_t st = 0;
        if ((t.flags & kRestore) && !bad)
            for (uint64_t i = 64 * w; i < n && i < 64 * w + 64; ++i) {
                const uint8_t b = t.status[i];
                if (b == 1) st |= 1ull << (i & 63);
                else if (b) ++o.n_unexpected;
            }
        uint64_t now, changed;
        word_round(t.flags, bad, have[w], st, t.ok ? t.ok[w] : 0, m, &now, &changed);
        if (now != have[w]) have[w] = now;
        for (uint64_t x = changed; x; x &= x - 1, ++n_changed)
            if (n_changed < t.changed_cap) t.changed[n_changed] = (uint32_t)(64 * w + (uint64_t)__builtin_ctzll(x));
        n_complete += (uint64_t)__builtin_popcountll(now & m);
        if (t.flags & kEmitMissing)
            for (uint64_t x = ~now & m; x; x &= x - 1, ++n_missing)
                if (n_missing < t.missing_cap) t.missing[n_missing] = (uint32_t)(64 * w + (uint64_t)__builtin_ctzll(x));
        if (t.flags & kEmitStatus)
            for (uint64_t i = 64 * w; i < n && i < 64 * w + 64; ++i) t.status_out[i] = (uint8_t)((now >> (i & 63)) & 1);
        if (t.flags & kEmitWire) put_be64(t.wire_out + 8 + 8 * w, now & m);
    }
    o.n_changed = (uint32_t)n_changed;
    o.n_complete = (uint32_t)n_complete;
    o.bytes = bytes_downloaded(n_complete, t.piece_length, t.length);
    return o;
}

}  // namespace hv
}  // namespace krk
