// piece_request_math.hpp -- what to ask the peers for next (krk_piece_availability,
// krk_piece_select, krk_piece_request_round): the availability counts numPeersByPiece
// (lib/torrent/scheduler/dispatch/dispatcher.go:257-284) as the column sum of the peers'
// bitfields, and piecerequest.Manager.ReservePieces' selection (piecerequest/manager.go:101-137,
// rarest_first_policy.go:38-44, default_policy.go:33-66) as a k-smallest over the packed key
// (uint64)key(i) << 32 | i under bit masks.  Bitsets are willf/bitset words (bitfield_math.hpp):
// piece i = bit i & 63 of word i >> 6; tail bits past n are ignored wherever a row is read.
// Ties go to the lower piece index (the reference's heap leaves them to container/heap's sift
// order); the sequence of keys popped is the same.  Header-only and free of the runtime, so that
// tests/native/piece_request_main.cpp builds it stand-alone under AddressSanitizer and
// UndefinedBehaviorSanitizer; piece_request.hip computes the same picks.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define KRK_PR_HD __host__ __device__
#else
#define KRK_PR_HD
#endif

namespace krk {
namespace pr {

constexpr uint32_t kMaxLimit = 16;          // KRK_PR_MAX_LIMIT
constexpr uint32_t kRarestFirst = 0;        // KRK_PR_RAREST_FIRST
constexpr uint32_t kSample = 1;             // KRK_PR_SAMPLE
constexpr uint32_t kPolicyMask = 0xFF;
constexpr uint32_t kAllowDuplicates = 0x100;  // KRK_PR_ALLOW_DUPLICATES
constexpr uint32_t kNone = 0xFFFFFFFFu;     // a picks entry past n_picked

inline uint64_t words(uint64_t n) { return n / 64 + (n % 64 != 0); }
inline bool flags_ok(uint32_t flags) {
    return !(flags & ~(kPolicyMask | kAllowDuplicates)) && (flags & kPolicyMask) <= kSample;
}
// The bits of word w that are pieces of a torrent of n.
inline uint64_t live_bits(uint64_t n, uint64_t w) { return n - w * 64 >= 64 ? ~0ull : (1ull << (n - w * 64)) - 1; }

// splitmix64: the project's constants (the synthetic blobs' seeds use the same mix).
KRK_PR_HD inline uint64_t splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// KRK_PR_SAMPLE's key of piece i for peer p: the limit smallest are a uniform sample.
KRK_PR_HD inline uint32_t sample_key(uint64_t seed, uint32_t peer, uint32_t i) {
    return (uint32_t)(splitmix64(seed ^ ((uint64_t)peer << 32 | i)) >> 32);
}

// counts[i] = the rows (n_peers of them, `stride` words apart) with bit i set, i < n.
inline void availability(const uint64_t* rows, uint64_t stride, uint32_t n_peers, uint64_t n, uint32_t* counts) {
    for (uint64_t i = 0; i < n; ++i) counts[i] = 0;
    for (uint32_t p = 0; p < n_peers; ++p) {
        const uint64_t* r = rows + (uint64_t)p * stride;
        for (uint64_t w = 0; w * 64 < n; ++w)
            for (uint64_t x = r[w] & live_bits(n, w); x; x &= x - 1) ++counts[w * 64 + (uint64_t)__builtin_ctzll(x)];
    }
}

// The min(q, |c|) pieces of c = a & ~x & ~y & ~z (x, y, z nullable) with the smallest
// (key(i), i), ascending, into picks; returns how many.  q <= kMaxLimit.  counts is read only
// under kRarestFirst.
inline uint32_t select(const uint64_t* a, const uint64_t* x, const uint64_t* y, const uint64_t* z,
                       const uint32_t* counts, uint64_t n, uint32_t q, uint32_t policy, uint64_t seed, uint32_t peer,
                       uint32_t* picks) {
    uint64_t best[kMaxLimit];
    uint32_t m = 0;
    if (!q || q > kMaxLimit) return 0;
    for (uint64_t w = 0; w * 64 < n; ++w) {
        uint64_t c = a[w] & live_bits(n, w);
        if (x) c &= ~x[w];
        if (y) c &= ~y[w];
        if (z) c &= ~z[w];
        for (; c; c &= c - 1) {
            const uint32_t i = (uint32_t)(w * 64 + (uint64_t)__builtin_ctzll(c));
            const uint32_t key = policy == kSample ? sample_key(seed, peer, i) : counts[i];
            const uint64_t pk = (uint64_t)key << 32 | i;
            if (m == q) {
                if (pk > best[m - 1]) continue;
                --m;  // the largest leaves
            }
            uint32_t j = m;
            for (; j && best[j - 1] > pk; --j) best[j] = best[j - 1];
            best[j] = pk;
            ++m;
        }
    }
    for (uint32_t j = 0; j < m; ++j) picks[j] = (uint32_t)best[j];
    return m;
}

// One torrent's round: rows = have, then (bits_p, blocked_p) a peer, W = words(n) words each;
// quota, n_picked and picks (rows of `limit`) start at the torrent's first peer.  taken: W words
// of scratch (unused with kAllowDuplicates).  counts (n entries) is read only under
// kRarestFirst.  Every n_picked[p] and picks[p * limit + j], j < limit, is stored.
inline void round_torrent(const uint64_t* rows, uint64_t n, uint32_t n_peers, uint32_t flags, uint64_t seed,
                          const int32_t* quota, uint32_t limit, const uint32_t* counts, uint64_t* taken,
                          uint32_t* picks, uint32_t* n_picked) {
    const uint64_t W = words(n);
    const bool dup = (flags & kAllowDuplicates) != 0;
    if (!dup)
        for (uint64_t w = 0; w < W; ++w) taken[w] = 0;
    for (uint32_t p = 0; p < n_peers; ++p) {
        const uint64_t* row = rows + (1 + 2 * (uint64_t)p) * W;
        const uint32_t q = quota[p] <= 0 ? 0 : ((uint32_t)quota[p] < limit ? (uint32_t)quota[p] : limit);
        uint32_t* out = picks + (uint64_t)p * limit;
        const uint32_t m = select(row, rows, row + W, dup ? nullptr : taken, counts, n, q, flags & kPolicyMask, seed, p, out);
        n_picked[p] = m;
        for (uint32_t j = m; j < limit; ++j) out[j] = kNone;
        if (!dup)
            for (uint32_t j = 0; j < m; ++j) taken[out[j] >> 6] |= 1ull << (out[j] & 63);
    }
}

}  // namespace pr
}  // namespace krk
