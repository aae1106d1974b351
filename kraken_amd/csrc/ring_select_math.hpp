// ring_select_math.hpp -- ring ownership as 65,536-bit shard predicates, and a predicate applied
// to digests (krk_ring_mask_owns, krk_ring_mask_moved, krk_ring_select): what maybeDelete's
// `owns` (origin/blobserver/server.go:686-759) and applyToReplicas' replica set (426-454) ask,
// one blob at a time, of hashRing.Locations(d).  Locations(d) depends on d only through its
// ShardID (the first two digest bytes), so "owns", "owner set changed between two memberships"
// and every combination of them is a mask of 1,024 uint64 words: shard s is bit s & 63 of word
// s >> 6 (the project's bitset layout, bitfield_math.hpp).  Header-only and free of the
// runtime, so that tests/native/ring_select_math_main.cpp builds it stand-alone under
// AddressSanitizer and UndefinedBehaviorSanitizer; ring_select.hip runs the same selection.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace krk {
namespace rs {

constexpr uint32_t kShards = 65536;
constexpr uint32_t kMaskWords = kShards / 64;

inline uint64_t words(uint64_t n) { return n / 64 + (n % 64 != 0); }
inline uint32_t shard_of(const uint8_t* digest32) { return (uint32_t)digest32[0] << 8 | digest32[1]; }

// A table as krk_ring_owner_table returns it: counts[s] <= row entries a row.
inline bool table_ok(const int32_t* locs, const uint8_t* counts, uint32_t row) {
    if (!locs || !counts || !row) return false;
    for (uint32_t s = 0; s < kShards; ++s)
        if (counts[s] > row) return false;
    return true;
}

// mask[s] = node is one of Locations(s).  false (mask untouched): a null table, row == 0 or a
// count past the row.
inline bool mask_owns(const int32_t* locs, const uint8_t* counts, uint32_t row, int32_t node, uint64_t* mask) {
    if (!mask || !table_ok(locs, counts, row)) return false;
    memset(mask, 0, kMaskWords * 8);
    for (uint32_t s = 0; s < kShards; ++s) {
        const int32_t* L = locs + (uint64_t)s * row;
        bool has = false;
        for (uint32_t q = 0; q < counts[s]; ++q) has |= L[q] == node;
        mask[s >> 6] |= (uint64_t)has << (s & 63);
    }
    return true;
}

// mask[s] = the owner SETS of s differ between membership A and B (order ignored, as
// stringset.FromSlice ignores it).  b_to_a[j]: the index in A of B's node j, -1 for a node A
// does not have; NULL: the same node list.  false (mask untouched): a null table, row == 0, a
// count past the row or a B owner outside [0, n_nodes_b).
inline bool mask_moved(const int32_t* locs_a, const uint8_t* counts_a, uint32_t row_a, const int32_t* locs_b,
                       const uint8_t* counts_b, uint32_t row_b, const int32_t* b_to_a, uint32_t n_nodes_b,
                       uint64_t* mask) {
    if (!mask || !table_ok(locs_a, counts_a, row_a) || !table_ok(locs_b, counts_b, row_b)) return false;
    for (uint32_t s = 0; s < kShards; ++s)
        for (uint32_t q = 0; q < counts_b[s]; ++q) {
            const int32_t j = locs_b[(uint64_t)s * row_b + q];
            if (j < 0 || (uint32_t)j >= n_nodes_b) return false;
        }
    memset(mask, 0, kMaskWords * 8);
    std::vector<int32_t> a, b;
    for (uint32_t s = 0; s < kShards; ++s) {
        const int32_t* A = locs_a + (uint64_t)s * row_a;
        const int32_t* B = locs_b + (uint64_t)s * row_b;
        a.assign(A, A + counts_a[s]);
        b.clear();
        bool moved = false;
        for (uint32_t q = 0; q < counts_b[s]; ++q) {
            const int32_t j = b_to_a ? b_to_a[B[q]] : B[q];
            if (j < 0) moved = true;  // an owner A does not know
            b.push_back(j);
        }
        if (!moved) {
            std::sort(a.begin(), a.end());
            a.erase(std::unique(a.begin(), a.end()), a.end());
            std::sort(b.begin(), b.end());
            b.erase(std::unique(b.begin(), b.end()), b.end());
            moved = a != b;
        }
        mask[s >> 6] |= (uint64_t)moved << (s & 63);
    }
    return true;
}

// sel(i) = (mask[ShardID(d_i)] ^ invert) | or_bits[i].  Every one of bits[0, words(n)) is
// stored, the last word's tail bits 0; idx (nullable) receives the first min(count, idx_cap)
// selected i, ascending, and nothing past them.  Returns the count.
inline uint64_t select(const uint8_t* digests32, uint64_t n, const uint64_t* mask, bool invert, const uint64_t* or_bits,
                       uint64_t* bits, uint64_t* idx, uint64_t idx_cap) {
    uint64_t count = 0;
    for (uint64_t w = 0; w * 64 < n; ++w) {
        const uint64_t m = n - w * 64 < 64 ? n - w * 64 : 64;
        uint64_t word = 0;
        for (uint64_t l = 0; l < m; ++l) {
            const uint32_t s = shard_of(digests32 + 32 * (w * 64 + l));
            word |= (((mask[s >> 6] >> (s & 63)) & 1) ^ (uint64_t)invert) << l;
        }
        if (or_bits) word |= or_bits[w] & (m == 64 ? ~0ull : (1ull << m) - 1);
        bits[w] = word;
        for (uint64_t x = word; x; x &= x - 1) {
            if (idx && count < idx_cap) idx[count] = w * 64 + (uint64_t)__builtin_ctzll(x);
            ++count;
        }
    }
    return count;
}

}  // namespace rs
}  // namespace krk
