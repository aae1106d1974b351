// bitfield_math.hpp -- the host bitfield packer's arithmetic (krk_bitfield_words,
// krk_piece_bitfield): willf/bitset words, piece i = bit i & 63 of word i >> 6, 1 = the sums
// match.  Header-only and free of the runtime, so that tests/native/piece_bitfield_main.cpp
// builds it stand-alone under AddressSanitizer and UndefinedBehaviorSanitizer.
#pragma once
#include <stdint.h>

namespace krk {
namespace bf {

inline uint64_t words(uint64_t n_pieces) { return n_pieces / 64 + (n_pieces % 64 != 0); }

// bits[0, words(n)) from sums and expected (n entries each); returns the matching pieces.  The
// last word's tail bits are 0.
inline uint64_t pack(const uint32_t* sums, const uint32_t* expected, uint64_t n, uint64_t* bits) {
    uint64_t good = 0;
    for (uint64_t w = 0; w * 64 < n; ++w) {
        const uint64_t m = n - w * 64 < 64 ? n - w * 64 : 64;
        uint64_t word = 0;
        for (uint64_t l = 0; l < m; ++l) word |= (uint64_t)(sums[w * 64 + l] == expected[w * 64 + l]) << l;
        bits[w] = word;
        good += (uint64_t)__builtin_popcountll(word);
    }
    return good;
}

}  // namespace bf
}  // namespace krk
