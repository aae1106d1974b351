// The host bitfield packer (kraken_amd/csrc/bitfield_math.hpp: krk_bitfield_words and
// krk_piece_bitfield's loop) as a stand-alone program: every piece count around the word
// edges, mismatches at lane 0, lane 63, the first bit of the second word and the last piece,
// none and all bad, into exactly sized heap arrays full of 0xFF (so an overrun is the
// sanitizer's to report), against a bit-at-a-time reference.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../kraken_amd/csrc/bitfield_math.hpp"

using namespace krk;

static int check(uint64_t n, const std::vector<uint64_t>& bad) {
    uint32_t* sums = (uint32_t*)malloc(n ? n * 4 : 1);
    uint32_t* expected = (uint32_t*)malloc(n ? n * 4 : 1);
    const uint64_t nw = bf::words(n);
    uint64_t* bits = (uint64_t*)malloc(nw ? nw * 8 : 1);
    memset(bits, 0xFF, nw * 8);
    uint64_t x = 0x9E3779B97F4A7C15ull * (n + 1);
    for (uint64_t i = 0; i < n; ++i) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        sums[i] = expected[i] = (uint32_t)x;
    }
    std::vector<char> is_bad(n, 0);
    for (uint64_t p : bad)
        if (p < n && !is_bad[p]) {
            is_bad[p] = 1;
            sums[p] ^= 1u << (p % 32);
        }
    uint64_t n_bad = 0;
    for (char b : is_bad) n_bad += b;
    const uint64_t good = bf::pack(sums, expected, n, bits);
    int wrong = good != n - n_bad;
    for (uint64_t i = 0; i < nw * 64; ++i) {
        const int bit = (int)((bits[i >> 6] >> (i & 63)) & 1);
        wrong += bit != (i < n && !is_bad[i]);
    }
    free(sums);
    free(expected);
    free(bits);
    return wrong;
}

int main() {
    int mismatches = 0;
    const uint64_t want[][2] = {{0, 0}, {1, 1}, {63, 1}, {64, 1}, {65, 2}, {(1ull << 32) + 1, (1ull << 26) + 1}};
    for (auto& w : want) mismatches += bf::words(w[0]) != w[1];
    int cases = 0;
    for (uint64_t n : {0, 1, 2, 63, 64, 65, 127, 128, 129, 513, 4096, 4097}) {
        std::vector<uint64_t> all;
        for (uint64_t i = 0; i < n; ++i) all.push_back(i);
        const std::vector<std::vector<uint64_t>> sets = {{}, all, {0}, {63}, {64}, {n ? n - 1 : 0}, {0, 63, 64, n ? n - 1 : 0}};
        for (auto& s : sets) {
            mismatches += check(n, s);
            ++cases;
        }
    }
    printf("piece_bitfield: %d cases, %d mismatches\n", cases, mismatches);
    return mismatches != 0;
}
