// The ring selection's host arithmetic (kraken_amd/csrc/ring_select_math.hpp: what
// krk_ring_mask_owns, krk_ring_mask_moved and krk_ring_select run) as a stand-alone program: the
// selection at every digest count around the word edges, with and without invert and or_bits
// (whose last word carries set bits past n), at every idx_cap around the count, into exactly
// sized heap arrays (so an overrun is the sanitizer's to report) against a bit-at-a-time
// reference; and the mask builders on small hand-made tables, refusals included.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../kraken_amd/csrc/ring_select_math.hpp"

using namespace krk;

static uint64_t rnd(uint64_t& x) {
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
    return x;
}

static int check_select(uint64_t n, int mask_kind, bool invert, bool with_or, int& cases) {
    uint64_t x = 0x9E3779B97F4A7C15ull * (n + 1) + (uint64_t)mask_kind;
    uint8_t* d = (uint8_t*)malloc(n ? 32 * n : 1);
    for (uint64_t i = 0; i < 32 * n; ++i) d[i] = (uint8_t)rnd(x);
    uint64_t* mask = (uint64_t*)malloc(rs::kMaskWords * 8);
    for (uint32_t w = 0; w < rs::kMaskWords; ++w) mask[w] = mask_kind == 0 ? 0 : mask_kind == 1 ? ~0ull : rnd(x);
    const uint64_t nw = rs::words(n);
    uint64_t* orb = (uint64_t*)malloc(nw ? nw * 8 : 1);
    for (uint64_t w = 0; w < nw; ++w) orb[w] = rnd(x) & rnd(x) & rnd(x);
    if (n % 64) orb[nw - 1] |= 1ull << 63;  // past n: must not come through
    std::vector<uint64_t> want;
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t s = (uint32_t)d[32 * i] << 8 | d[32 * i + 1];
        bool sel = (((mask[s / 64] >> (s % 64)) & 1) != 0) != invert;
        if (with_or) sel = sel || ((orb[i / 64] >> (i % 64)) & 1);
        if (sel) want.push_back(i);
    }
    int wrong = 0;
    const uint64_t c = want.size();
    for (uint64_t cap : {(uint64_t)0, c ? c - 1 : 0, c, c + 1}) {
        uint64_t* bits = (uint64_t*)malloc(nw ? nw * 8 : 1);
        memset(bits, 0xFF, nw * 8);
        uint64_t* idx = cap ? (uint64_t*)malloc(cap * 8) : nullptr;
        if (cap) memset(idx, 0xFF, cap * 8);
        const uint64_t got = rs::select(d, n, mask, invert, with_or ? orb : nullptr, bits, idx, cap);
        wrong += got != c;
        for (uint64_t i = 0; i < nw * 64; ++i) {
            bool sel = false;
            for (uint64_t v : want) sel |= v == i;
            wrong += (((bits[i / 64] >> (i % 64)) & 1) != 0) != sel;
        }
        for (uint64_t k = 0; k < cap; ++k) wrong += idx[k] != (k < c ? want[k] : ~0ull);
        free(bits);
        free(idx);
        ++cases;
    }
    free(d);
    free(mask);
    free(orb);
    return wrong;
}

static int check_masks() {
    int wrong = 0;
    // two tables of row 2 and 3: shard s of A is owned by {s % 3, (s + 1) % 3}; B lists the same
    // owners in the other order and, for shards divisible by 5, node 3 as well
    const uint32_t S = rs::kShards;
    int32_t* la = (int32_t*)malloc(S * 2 * 4);
    int32_t* lb = (int32_t*)malloc(S * 3 * 4);
    uint8_t* ca = (uint8_t*)malloc(S);
    uint8_t* cb = (uint8_t*)malloc(S);
    for (uint32_t s = 0; s < S; ++s) {
        la[2 * s] = (int32_t)(s % 3), la[2 * s + 1] = (int32_t)((s + 1) % 3), ca[s] = 2;
        lb[3 * s] = (int32_t)((s + 1) % 3), lb[3 * s + 1] = (int32_t)(s % 3), lb[3 * s + 2] = s % 5 ? -1 : 3;
        cb[s] = s % 5 ? 2 : 3;
    }
    uint64_t* m = (uint64_t*)malloc(rs::kMaskWords * 8);
    for (int32_t node = -1; node < 4; ++node) {
        wrong += !rs::mask_owns(la, ca, 2, node, m);
        for (uint32_t s = 0; s < S; ++s)
            wrong += (((m[s / 64] >> (s % 64)) & 1) != 0) != ((int32_t)(s % 3) == node || (int32_t)((s + 1) % 3) == node);
    }
    const int32_t ident[4] = {0, 1, 2, -1}, perm[4] = {1, 2, 0, -1};
    wrong += !rs::mask_moved(la, ca, 2, lb, cb, 3, ident, 4, m);
    for (uint32_t s = 0; s < S; ++s) wrong += (((m[s / 64] >> (s % 64)) & 1) != 0) != (s % 5 == 0);
    wrong += !rs::mask_moved(la, ca, 2, lb, cb, 3, nullptr, 4, m);  // NULL: node 3 is then a node of A's
    for (uint32_t s = 0; s < S; ++s) wrong += (((m[s / 64] >> (s % 64)) & 1) != 0) != (s % 5 == 0);
    wrong += !rs::mask_moved(la, ca, 2, la, ca, 2, perm, 3, m);  // renumbered: {s+1, s+2} against {s, s+1}
    for (uint32_t s = 0; s < S; ++s) wrong += ((m[s / 64] >> (s % 64)) & 1) != 1;
    wrong += !rs::mask_moved(la, ca, 2, la, ca, 2, nullptr, 3, m);
    for (uint32_t w = 0; w < rs::kMaskWords; ++w) wrong += m[w] != 0;
    // refusals leave the mask as it was
    memset(m, 0xA5, rs::kMaskWords * 8);
    wrong += rs::mask_owns(nullptr, ca, 2, 0, m) || rs::mask_owns(la, nullptr, 2, 0, m) || rs::mask_owns(la, ca, 0, 0, m);
    wrong += rs::mask_owns(la, ca, 1, 0, m);                          // counts of 2 in rows of 1
    wrong += rs::mask_moved(la, ca, 2, lb, cb, 3, ident, 3, m);        // B owner 3 outside [0, 3)
    wrong += rs::mask_moved(la, ca, 0, lb, cb, 3, ident, 4, m) || rs::mask_moved(la, ca, 2, lb, cb, 0, ident, 4, m);
    wrong += rs::mask_moved(la, ca, 2, nullptr, cb, 3, ident, 4, m) || rs::mask_moved(la, ca, 2, lb, cb, 3, ident, 4, nullptr);
    for (uint32_t w = 0; w < rs::kMaskWords; ++w) wrong += m[w] != 0xA5A5A5A5A5A5A5A5ull;
    free(la), free(lb), free(ca), free(cb), free(m);
    return wrong;
}

int main() {
    int mismatches = 0, cases = 0;
    const uint64_t want[][2] = {{0, 0}, {1, 1}, {63, 1}, {64, 1}, {65, 2}, {(1ull << 32) + 1, (1ull << 26) + 1}};
    for (auto& w : want) mismatches += rs::words(w[0]) != w[1];
    for (uint64_t n : {0, 1, 63, 64, 65, 128, 129})
        for (int mask_kind = 0; mask_kind < 3; ++mask_kind)
            for (int invert = 0; invert < 2; ++invert)
                for (int with_or = 0; with_or < 2; ++with_or) mismatches += check_select(n, mask_kind, invert, with_or, cases);
    mismatches += check_masks();
    printf("ring_select_math: %d cases, %d mismatches\n", cases, mismatches);
    return mismatches != 0;
}
