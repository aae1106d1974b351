// find_sentinel_block.cpp -- the fixture of the tail handoff's sentinel collision
// (tests/golden/sha_sentinel_block.json).
//
// offload.cpp takes a midstate in the page-locked note as written once none of its eight words
// equals the note's fill, 0xFFFFFFFF; a true midstate word may equal the fill, and the host then
// waits for the launch to end instead.  This program finds an input that takes that branch: the
// first 64-byte block B -- an 8-byte little-endian counter from 0 in its leading bytes, 56 zero
// bytes after it -- for which compress(IV, B) holds a word 0xFFFFFFFF, and the first counter whose
// midstate holds none (the control).  About 2^29 compressions are expected (8 words x 2^-32 each).
//
// Plain portable SHA-256 (FIPS 180-4), no library code.  Build and run:
//   c++ -O2 -std=c++17 -pthread -o find_sentinel_block find_sentinel_block.cpp && ./find_sentinel_block
// It prints the fixture as JSON.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

static const uint32_t kIV[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a,
                                0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
static const uint32_t kK[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
    0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
    0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
    0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
    0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
constexpr uint32_t kSentinel = 0xFFFFFFFFu;

static inline uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

static void block_of(uint64_t counter, uint8_t b[64]) {
    memset(b, 0, 64);
    for (int k = 0; k < 8; ++k) b[k] = (uint8_t)(counter >> (8 * k));
}

static void compress(const uint32_t in[8], const uint8_t b[64], uint32_t out[8]) {
    uint32_t w[64];
    for (int i = 0; i < 16; ++i)
        w[i] = (uint32_t)b[4 * i] << 24 | (uint32_t)b[4 * i + 1] << 16 | (uint32_t)b[4 * i + 2] << 8 | b[4 * i + 3];
    for (int i = 16; i < 64; ++i) {
        const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
        const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
        w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = in[0], bb = in[1], c = in[2], d = in[3], e = in[4], f = in[5], g = in[6], h = in[7];
    for (int i = 0; i < 64; ++i) {
        const uint32_t t1 = h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + kK[i] + w[i];
        const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & bb) ^ (a & c) ^ (bb & c));
        h = g, g = f, f = e, e = d + t1, d = c, c = bb, bb = a, a = t1 + t2;
    }
    const uint32_t v[8] = {a, bb, c, d, e, f, g, h};
    for (int k = 0; k < 8; ++k) out[k] = in[k] + v[k];
}

static int sentinel_word(const uint32_t h[8]) {
    for (int k = 0; k < 8; ++k)
        if (h[k] == kSentinel) return k;
    return -1;
}

static void print_entry(const char* name, uint64_t counter, bool last) {
    uint8_t b[64];
    uint32_t h[8];
    block_of(counter, b);
    compress(kIV, b, h);
    printf("  \"%s\": {\"counter\": %llu, \"block\": \"", name, (unsigned long long)counter);
    for (int k = 0; k < 64; ++k) printf("%02x", b[k]);
    printf("\", \"word\": %d, \"midstate\": [", sentinel_word(h));
    for (int k = 0; k < 8; ++k) printf("\"%08x\"%s", h[k], k < 7 ? ", " : "");
    printf("]}%s\n", last ? "" : ",");
}

int main() {
    // counters in spans handed out in ascending order; a span is skipped once a smaller hit is known,
    // so the smallest hit -- the first -- is what remains whatever the threads' timing
    constexpr uint64_t kSpan = 1ull << 20;
    std::atomic<uint64_t> next{0}, best{UINT64_MAX};
    const unsigned T = std::max(1u, std::thread::hardware_concurrency());
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < T; ++t)
        pool.emplace_back([&] {
            uint8_t b[64];
            uint32_t h[8];
            for (;;) {
                const uint64_t lo = next.fetch_add(kSpan);
                if (lo >= best.load()) return;
                for (uint64_t c = lo; c < lo + kSpan; ++c) {
                    block_of(c, b);
                    compress(kIV, b, h);
                    if (sentinel_word(h) < 0) continue;
                    uint64_t cur = best.load();
                    while (c < cur && !best.compare_exchange_weak(cur, c)) {
                    }
                    break;
                }
            }
        });
    for (auto& th : pool) th.join();
    uint64_t control = 0;
    for (;; ++control) {
        uint8_t b[64];
        uint32_t h[8];
        block_of(control, b);
        compress(kIV, b, h);
        if (sentinel_word(h) < 0) break;
    }
    printf("{\n  \"sentinel\": \"%08x\",\n", kSentinel);
    print_entry("collision", best.load(), false);
    print_entry("control", control, true);
    printf("}\n");
    return 0;
}
