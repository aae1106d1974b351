// The re-piece arithmetic (kraken_amd/csrc/repiece_math.hpp: what krk_repiece_sums,
// krk_repiece_batch and piece_repiece.hip run) as a stand-alone program: the k <= 64 and k > 64
// shapes of the kernel's decomposition over real bytes against an in-program bytewise CRC-32,
// and 64-bit distances (pieces of 2^33 bytes, lengths near 2^40) against a left-to-right fold of
// the same sums, into exactly sized heap arrays full of 0xFF (so an overrun is the sanitizer's to
// report).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../kraken_amd/csrc/repiece_math.hpp"

using namespace krk;

static uint32_t crc_bytes(const uint8_t* p, uint64_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (uint64_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int b = 0; b < 8; ++b) c = (c >> 1) ^ (kCrcPoly & (0u - (c & 1u)));
    }
    return ~c;
}

static uint64_t g_x = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_x ^= g_x << 13, g_x ^= g_x >> 7, g_x ^= g_x << 17;
    return (uint32_t)(g_x >> 16);
}

static X8Pow g_tab;

// One blob of `length` real bytes: old sums at po, re-pieced by k, against the bytes' own sums.
static int check_bytes(uint64_t length, uint64_t po, uint64_t k) {
    uint8_t* data = (uint8_t*)malloc(length ? length : 1);
    for (uint64_t i = 0; i < length; ++i) data[i] = (uint8_t)rnd();
    const uint64_t n_old = rp::num_pieces(length, po), n_new = rp::num_pieces(length, po * k);
    uint32_t* old = (uint32_t*)malloc(n_old ? n_old * 4 : 1);
    uint32_t* out = (uint32_t*)malloc(n_new ? n_new * 4 : 1);
    memset(out, 0xFF, n_new * 4);
    for (uint64_t i = 0; i < n_old; ++i) old[i] = crc_bytes(data + i * po, rp::piece_end(i, po, length) - i * po);
    rp::repiece(old, length, po, k, out, g_tab.v);
    int wrong = 0;
    for (uint64_t j = 0; j < n_new; ++j)
        wrong += out[j] != crc_bytes(data + j * po * k, rp::piece_end(j, po * k, length) - j * po * k);
    // the kernel's view: every old piece's term XOR-ed into its new piece, in any order
    std::vector<uint32_t> acc(n_new, 0);
    for (uint64_t i = n_old; i-- > 0;) acc[i / k] ^= rp::term(old[i], i, po, k, length, g_tab.v);
    for (uint64_t j = 0; j < n_new; ++j) wrong += acc[j] != out[j];
    free(data);
    free(old);
    free(out);
    return wrong;
}

// No bytes: random sums, pieces of 2^33 bytes; the reference folds left to right,
// acc = shift(acc, |piece|) ^ sum, with shift through crc_math.hpp's x8n.
static int check_far(uint64_t length, uint64_t po, uint64_t k) {
    const uint64_t n_old = rp::num_pieces(length, po), n_new = rp::num_pieces(length, po * k);
    uint32_t* old = (uint32_t*)malloc(n_old * 4);
    uint32_t* out = (uint32_t*)malloc(n_new * 4);
    memset(out, 0xFF, n_new * 4);
    for (uint64_t i = 0; i < n_old; ++i) old[i] = rnd();
    rp::repiece(old, length, po, k, out, g_tab.v);
    int wrong = 0;
    for (uint64_t j = 0; j < n_new; ++j) {
        uint32_t acc = 0;
        for (uint64_t i = j * k; i < n_old && i < (j + 1) * k; ++i)
            acc = gf2_mulmod(acc, x8n(rp::piece_end(i, po, length) - i * po, g_tab.v)) ^ old[i];
        wrong += acc != out[j];
    }
    free(old);
    free(out);
    return wrong;
}

int main() {
    g_tab = make_x8pow();
    int mismatches = 0, cases = 0;
    // the counting rules
    mismatches += rp::num_pieces(0, 16) != 0 || rp::num_pieces(1, 16) != 1 || rp::num_pieces(16, 16) != 1 ||
                  rp::num_pieces(17, 16) != 2;
    mismatches += rp::units(0, 2) != 0 || rp::units(32, 2) != 1 || rp::units(33, 2) != 2 || rp::units(3, 33) != 3 ||
                  rp::units(2, 64) != 2 || rp::units(5, 65) != 5 || rp::units(64, 1) != 1 || rp::units(65, 1) != 2;
    mismatches += rp::piece_end(0, 1ull << 62, (1ull << 63) - 1) != (1ull << 62) ||
                  rp::piece_end(1, 1ull << 62, (1ull << 63) - 1) != (1ull << 63) - 1;
    mismatches += rp::shift(0x12345678u, 0, g_tab.v) != 0x12345678u;
    const uint64_t po = 16;
    // group A: k <= 64, g = 64 / k new pieces a wave
    for (uint64_t k : {1, 2, 3, 4, 5, 21, 22, 31, 32, 33, 63, 64}) {
        const uint64_t g = 64 / k;
        for (uint64_t n_new : {g - 1, g, g + 1, 2 * g, 2 * g + 1})
            for (uint64_t last_olds : {(uint64_t)1, k > 1 ? k - 1 : 1, k})
                for (uint64_t tail : {(uint64_t)1, po - 1, po}) {
                    const uint64_t length = n_new ? ((n_new - 1) * k + last_olds - 1) * po + tail : 0;
                    mismatches += check_bytes(length, po, k);
                    ++cases;
                }
    }
    // group B: k > 64, the lanes stride
    for (uint64_t k : {65, 127, 128, 129, 4097})
        for (uint64_t n_old : {k - 1, k, k + 1})
            for (uint64_t tail : {(uint64_t)1, po}) {
                mismatches += check_bytes((n_old - 1) * po + tail, po, k);
                ++cases;
            }
    // other old piece lengths, and a ratio that covers the blob
    for (uint64_t p : {1, 3, 64, 4096})
        for (uint64_t k : {1, 2, 3, 5, 63, 64, 65, 129, 1 << 20}) {
            mismatches += check_bytes(40000 + p / 2, p, k);
            ++cases;
        }
    // group F: 64-bit distances
    for (uint64_t k : {3, 129})
        for (uint64_t length : {(1ull << 40) - 12345, (1ull << 40) + 1, (1ull << 40) + (1ull << 33) + 777, (1ull << 41) + 5}) {
            mismatches += check_far(length, 1ull << 33, k);
            ++cases;
        }
    printf("repiece_math: %d cases, %d mismatches\n", cases, mismatches);
    return mismatches != 0;
}
