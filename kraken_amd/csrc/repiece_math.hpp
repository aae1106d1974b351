// repiece_math.hpp -- stored piece sums re-pieced to a coarser piece length with no blob byte
// read (krk_repiece_sums, krk_repiece_batch, piece_repiece.hip).  On finalised IEEE sums the
// init / xor-out terms cancel under concatenation (crc_math.hpp):
//     crc(A || B) = shift(crc(A), |B|) ^ crc(B),      shift(c, n) = c * x^(8n) mod P,
// so with new pieces of k old pieces each, new piece j's sum is the XOR, over the old pieces i it
// covers, of shift(old_sum_i, d_i), d_i = the bytes from old piece i's end to new piece j's end.
// Multiplying by x^n is a bijection mod P (P has a constant term): a wrong old sum stays visible.
// The host entry points and the kernel both call term(); header-only and free of the runtime, so
// that tests/native/repiece_math_main.cpp builds it stand-alone under AddressSanitizer and
// UndefinedBehaviorSanitizer.  All index and distance arithmetic is 64-bit.
#pragma once
#include <stdint.h>

#include "crc_math.hpp"

namespace krk {
namespace rp {

// The krk_num_pieces rule: ceil(length / piece_length), none for an empty blob.
KRK_HD uint64_t num_pieces(uint64_t length, uint64_t piece_length) {
    return length / piece_length + (length % piece_length != 0);
}

// The end of piece i (i < num_pieces) of a blob cut into pieces of piece_length bytes; formed
// from length - i * piece_length, so a piece length near 2^63 does not overflow.
KRK_HD uint64_t piece_end(uint64_t i, uint64_t piece_length, uint64_t length) {
    const uint64_t start = i * piece_length;
    return length - start <= piece_length ? length : start + piece_length;
}

// d_i: the bytes from old piece i's end to the end of the new piece (k old pieces each) it is in.
KRK_HD uint64_t distance(uint64_t i, uint64_t po, uint64_t k, uint64_t length) {
    return piece_end(i / k, po * k, length) - piece_end(i, po, length);
}

// shift(c, n) = c * x^(8n) mod P over the x^(8 * 2^b) power table (crc_math.hpp x8n, started
// from c instead of 1).
KRK_HD uint32_t shift(uint32_t c, uint64_t n, const uint32_t* x8pow) {
    for (int b = 0; n; ++b, n >>= 1)
        if (n & 1) c = gf2_mulmod(c, x8pow[b]);
    return c;
}

// Old piece i's term of its new piece's sum.
KRK_HD uint32_t term(uint32_t old_sum, uint64_t i, uint64_t po, uint64_t k, uint64_t length, const uint32_t* x8pow) {
    return shift(old_sum, distance(i, po, k, length), x8pow);
}

// The kernel's decomposition: new pieces a unit (one wave's work) and units a blob.  k <= 64:
// 64 / k consecutive new pieces, one old piece a lane; k > 64: one new piece.
constexpr uint64_t kLanes = 64;
KRK_HD uint64_t pieces_per_unit(uint64_t k) { return k <= kLanes ? kLanes / k : 1; }
KRK_HD uint64_t units(uint64_t n_new, uint64_t k) {
    const uint64_t g = pieces_per_unit(k);
    return n_new / g + (n_new % g != 0);
}

// One blob on the host: out[0, num_pieces(length, po * k)) from old[0, num_pieces(length, po)).
inline void repiece(const uint32_t* old, uint64_t length, uint64_t po, uint64_t k, uint32_t* out,
                    const uint32_t* x8pow) {
    const uint64_t n_old = num_pieces(length, po);
    for (uint64_t i = 0; i < n_old;) {
        const uint64_t m = n_old - i < k ? n_old - i : k;  // old pieces of new piece i / k
        uint32_t s = 0;
        for (uint64_t e = i + m; i < e; ++i) s ^= term(old[i], i, po, k, length, x8pow);
        out[(i - 1) / k] = s;
    }
}

}  // namespace rp
}  // namespace krk
