// engine_math.hpp -- the submission engine's piece arithmetic: how a CRC request
// over stream bytes [a, a + len) is cut at the multiples of the piece length (portions(), what
// launch_crc of engine.cpp lays out as items and runs), and how the portions' CRCs, each hashed as an
// independent message, fold back into the stream's piece sums in submission order (fold(), what
// stream_fold of piece_stream.cpp runs on the completer thread).  On finalised IEEE sums (crc_math.hpp)
//     crc(A || B) = shift(crc(A), |B|) ^ crc(B),      shift(c, n) = c * x^(8n) mod P,
// so a portion that starts a piece sets the piece's sum and one that continues a piece shifts the
// sum by its own length and XORs its CRC in.  Header-only and free of the runtime, so that
// tests/native/engine_math_main.cpp builds it stand-alone under AddressSanitizer and
// UndefinedBehaviorSanitizer.  All offset, index and distance arithmetic is 64-bit.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "crc_math.hpp"

namespace krk {
namespace em {

// Portions of stream bytes [a, a+len) cut at multiples of P (P == 0: one portion).
struct Portions {
    uint64_t first_end;  // end of the first portion
    uint64_t f0, f1;     // whole pieces [f0, f1) strictly inside
    bool head, tail;     // a partial portion before / after the whole pieces
    uint64_t count;
};

inline Portions portions(uint64_t a, uint64_t len, uint64_t P) {
    Portions p{};
    const uint64_t b = a + len;
    if (!len) return p;
    if (P == 0) {
        p.head = true;
        p.first_end = b;
        p.count = 1;
        return p;
    }
    p.f0 = (a + P - 1) / P;
    p.f1 = b / P;
    if (p.f1 < p.f0) {  // inside one piece, touching neither boundary
        p.head = true;
        p.first_end = b;
        p.f0 = p.f1 = 0;
        p.count = 1;
        return p;
    }
    p.head = a < p.f0 * P;
    p.tail = b > p.f1 * P;
    p.first_end = p.head ? p.f0 * P : a;
    p.count = (p.head ? 1 : 0) + (p.f1 - p.f0) + (p.tail ? 1 : 0);
    return p;
}

// Fold the n portion CRCs of the request over stream bytes [off, off + len), pieces of P > 0
// bytes, into sums (one entry a piece begun so far), the stream's requests in submission order.
// False = "broken order": a portion continues a piece that no earlier portion began; the portions
// before it stay folded, nothing after it is.
inline bool fold(std::vector<uint32_t>& sums, uint64_t off, uint64_t len, uint64_t P, const uint32_t* crcs, size_t n,
                 const uint32_t* x8pow) {
    const uint64_t b = off + len;
    uint64_t q = off;
    for (size_t k = 0; k < n; ++k) {
        const uint64_t pi = q / P;
        const uint64_t next = (pi + 1) * P;
        const uint64_t e = b < next ? b : next;
        if (q % P == 0) {
            if (sums.size() <= pi) sums.resize(pi + 1);
            sums[pi] = crcs[k];
        } else if (pi < sums.size()) {
            sums[pi] = gf2_mulmod(sums[pi], x8n(e - q, x8pow)) ^ crcs[k];
        } else {  // a continuation with no start: never expected in submission order
            return false;
        }
        q = e;
    }
    return true;
}

}  // namespace em
}  // namespace krk
