// info_hash_math.hpp -- the arithmetic of the device InfoHash (info_hash.hip), host and device:
// decimal digit count and emit (multiply-high by reciprocal constants: no divide, no floating
// point), the bencode header of core.info as bencode_info (host_meta.cpp) writes it, the
// SHA-1 padding bytes, the byte ring the stream is formatted into, and the SHA-1 block
// function.  The kernel runs these 64 lanes at a time; krk_info_hash_math_host
// (info_hash_dev.cpp) and tests/native/info_hash_math_main.cpp run the same functions one
// lane after another on the CPU.  Nothing here needs the HIP headers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KRK_IH_HD __host__ __device__ __forceinline__
#else
#define KRK_IH_HD inline
#endif

namespace krk {
namespace ih {

// ------------------------------------------------------------------ the byte ring
// Stream byte p lives at ring byte (p mod kRingBytes) ^ 3: a SHA-1 block is then sixteen
// consecutive little-endian words of the ring, already in the big-endian order SHA-1 reads.
// A step adds at most 64 x 12 bytes ("i" + 10 digits + "e" a lane) to a remainder below 64.
constexpr uint32_t kRingBytes = 1024;
constexpr uint32_t kRingWords = kRingBytes / 4;
constexpr uint32_t kMaxStepBytes = 64 * 12;
static_assert(63 + kMaxStepBytes <= kRingBytes, "a step's bytes plus the remainder fit the ring");

KRK_IH_HD uint32_t ring_byte(uint64_t pos) { return ((uint32_t)pos & (kRingBytes - 1)) ^ 3u; }
// first word of the block at stream offset `done` (a multiple of 64: a block never wraps)
KRK_IH_HD uint32_t ring_block(uint64_t done) { return ((uint32_t)done & (kRingBytes - 1)) >> 2; }

// ------------------------------------------------------------------ decimal
KRK_IH_HD uint32_t mulhi32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}
KRK_IH_HD uint64_t mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}
// floor(v / 10), exact for every v: ceil(2^35 / 10) and ceil(2^67 / 10)
KRK_IH_HD uint32_t div10(uint32_t v) { return mulhi32(v, 0xCCCCCCCDu) >> 3; }
KRK_IH_HD uint64_t div10(uint64_t v) { return mulhi64(v, 0xCCCCCCCCCCCCCCCDull) >> 3; }

// Decimal digits of v, no leading zeros (1 for 0): a compare ladder.
KRK_IH_HD uint32_t digits(uint32_t v) {
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) +
           (v >= 10000000u) + (v >= 100000000u) + (v >= 1000000000u);
}
KRK_IH_HD uint32_t digits(uint64_t v) {
    uint32_t nd = 1;
    uint64_t p = 10;
    for (int k = 0; k < 19; ++k) {  // p = 10^1 .. 10^19, the last below 2^64
        nd += v >= p;
        p *= 10;  // past 10^19 the product wraps and is not used
    }
    return nd;
}

// The nd = digits(v) digits of v at stream bytes [at, at + nd): put(position, byte).
template <class Put>
KRK_IH_HD void emit(uint32_t v, uint32_t nd, uint64_t at, Put&& put) {
#pragma unroll
    for (uint32_t k = 0; k < 10; ++k) {
        const uint32_t q = div10(v);
        if (k < nd) put(at + (nd - 1 - k), (uint8_t)('0' + (v - q * 10u)));
        v = q;
    }
}
template <class Put>
KRK_IH_HD void emit(uint64_t v, uint32_t nd, uint64_t at, Put&& put) {
    for (uint32_t k = 0; k < nd; ++k) {
        const uint64_t q = div10(v);
        put(at + (nd - 1 - k), (uint8_t)('0' + (uint32_t)(v - q * 10u)));
        v = q;
    }
}
// put_i64 of host_meta.cpp: '-' and the magnitude for a negative value.  Returns the bytes.
template <class Put>
KRK_IH_HD uint32_t emit_i64(int64_t v, uint64_t at, Put&& put) {
    uint32_t n = 0;
    uint64_t m = (uint64_t)v;
    if (v < 0) {
        put(at, (uint8_t)'-');
        n = 1;
        m = (uint64_t)0 - m;
    }
    const uint32_t nd = digits(m);
    emit(m, nd, at + n, put);
    return n + nd;
}
// One list element "i<sum>e" of nd = digits(sum) digits: nd + 2 bytes at `at`.
template <class Put>
KRK_IH_HD void emit_sum(uint32_t sum, uint32_t nd, uint64_t at, Put&& put) {
    put(at, (uint8_t)'i');
    emit(sum, nd, at + 1, put);
    put(at + 1 + nd, (uint8_t)'e');
}

// ------------------------------------------------------------------ the header
template <class Put>
KRK_IH_HD uint32_t emit_text(const char* s, uint32_t n, uint64_t at, Put&& put) {
    for (uint32_t k = 0; k < n; ++k) put(at + k, (uint8_t)s[k]);
    return n;
}
// "d6:Lengthi<L>e4:Name<len>:" -- what precedes the name's bytes (at most 58 bytes).
template <class Put>
KRK_IH_HD uint32_t header_before_name(int64_t length, uint64_t name_len, uint64_t at, Put&& put) {
    uint32_t n = emit_text("d6:Lengthi", 10, at, put);
    n += emit_i64(length, at + n, put);
    n += emit_text("e4:Name", 7, at + n, put);
    n += emit_i64((int64_t)name_len, at + n, put);
    n += emit_text(":", 1, at + n, put);
    return n;
}
// "11:PieceLengthi<P>e9:PieceSumsl" -- between the name and the sums (at most 48 bytes).
template <class Put>
KRK_IH_HD uint32_t header_after_name(int64_t piece_length, uint64_t at, Put&& put) {
    uint32_t n = emit_text("11:PieceLengthi", 15, at, put);
    n += emit_i64(piece_length, at + n, put);
    n += emit_text("e9:PieceSumsl", 13, at + n, put);
    return n;
}
constexpr uint32_t kMaxHeaderPart = 58;

// ------------------------------------------------------------------ SHA-1
// Padding of a message of `total` bytes: 0x80, zeros to 56 mod 64, the bit length big-endian.
KRK_IH_HD uint32_t pad_bytes(uint64_t total) { return ((55u - (uint32_t)total) & 63u) + 9u; }  // 9 .. 72
KRK_IH_HD uint8_t pad_byte(uint32_t k, uint32_t n_pad, uint64_t total) {
    if (k == 0) return 0x80;
    if (k + 8 < n_pad) return 0;
    return (uint8_t)((total * 8) >> (8 * (n_pad - 1 - k)));
}

KRK_IH_HD uint32_t rotl(uint32_t x, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(x, x, 32 - n);
#else
    return (x << n) | (x >> (32 - n));
#endif
}
// The round functions, one v_bitop3_b32 each on the device (truth tables over b, c, d).
KRK_IH_HD uint32_t f_ch(uint32_t b, uint32_t c, uint32_t d) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(b, c, d, 0xCA);
#else
    return (b & c) | (~b & d);
#endif
}
KRK_IH_HD uint32_t f_parity(uint32_t b, uint32_t c, uint32_t d) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(b, c, d, 0x96);
#else
    return b ^ c ^ d;
#endif
}
KRK_IH_HD uint32_t f_maj(uint32_t b, uint32_t c, uint32_t d) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(b, c, d, 0xE8);
#else
    return (b & c) | (b & d) | (c & d);
#endif
}

KRK_IH_HD void sha1_init(uint32_t h[5]) {
    h[0] = 0x67452301u;
    h[1] = 0xEFCDAB89u;
    h[2] = 0x98BADCFEu;
    h[3] = 0x10325476u;
    h[4] = 0xC3D2E1F0u;
}

// One 64-byte block: w[16] big-endian message words (overwritten by the schedule).
KRK_IH_HD void sha1_block(uint32_t h[5], uint32_t w[16]) {
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
#define KRK_IH_W(t) \
    (w[(t) & 15] = rotl(f_parity(w[((t) + 13) & 15], w[((t) + 8) & 15], w[((t) + 2) & 15]) ^ w[(t) & 15], 1))
#define KRK_IH_ROUND(f, k, x)                         \
    {                                                 \
        const uint32_t t_ = rotl(a, 5) + f(b, c, d) + e + (k) + (x); \
        e = d;                                        \
        d = c;                                        \
        c = rotl(b, 30);                              \
        b = a;                                        \
        a = t_;                                       \
    }
#pragma unroll
    for (int t = 0; t < 16; ++t) KRK_IH_ROUND(f_ch, 0x5A827999u, w[t])
#pragma unroll
    for (int t = 16; t < 20; ++t) KRK_IH_ROUND(f_ch, 0x5A827999u, KRK_IH_W(t))
#pragma unroll
    for (int t = 20; t < 40; ++t) KRK_IH_ROUND(f_parity, 0x6ED9EBA1u, KRK_IH_W(t))
#pragma unroll
    for (int t = 40; t < 60; ++t) KRK_IH_ROUND(f_maj, 0x8F1BBCDCu, KRK_IH_W(t))
#pragma unroll
    for (int t = 60; t < 80; ++t) KRK_IH_ROUND(f_parity, 0xCA62C1D6u, KRK_IH_W(t))
#undef KRK_IH_ROUND
#undef KRK_IH_W
    h[0] += a;
    h[1] += b;
    h[2] += c;
    h[3] += d;
    h[4] += e;
}
// Digest byte k (0 .. 19) of the state.
KRK_IH_HD uint8_t digest_byte(const uint32_t h[5], uint32_t k) {
    const uint32_t q = k >> 2;
    const uint32_t v = q == 0 ? h[0] : q == 1 ? h[1] : q == 2 ? h[2] : q == 3 ? h[3] : h[4];
    return (uint8_t)(v >> (24 - 8 * (k & 3)));
}

}  // namespace ih
}  // namespace krk
