// digest_hex_math.hpp -- a cache listing's text turned into what the ring selection takes: the
// SHA-256 hex codec (core.NewSHA256DigestFromHex / ValidateSHA256 / Digest.Hex(),
// core/digest.go:57-68,143-161) and the expiry comparison of maybeDelete
// (origin/blobserver/server.go:686-759) and of the store's TTL/TTI rule readyForDeletion
// (lib/store/cleanup.go:112-155).  A name is 64 bytes held as 16 little-endian uint32 words (byte
// p is bits 8 (p & 3).. of word p >> 2), a digest 8 such words, so the host forms and
// digest_hex.hip run the same lines on registers.  Header-only, __host__ __device__ and free of
// the runtime, so that tests/native/digest_hex_math_main.cpp builds it stand-alone under
// AddressSanitizer and UndefinedBehaviorSanitizer.
//
// Listing layout (krk_metainfo_batch_dev's names / name_off): names are bytes back to back, off
// has n + 1 entries, name i is names[off[i], off[i + 1]), off[0] need not be 0.  Its length is
// the unsigned 64-bit difference; any length but 64 is a length error and no byte of that name
// is read (a decreasing pair is a length error like any other).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KRK_DH_HD __host__ __device__ __forceinline__
#else
#define KRK_DH_HD inline
#endif

// One status word a name: 0 valid; KRK_DHEX_LEN | min(len, 0x3FFFFFFF) for a length but 64;
// KRK_DHEX_BYTE | p << 8 | byte for the first byte, in index order, that is no hex digit
// (encoding/hex's InvalidByteError), p in 0..63.
#define KRK_DHEX_LEN 0x40000000u
#define KRK_DHEX_BYTE 0x80000000u
// A missing _last_access_time in an access-time column.
#define KRK_NO_TIME INT64_MIN

namespace krk {
namespace dh {

constexpr uint32_t kNameLen = 64;
constexpr uint32_t kLenMax = 0x3FFFFFFFu;

inline uint64_t words(uint64_t n) { return n / 64 + (n % 64 != 0); }

KRK_DH_HD uint32_t len_status(uint64_t len) {
    return len == kNameLen ? 0u : KRK_DHEX_LEN | (uint32_t)(len < kLenMax ? len : kLenMax);
}

// The value of hex digit c (either case), or a value above 15 for any other byte.
KRK_DH_HD uint32_t nibble(uint32_t c) {
    const uint32_t d = c - '0', a = (c | 0x20) - 'a';
    return d < 10 ? d : a < 6 ? a + 10 : 16u;
}

KRK_DH_HD uint32_t hex_char(uint32_t v) { return v + (v < 10 ? '0' : 'a' - 10); }

// 64 name bytes -> 32 digest bytes.  Returns 0, or the bad-byte status of the lowest position
// that is no hex digit; then d is all zero.
KRK_DH_HD uint32_t parse_words(const uint32_t w[16], uint32_t d[8]) {
    uint32_t first = kNameLen, any = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t j = 0; j < 8; ++j) {
        uint32_t out = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (uint32_t b = 0; b < 4; ++b) {  // digest byte 4 j + b from name bytes 8 j + 2 b, + 1
            const uint32_t p = 8 * j + 2 * b;
            const uint32_t pair = (w[p >> 2] >> (8 * (p & 3))) & 0xFFFFu;
            const uint32_t hi = nibble(pair & 0xFF), lo = nibble(pair >> 8);
            const uint32_t bad = hi > 15 ? p : lo > 15 ? p + 1 : kNameLen;
            first = bad < first ? bad : first;
            any |= hi | lo;
            out |= ((hi << 4 | lo) & 0xFF) << (8 * b);
        }
        d[j] = out;
    }
    if (any <= 15) return 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t j = 0; j < 8; ++j) d[j] = 0;
    uint32_t byte = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < 16; ++k)  // a select a word, no dynamic register index
        byte = (first >> 2) == k ? (w[k] >> (8 * (first & 3))) & 0xFF : byte;
    return KRK_DHEX_BYTE | first << 8 | byte;
}

// 32 digest bytes -> 64 lowercase characters (Digest.Hex()).
KRK_DH_HD void format_words(const uint32_t d[8], uint32_t h[16]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t j = 0; j < 16; ++j) {  // name bytes 4 j.. from digest bytes 2 j, 2 j + 1
        const uint32_t two = (d[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
        h[j] = hex_char((two >> 4) & 15) | hex_char(two & 15) << 8 | hex_char((two >> 12) & 15) << 16 |
               hex_char((two >> 8) & 15) << 24;
    }
}

// time.Time.Sub: the difference saturates at the int64 limits.
KRK_DH_HD int64_t sat_sub(int64_t a, int64_t b) {
    int64_t r;
    if (!__builtin_sub_overflow(a, b, &r)) return r;
    return b < 0 ? INT64_MAX : INT64_MIN;  // a - b overflowed upwards only when b is negative
}

// now.Sub(t) > d, strict, all in nanoseconds.
KRK_DH_HD bool expired(int64_t now, int64_t t, int64_t d) { return sat_sub(now, t) > d; }

#if !defined(__HIP_DEVICE_COMPILE__)
// ------------------------------------------------------------------ host forms
inline uint32_t load_le32(const uint8_t* p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
inline void store_le32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8), p[2] = (uint8_t)(v >> 16), p[3] = (uint8_t)(v >> 24);
}

struct NibbleTable {
    uint8_t v[256];
    NibbleTable() {
        for (uint32_t c = 0; c < 256; ++c) v[c] = (uint8_t)nibble(c);
    }
};

// Name i of a listing: its status, and its digest words (zero unless valid) in d.
inline uint32_t parse_name(const uint8_t* names, const uint64_t* off, uint64_t i, uint32_t d[8]) {
    const uint32_t ls = len_status(off[i + 1] - off[i]);
    if (ls) {
        for (uint32_t j = 0; j < 8; ++j) d[j] = 0;
        return ls;
    }
    // a valid name through a 256-entry table of nibble(); any other through parse_words, which
    // finds the status word (and gives the same digest for a valid name: the native test runs both)
    static const NibbleTable T;
    const uint8_t* p = names + off[i];
    uint32_t any = 0;
    for (uint32_t j = 0; j < 8; ++j) {
        uint32_t out = 0;
        for (uint32_t b = 0; b < 4; ++b) {
            const uint32_t hi = T.v[p[8 * j + 2 * b]], lo = T.v[p[8 * j + 2 * b + 1]];
            any |= hi | lo;
            out |= ((hi << 4 | lo) & 0xFF) << (8 * b);
        }
        d[j] = out;
    }
    if (any <= 15) return 0;
    uint32_t w[16];
    for (uint32_t k = 0; k < 16; ++k) w[k] = load_le32(p + 4 * k);
    return parse_words(w, d);
}

// Every digest byte, status word (nullable) and valid word (nullable; words(n) of them, tail
// bits 0) is stored.
inline void parse_listing(const uint8_t* names, const uint64_t* off, uint64_t n, uint8_t* digests32, uint32_t* status,
                          uint64_t* valid) {
    for (uint64_t w = 0; w * 64 < n; ++w) {
        const uint64_t m = n - w * 64 < 64 ? n - w * 64 : 64;
        uint64_t word = 0;
        for (uint64_t l = 0; l < m; ++l) {
            const uint64_t i = w * 64 + l;
            uint32_t d[8];
            const uint32_t st = parse_name(names, off, i, d);
            for (uint32_t j = 0; j < 8; ++j) store_le32(digests32 + 32 * i + 4 * j, d[j]);
            if (status) status[i] = st;
            word |= (uint64_t)(st == 0) << l;
        }
        if (valid) valid[w] = word;
    }
}

inline void format_listing(const uint8_t* digests32, uint64_t n, uint8_t* hex) {
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t d[8], h[16];
        for (uint32_t j = 0; j < 8; ++j) d[j] = load_le32(digests32 + 32 * i + 4 * j);
        format_words(d, h);
        for (uint32_t k = 0; k < 16; ++k) store_le32(hex + 64 * i + 4 * k, h[k]);
    }
}

// bit i = (mtime && expired(now, mtime[i], ttl)) || (atime && atime[i] != KRK_NO_TIME &&
// expired(now, atime[i], tti)); words(n) words, tail bits 0, every word stored.
inline void expiry_bits(const int64_t* mtime, const int64_t* atime, uint64_t n, int64_t now, int64_t ttl, int64_t tti,
                        uint64_t* bits) {
    for (uint64_t w = 0; w * 64 < n; ++w) {
        const uint64_t m = n - w * 64 < 64 ? n - w * 64 : 64;
        uint64_t word = 0;
        for (uint64_t l = 0; l < m; ++l) {
            const uint64_t i = w * 64 + l;
            const bool e = (mtime && expired(now, mtime[i], ttl)) ||
                           (atime && atime[i] != KRK_NO_TIME && expired(now, atime[i], tti));
            word |= (uint64_t)e << l;
        }
        bits[w] = word;
    }
}

// sel(i) = valid(i) & ((mask[ShardID(d_i)] ^ invert) | expired(now, mtime[i], ttl)); mtime
// NULL: no expiry term.  bits / idx / idx_cap / the returned count as rs::select; valid
// (nullable) as parse_listing's.
inline uint64_t cleanup_plan(const uint8_t* names, const uint64_t* off, uint64_t n, const int64_t* mtime, int64_t now,
                             int64_t ttl, const uint64_t* mask, bool invert, uint64_t* bits, uint64_t* valid,
                             uint64_t* idx, uint64_t idx_cap) {
    uint64_t count = 0;
    for (uint64_t w = 0; w * 64 < n; ++w) {
        const uint64_t m = n - w * 64 < 64 ? n - w * 64 : 64;
        uint64_t word = 0, ok = 0;
        for (uint64_t l = 0; l < m; ++l) {
            const uint64_t i = w * 64 + l;
            uint32_t d[8];
            if (parse_name(names, off, i, d)) continue;
            const uint32_t s = (d[0] & 0xFF) << 8 | ((d[0] >> 8) & 0xFF);  // ShardID: digest bytes 0, 1
            const bool sel = ((((mask[s >> 6] >> (s & 63)) & 1) != 0) != invert) || (mtime && expired(now, mtime[i], ttl));
            ok |= 1ull << l;
            word |= (uint64_t)sel << l;
        }
        bits[w] = word;
        if (valid) valid[w] = ok;
        for (uint64_t x = word; x; x &= x - 1) {
            if (idx && count < idx_cap) idx[count] = w * 64 + (uint64_t)__builtin_ctzll(x);
            ++count;
        }
    }
    return count;
}
#endif  // !__HIP_DEVICE_COMPILE__

}  // namespace dh
}  // namespace krk
