// info_hash_math_main.cpp -- the device InfoHash's arithmetic (kraken_amd/csrc/info_hash_math.hpp)
// as a stand-alone CPU program, meant for the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -o info_hash_math_san info_hash_math_main.cpp && ./info_hash_math_san
// (tests/test_info_hash_math_native.py does exactly that).  It links nothing of the library:
// the header's stream -- header, name, sums through the byte ring, padding, SHA-1 blocks, one
// lane after another as the kernel's 64 lanes do it -- is compared with a textbook bencode
// (snprintf) + SHA-1 written here, on the reference's known answer, every decimal width,
// the int64 edges, every padding residue and the 64-lane step edges.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../kraken_amd/csrc/info_hash_math.hpp"

namespace ih = krk::ih;

static void via_header(int64_t P, const std::vector<uint32_t>& sums, const std::string& name, int64_t L,
                       uint8_t out[20]) {
    uint32_t ring[ih::kRingWords] = {};
    uint8_t* ring8 = reinterpret_cast<uint8_t*>(ring);
    uint32_t h[5];
    ih::sha1_init(h);
    uint64_t pos = 0, done = 0;
    auto put = [&](uint64_t at, uint8_t c) { ring8[ih::ring_byte(at)] = c; };
    auto drain = [&] {
        for (; pos - done >= 64; done += 64) {
            uint32_t w[16];
            memcpy(w, ring + ih::ring_block(done), sizeof w);
            ih::sha1_block(h, w);
        }
    };
    pos += ih::header_before_name(L, name.size(), pos, put);
    drain();
    for (size_t base = 0; base < name.size(); base += 64) {
        const size_t m = name.size() - base < 64 ? name.size() - base : 64;
        for (size_t l = 0; l < m; ++l) put(pos + l, (uint8_t)name[base + l]);
        pos += m;
        drain();
    }
    pos += ih::header_after_name(P, pos, put);
    drain();
    for (size_t base = 0; base < sums.size(); base += 64) {
        const size_t m = sums.size() - base < 64 ? sums.size() - base : 64;
        uint32_t off = 0;
        for (size_t l = 0; l < m; ++l) {
            const uint32_t v = sums[base + l], nd = ih::digits(v);
            ih::emit_sum(v, nd, pos + off, put);
            off += nd + 2;
        }
        pos += off;
        drain();
    }
    put(pos, 'e');
    put(pos + 1, 'e');
    pos += 2;
    const uint64_t total = pos;
    const uint32_t n_pad = ih::pad_bytes(total);
    for (uint32_t k = 0; k < n_pad; ++k) put(total + k, ih::pad_byte(k, n_pad, total));
    pos += n_pad;
    drain();
    for (uint32_t k = 0; k < 20; ++k) out[k] = ih::digest_byte(h, k);
}

static void textbook(int64_t P, const std::vector<uint32_t>& sums, const std::string& name, int64_t L,
                     uint8_t out[20]) {
    char num[64];
    std::string s = "d6:Lengthi";
    snprintf(num, sizeof num, "%" PRId64, L);
    s += num;
    s += "e4:Name";
    snprintf(num, sizeof num, "%zu:", name.size());
    s += num;
    s += name;
    s += "11:PieceLengthi";
    snprintf(num, sizeof num, "%" PRId64, P);
    s += num;
    s += "e9:PieceSumsl";
    for (uint32_t v : sums) {
        snprintf(num, sizeof num, "i%" PRIu32 "e", v);
        s += num;
    }
    s += "ee";
    const uint64_t bits = (uint64_t)s.size() * 8;
    s.push_back((char)0x80);
    while (s.size() % 64 != 56) s.push_back(0);
    for (int i = 7; i >= 0; --i) s.push_back((char)(bits >> (8 * i)));
    uint32_t h[5] = {0x67452301u, 0xEFCDAB89u, 0x98BADCFEu, 0x10325476u, 0xC3D2E1F0u};
    for (size_t b = 0; b < s.size(); b += 64) {
        uint32_t w[80];
        for (int t = 0; t < 16; ++t)
            w[t] = (uint32_t)(uint8_t)s[b + 4 * t] << 24 | (uint32_t)(uint8_t)s[b + 4 * t + 1] << 16 |
                   (uint32_t)(uint8_t)s[b + 4 * t + 2] << 8 | (uint32_t)(uint8_t)s[b + 4 * t + 3];
        for (int t = 16; t < 80; ++t) {
            const uint32_t x = w[t - 3] ^ w[t - 8] ^ w[t - 14] ^ w[t - 16];
            w[t] = x << 1 | x >> 31;
        }
        uint32_t a = h[0], bb = h[1], c = h[2], d = h[3], e = h[4];
        for (int t = 0; t < 80; ++t) {
            uint32_t f, k;
            if (t < 20) { f = (bb & c) | (~bb & d); k = 0x5A827999u; }
            else if (t < 40) { f = bb ^ c ^ d; k = 0x6ED9EBA1u; }
            else if (t < 60) { f = (bb & c) | (bb & d) | (c & d); k = 0x8F1BBCDCu; }
            else { f = bb ^ c ^ d; k = 0xCA62C1D6u; }
            const uint32_t tmp = (a << 5 | a >> 27) + f + e + k + w[t];
            e = d;
            d = c;
            c = bb << 30 | bb >> 2;
            bb = a;
            a = tmp;
        }
        h[0] += a; h[1] += bb; h[2] += c; h[3] += d; h[4] += e;
    }
    for (int k = 0; k < 20; ++k) out[k] = (uint8_t)(h[k / 4] >> (24 - 8 * (k % 4)));
}

static int g_fail = 0, g_cases = 0;
static void check(int64_t P, const std::vector<uint32_t>& sums, const std::string& name, int64_t L, const char* what) {
    uint8_t a[20], b[20];
    via_header(P, sums, name, L, a);
    textbook(P, sums, name, L, b);
    ++g_cases;
    if (memcmp(a, b, 20) != 0) {
        ++g_fail;
        fprintf(stderr, "MISMATCH %s: P=%" PRId64 " n_sums=%zu name_len=%zu L=%" PRId64 "\n", what, P, sums.size(),
                name.size(), L);
    }
}

int main() {
    // core/metainfo_test.go:61-76
    {
        uint8_t a[20];
        char hex[41];
        via_header(4194304, {2131691452u}, "289314c356bc2a19802c3e31505506db30ea81a0bcaea4ec3e079524c8ac3cf5", 236, a);
        for (int k = 0; k < 20; ++k) snprintf(hex + 2 * k, 3, "%02x", a[k]);
        ++g_cases;
        if (strcmp(hex, "85b978c4377625b3963df406d0dd3a1da5a7d9c3") != 0) {
            ++g_fail;
            fprintf(stderr, "MISMATCH reference KAT: %s\n", hex);
        }
    }
    std::vector<uint32_t> widths = {0, 2147483647u, 2147483648u, 4294967295u};
    for (uint32_t p = 10, k = 1; k < 10; ++k, p *= 10) {
        widths.push_back(p - 1);
        widths.push_back(p);
        if (k == 9) break;
    }
    check(4 << 20, widths, "digits", 5, "all widths");
    for (uint32_t v : widths)
        for (size_t reps : {size_t(1), size_t(64), size_t(65)}) check(1 << 20, std::vector<uint32_t>(reps, v), "abc", 77, "width step");
    const int64_t edges[] = {0, 1, 9, 10, int64_t(1) << 31, INT64_MAX, -1, INT64_MIN};
    for (int64_t L : edges)
        for (int64_t P : edges) check(P, {1, 22, 333}, "xxxxxxx", L, "int64");
    for (size_t n = 0; n <= 130; ++n) {
        std::string name(n, 'a');
        for (size_t i = 0; i < n; ++i) name[i] = (char)(33 + (7 * i + n) % 90);
        check(1, {}, name, 0, "residue");
    }
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (size_t n : {size_t(0), size_t(1), size_t(63), size_t(64), size_t(65), size_t(127), size_t(128), size_t(129),
                     size_t(1000), size_t(4097), size_t(81920)}) {
        std::vector<uint32_t> s(n);
        for (size_t i = 0; i < n; ++i) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            s[i] = (uint32_t)(x >> 32) >> ((x >> 8) % 32);
        }
        check(1 << 20, s, std::string(2 * (n % 50) + 1, 'n'), (int64_t)n << 20, "tile edge");
    }
    printf("info_hash_math: %d cases, %d mismatches\n", g_cases, g_fail);
    return g_fail ? 1 : 0;
}
