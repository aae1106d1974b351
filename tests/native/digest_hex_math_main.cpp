// The digest hex codec's and the expiry rule's arithmetic (kraken_amd/csrc/digest_hex_math.hpp:
// what krk_digest_parse_hex, krk_digest_format_hex, krk_expiry_bits and krk_cleanup_plan run and
// digest_hex.hip equals) as a stand-alone program: the status words, the saturating subtraction
// at both int64 limits, and parse / format against a bytewise table, over exactly sized heap
// arrays (so an overrun is the sanitizer's to report).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../kraken_amd/csrc/digest_hex_math.hpp"

using namespace krk;

static uint64_t rnd(uint64_t& x) {
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
    return x;
}

static int tab[256];  // a byte's hex value, -1 for a byte that is no hex digit

// The contract a byte at a time: status and digest of one name.
static uint32_t ref_parse(const std::string& s, uint8_t d[32]) {
    memset(d, 0, 32);
    if (s.size() != 64) return KRK_DHEX_LEN | (uint32_t)(s.size() < 0x3FFFFFFF ? s.size() : 0x3FFFFFFF);
    for (uint32_t p = 0; p < 64; ++p)
        if (tab[(uint8_t)s[p]] < 0) return KRK_DHEX_BYTE | p << 8 | (uint8_t)s[p];
    for (uint32_t j = 0; j < 32; ++j) d[j] = (uint8_t)(tab[(uint8_t)s[2 * j]] << 4 | tab[(uint8_t)s[2 * j + 1]]);
    return 0;
}

// A listing through dh::parse_listing / format_listing / cleanup_plan against ref_parse.
static int check_listing(const std::vector<std::string>& list, uint64_t lead, int& cases) {
    const uint64_t n = list.size();
    uint64_t total = lead;
    for (auto& s : list) total += s.size();
    uint8_t* text = (uint8_t*)malloc(total ? total : 1);
    uint64_t* off = (uint64_t*)malloc((n + 1) * 8);
    memset(text, 'g', lead);
    off[0] = lead;
    for (uint64_t i = 0; i < n; ++i) {
        memcpy(text + off[i], list[i].data(), list[i].size());
        off[i + 1] = off[i] + list[i].size();
    }
    const uint64_t nw = dh::words(n);
    uint8_t* dig = (uint8_t*)malloc(n ? 32 * n : 1);
    uint32_t* st = (uint32_t*)malloc(n ? 4 * n : 1);
    uint64_t* valid = (uint64_t*)malloc(nw ? 8 * nw : 1);
    memset(dig, 0xFF, 32 * n), memset(st, 0xFF, 4 * n), memset(valid, 0xFF, 8 * nw);
    dh::parse_listing(text, off, n, dig, st, valid);
    int wrong = 0;
    std::vector<uint8_t> okv(n);
    for (uint64_t i = 0; i < n; ++i) {
        uint8_t d[32];
        const uint32_t want = ref_parse(list[i], d);
        okv[i] = want == 0;
        if (list[i].size() == 64) {  // the word form on its own (the device's lines), whatever parse_name took
            uint32_t w[16], dw[8];
            uint8_t db[32];
            for (uint32_t k = 0; k < 16; ++k) w[k] = dh::load_le32((const uint8_t*)list[i].data() + 4 * k);
            wrong += dh::parse_words(w, dw) != want;
            for (uint32_t j = 0; j < 8; ++j) dh::store_le32(db + 4 * j, dw[j]);
            wrong += memcmp(d, db, 32) != 0;
        }
        wrong += st[i] != want;
        wrong += memcmp(d, dig + 32 * i, 32) != 0;
    }
    for (uint64_t b = 0; b < nw * 64; ++b) wrong += ((valid[b / 64] >> (b % 64)) & 1) != (b < n && okv[b] ? 1u : 0u);
    // without the nullable outputs: the same digests
    uint8_t* dig2 = (uint8_t*)malloc(n ? 32 * n : 1);
    dh::parse_listing(text, off, n, dig2, nullptr, nullptr);
    wrong += n && memcmp(dig, dig2, 32 * n) != 0;
    // format: lowercase, and parse(format(d)) == d
    uint8_t* hex = (uint8_t*)malloc(n ? 64 * n : 1);
    dh::format_listing(dig, n, hex);
    for (uint64_t i = 0; i < n; ++i)
        for (uint32_t j = 0; j < 32; ++j) {
            const uint8_t b = dig[32 * i + j];
            wrong += hex[64 * i + 2 * j] != "0123456789abcdef"[b >> 4] || hex[64 * i + 2 * j + 1] != "0123456789abcdef"[b & 15];
        }
    // the plan: valid & ((mask ^ invert) | expired) with a mask of the even shards
    uint64_t mask[1024];
    for (auto& m : mask) m = 0x5555555555555555ull;
    int64_t* mt = (int64_t*)malloc(n ? 8 * n : 1);
    const int64_t now = 1000, ttl = 10;
    for (uint64_t i = 0; i < n; ++i) mt[i] = now - ttl - (int64_t)(i % 3);  // i % 3 == 0: not expired
    for (int invert = 0; invert < 2; ++invert)
        for (int with_mt = 0; with_mt < 2; ++with_mt) {
            std::vector<uint64_t> want;
            for (uint64_t i = 0; i < n; ++i) {
                const uint32_t s = (uint32_t)dig[32 * i] << 8 | dig[32 * i + 1];
                const bool m = (s % 2 == 0) != (invert != 0);
                if (okv[i] && (m || (with_mt && i % 3 != 0))) want.push_back(i);
            }
            const uint64_t c = want.size();
            for (uint64_t cap : {(uint64_t)0, c ? c - 1 : 0, c, c + 1}) {
                uint64_t* bits = (uint64_t*)malloc(nw ? 8 * nw : 1);
                uint64_t* idx = cap ? (uint64_t*)malloc(8 * cap) : nullptr;
                memset(bits, 0xFF, 8 * nw);
                if (cap) memset(idx, 0xFF, 8 * cap);
                memset(valid, 0xFF, 8 * nw);
                const uint64_t got = dh::cleanup_plan(text, off, n, with_mt ? mt : nullptr, now, ttl, mask, invert != 0,
                                                      bits, valid, idx, cap);
                wrong += got != c;
                uint64_t k = 0;
                for (uint64_t b = 0; b < nw * 64; ++b) {
                    const bool sel = k < c && want[k] == b;
                    wrong += ((bits[b / 64] >> (b % 64)) & 1) != (sel ? 1u : 0u);
                    wrong += ((valid[b / 64] >> (b % 64)) & 1) != (b < n && okv[b] ? 1u : 0u);
                    if (sel) {
                        if (k < cap) wrong += idx[k] != b;
                        ++k;
                    }
                }
                for (uint64_t j = c; j < cap; ++j) wrong += idx[j] != ~0ull;
                free(bits), free(idx);
                ++cases;
            }
        }
    free(text), free(off), free(dig), free(dig2), free(st), free(valid), free(hex), free(mt);
    ++cases;
    return wrong;
}

int main() {
    for (int c = 0; c < 256; ++c)
        tab[c] = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
    int wrong = 0, cases = 0;
    // the nibble and the character tables
    for (uint32_t c = 0; c < 256; ++c) wrong += (dh::nibble(c) > 15 ? -1 : (int)dh::nibble(c)) != tab[c];
    for (uint32_t v = 0; v < 16; ++v) wrong += dh::hex_char(v) != (uint32_t)"0123456789abcdef"[v];
    // length status words
    const uint64_t lens[] = {0, 1, 63, 65, 66, 128, 0x3FFFFFFE, 0x3FFFFFFF, 0x40000000, 1ull << 32, ~0ull, ~0ull - 62};
    for (uint64_t len : lens)
        wrong += dh::len_status(len) != (KRK_DHEX_LEN | (uint32_t)(len < 0x3FFFFFFF ? len : 0x3FFFFFFF));
    wrong += dh::len_status(64) != 0;
    // the saturating subtraction and the strict comparison
    const int64_t MIN = INT64_MIN, MAX = INT64_MAX;
    wrong += dh::sat_sub(MAX, -1) != MAX;
    wrong += dh::sat_sub(MAX, MIN) != MAX;
    wrong += dh::sat_sub(0, MIN) != MAX;
    wrong += dh::sat_sub(-1, MIN) != MAX;
    wrong += dh::sat_sub(MIN, 1) != MIN;
    wrong += dh::sat_sub(MIN, MAX) != MIN;
    wrong += dh::sat_sub(-2, MAX) != MIN;
    wrong += dh::sat_sub(-1, MAX) != MIN;  // exactly representable
    wrong += dh::sat_sub(MIN, MIN) != 0 || dh::sat_sub(MAX, MAX) != 0 || dh::sat_sub(5, 7) != -2;
    wrong += dh::expired(100, 90, 10) || !dh::expired(100, 89, 10);
    wrong += !dh::expired(0, MIN, MAX - 1) || dh::expired(0, MIN, MAX);  // saturated: MAX > MAX - 1 only
    wrong += dh::expired(-5, MAX, 0) || dh::expired(MIN, MAX, MIN);  // saturated at MIN: MIN > MIN is false
    {
        const int64_t mt[3] = {89, 90, MIN}, at[3] = {KRK_NO_TIME, 50, 99};
        uint64_t bits = ~0ull;
        dh::expiry_bits(mt, nullptr, 3, 100, 10, 0, &bits);
        wrong += bits != 0b101;
        dh::expiry_bits(nullptr, at, 3, 100, 10, 20, &bits);
        wrong += bits != 0b010;  // a missing access time never fires
        dh::expiry_bits(mt, at, 3, 100, 10, 20, &bits);
        wrong += bits != 0b111;
        dh::expiry_bits(nullptr, nullptr, 3, 100, 10, 20, &bits);
        wrong += bits != 0;
        cases += 4;
    }
    // listings: every byte value at position b & 63, 'g' at every position, two bad bytes, the
    // lengths, and random-case valid names at the word edges
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto valid_name = [&] {
        std::string s(64, '0');
        for (auto& ch : s) {
            const uint64_t r = rnd(x);
            ch = "0123456789abcdef0123456789ABCDEF"[r & 31];
        }
        return s;
    };
    std::vector<std::string> sweep;
    for (int b = 0; b < 256; ++b) {
        std::string s = valid_name();
        s[b & 63] = (char)b;
        sweep.push_back(s);
    }
    for (int p = 0; p < 64; ++p) {
        std::string s = valid_name();
        s[p] = 'g';
        sweep.push_back(s);
    }
    {
        std::string s = valid_name();
        s[40] = 'x', s[9] = '/';
        sweep.push_back(s);
        for (size_t len : {0, 1, 63, 65, 66, 128}) sweep.push_back(std::string(len, 'a'));
        s = valid_name().substr(0, 40);
        s[3] = 'z';
        sweep.push_back(s);
        sweep.push_back(std::string(64, 'g'));
    }
    for (uint64_t lead : {0, 1, 3, 7, 13}) wrong += check_listing(sweep, lead, cases);
    for (uint64_t n : {0, 1, 63, 64, 65, 127, 128, 129, 200}) {
        std::vector<std::string> list;
        for (uint64_t i = 0; i < n; ++i) list.push_back(i % 7 == 3 ? sweep[(i * 13) % sweep.size()] : valid_name());
        wrong += check_listing(list, n % 5, cases);
    }
    // a decreasing offset pair is a length error and reads nothing
    {
        const uint64_t off[3] = {64, 0, 64};
        uint8_t* text = (uint8_t*)malloc(64);
        memset(text, 'a', 64);
        uint8_t dig[64];
        uint32_t st[2];
        uint64_t valid = ~0ull;
        dh::parse_listing(text, off, 2, dig, st, &valid);
        wrong += st[0] != (KRK_DHEX_LEN | 0x3FFFFFFFu) || st[1] != 0 || valid != 2;
        for (int j = 0; j < 32; ++j) wrong += dig[j] != 0 || dig[32 + j] != 0xAA;
        free(text);
        ++cases;
    }
    printf("digest_hex_math: %d cases, %d mismatches\n", cases, wrong);
    return wrong != 0;
}
