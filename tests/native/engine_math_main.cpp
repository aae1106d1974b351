// The submission engine's piece arithmetic (kraken_amd/csrc/engine_math.hpp: what launch_crc
// of engine.cpp and stream_fold of piece_stream.cpp run) as a stand-alone program:
//  1. portions() over an exhaustive small space against a walk over the bytes;
//  2. fold() over real bytes cut into requests at every structural position, every portion's CRC
//     from an in-program bitwise CRC-32, every piece sum against the bitwise CRC of the piece;
//  3. 64-bit offsets and piece lengths over streams of zeros, whose CRC has a closed form
//     (crc_math.hpp: crc(n zero bytes) = shift(~0, n) ^ ~0), so no byte is touched.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <utility>
#include <vector>

#include "../../kraken_amd/csrc/engine_math.hpp"

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
static int g_cases = 0;

typedef std::vector<std::pair<uint64_t, uint64_t>> Segs;

// The portions of p as [start, end) pairs, in stream order.
static Segs expand(const em::Portions& p, uint64_t a, uint64_t len, uint64_t P) {
    Segs out;
    const uint64_t b = a + len;
    if (p.head) out.push_back({a, p.first_end});
    for (uint64_t i = p.f0; i < p.f1; ++i) out.push_back({i * P, (i + 1) * P});
    if (p.tail) out.push_back({a > p.f1 * P ? a : p.f1 * P, b});
    return out;
}

// 1. every P in 1..20, a in 0..3P, len in 0..3P+2, byte by byte.
static int check_portions_small() {
    int wrong = 0;
    for (uint64_t P = 1; P <= 20; ++P)
        for (uint64_t a = 0; a <= 3 * P; ++a)
            for (uint64_t len = 0; len <= 3 * P + 2; ++len) {
                Segs want;  // a new segment at a and at every multiple of P
                for (uint64_t x = a; x < a + len; ++x) {
                    if (x == a || x % P == 0) want.push_back({x, x});
                    want.back().second = x + 1;
                }
                bool head = false, tail = false;
                uint64_t whole = 0, first_whole = 0;
                for (const auto& s : want) {
                    if (s.first % P) head = true;
                    else if (s.second - s.first < P) tail = true;
                    else if (!whole++) first_whole = s.first / P;
                }
                const em::Portions p = em::portions(a, len, P);
                bool bad = p.count != want.size() || p.head != head || p.tail != tail || p.f1 - p.f0 != whole ||
                           (whole && p.f0 != first_whole) || expand(p, a, len, P) != want;
                if (p.head) bad |= p.first_end != want[0].second;
                wrong += bad;
                ++g_cases;
                // P == 0: the request is one portion
                const em::Portions z = em::portions(a, len, 0);
                wrong += len ? !(z.count == 1 && z.head && !z.tail && z.first_end == a + len && z.f0 == z.f1)
                             : z.count != 0;
            }
    return wrong;
}

static uint64_t g_seen[4];  // requests that: start a piece, end a piece, touch neither inside one, span >= 3 pieces

// 2. `data` cut into requests of R bytes (the last one shorter), pieces of P bytes.
static int check_fold_bytes(const std::vector<uint8_t>& data, uint64_t P, uint64_t R, uint64_t first) {
    const uint64_t L = data.size();
    std::vector<uint32_t> sums;
    int wrong = 0;
    uint32_t reg = 0xFFFFFFFFu;
    for (uint64_t off = 0; off < L;) {
        const uint64_t len = off == 0 && first ? (first < L ? first : L) : (R < L - off ? R : L - off);
        const em::Portions p = em::portions(off, len, P);
        std::vector<uint32_t> crcs;
        for (const auto& s : expand(p, off, len, P)) crcs.push_back(crc_bytes(data.data() + s.first, s.second - s.first));
        wrong += crcs.size() != p.count;
        wrong += !em::fold(sums, off, len, P, crcs.data(), crcs.size(), g_tab.v);
        g_seen[0] += off % P == 0;
        g_seen[1] += (off + len) % P == 0;
        g_seen[2] += off % P && (off + len) % P && off / P == (off + len) / P;
        g_seen[3] += (off + len - 1) / P - off / P >= 2;
        // the piece being filled holds the CRC of its bytes so far (reg: its bitwise register)
        for (uint64_t x = off; x < off + len; ++x) {
            if (x % P == 0) reg = 0xFFFFFFFFu;
            reg ^= data[x];
            for (int b = 0; b < 8; ++b) reg = (reg >> 1) ^ (kCrcPoly & (0u - (reg & 1u)));
        }
        off += len;
        const uint64_t np = (off + P - 1) / P;
        wrong += sums.size() != np;
        if (sums.size() == np && np) wrong += sums[np - 1] != ~reg;
    }
    const uint64_t np = (L + P - 1) / P;
    wrong += sums.size() != np;
    for (uint64_t i = 0; i < np && i < sums.size(); ++i)
        wrong += sums[i] != crc_bytes(data.data() + i * P, (L - i * P < P ? L - i * P : P));
    ++g_cases;
    return wrong;
}

static int check_broken_order() {
    int wrong = 0;
    const uint32_t c[3] = {1, 2, 3};
    std::vector<uint32_t> sums;
    wrong += em::fold(sums, 5, 3, 10, c, 1, g_tab.v) || !sums.empty();  // inside piece 0, nothing begun
    sums.assign(1, 7);
    wrong += em::fold(sums, 25, 3, 10, c, 1, g_tab.v) || sums.size() != 1 || sums[0] != 7;  // piece 2, only 0 begun
    // the portions before the broken one stay folded: piece 1 begun by this request, then a gap is
    // impossible inside one request, so a request whose first portion continues piece 1 of a
    // stream that holds piece 0 alone is the whole of it
    wrong += em::fold(sums, 15, 10, 10, c, 2, g_tab.v);
    sums.assign(2, 9);
    wrong += !em::fold(sums, 15, 10, 10, c, 2, g_tab.v) || sums.size() != 3 || sums[2] != 2;  // in order: folds
    g_cases += 4;
    return wrong;
}

// crc of n zero bytes, closed form
static uint32_t crc0(uint64_t n) { return gf2_mulmod(0xFFFFFFFFu, x8n(n, g_tab.v)) ^ 0xFFFFFFFFu; }

// 3. a stream of zeros, pieces of P bytes: requests [off, off + len) for the listed lengths from
// `start`, the piece `start` lies in begun by earlier requests (its sum preset to the closed form).
static int check_far(uint64_t P, uint64_t start, const std::vector<uint64_t>& lens) {
    int wrong = 0;
    std::vector<uint32_t> sums;
    const uint64_t p0 = start / P;
    if (start % P) {
        sums.assign(p0 + 1, 0xDEADBEEFu);
        sums[p0] = crc0(start - p0 * P);
    } else {
        sums.assign(p0, 0xDEADBEEFu);
    }
    uint64_t off = start;
    for (uint64_t len : lens) {
        const em::Portions p = em::portions(off, len, P);
        const Segs segs = expand(p, off, len, P);
        wrong += segs.size() != p.count;
        uint64_t at = off;  // the portions tile the request at the multiples of P
        std::vector<uint32_t> crcs;
        for (const auto& s : segs) {
            wrong += s.first != at || s.second <= s.first || (s.first / P != (s.second - 1) / P);
            at = s.second;
            crcs.push_back(crc0(s.second - s.first));
        }
        wrong += at != off + len;
        wrong += !em::fold(sums, off, len, P, crcs.data(), crcs.size(), g_tab.v);
        off += len;
        const uint64_t np = (off + P - 1) / P;
        wrong += sums.size() != np;
        for (uint64_t i = p0; i < np && i < sums.size(); ++i)
            wrong += sums[i] != crc0(off - i * P < P ? off - i * P : P);
    }
    for (uint64_t i = 0; i < p0 && i < sums.size(); ++i) wrong += sums[i] != 0xDEADBEEFu;  // earlier pieces untouched
    ++g_cases;
    return wrong;
}

int main() {
    g_tab = make_x8pow();
    int mismatches = 0;
    mismatches += check_portions_small();

    std::vector<uint8_t> data(5003);
    for (auto& b : data) b = (uint8_t)rnd();
    for (uint64_t P : {1, 2, 7, 64, 100, 999, 1000, 2501, 5002, 5003, 5004, 9000})
        for (uint64_t R : {(uint64_t)1, (uint64_t)3, P > 1 ? P - 1 : 1, P, P + 1, 2 * P + 3, 3 * P, (uint64_t)333, (uint64_t)5003})
            for (uint64_t first : {(uint64_t)0, P / 2 + 1}) mismatches += check_fold_bytes(data, P, R, first);
    for (int k = 0; k < 4; ++k) mismatches += g_seen[k] == 0;  // every structural position was cut
    mismatches += check_broken_order();

    // the closed form itself, against the bitwise CRC
    {
        std::vector<uint8_t> z(300, 0);
        for (uint64_t n = 0; n <= 300; ++n) mismatches += crc0(n) != crc_bytes(z.data(), n);
        ++g_cases;
    }
    const uint64_t S = 524288;
    for (uint64_t P : {(1ull << 31) - 1, (1ull << 31) + 1, (1ull << 33) + 5})
        for (uint64_t beyond : {1ull << 32, (1ull << 32) + 12345, 1ull << 40, (1ull << 40) + (1ull << 32) + 7}) {
            const uint64_t E = (beyond + P - 1) / P * P;  // the first piece end at or beyond it
            // requests of S bytes at multiples of S (what the engine submits) straddling E
            mismatches += check_far(P, (E - 2 * S) / S * S, {S, S, S, S, S});
            // a request that ends exactly on E, one that starts exactly on it
            mismatches += check_far(P, E - S, {S, S});
            // one byte either side
            mismatches += check_far(P, E - S - 1, {S, S});
            mismatches += check_far(P, E - S + 1, {S, S});
            // a request over several pieces from the middle of one
            mismatches += check_far(P, E - 777, {3 * P + 12345, 1, P - 1});
        }
    printf("engine_math: %d cases, %d mismatches\n", g_cases, mismatches);
    return mismatches != 0;
}
