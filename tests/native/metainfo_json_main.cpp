// metainfo_json_main.cpp -- the _torrentmeta JSON codec's arithmetic
// (kraken_amd/csrc/metainfo_json_math.hpp) as a stand-alone CPU program, meant for the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -o metainfo_json_san metainfo_json_main.cpp && ./metainfo_json_san
// (tests/test_metainfo_json_math_native.py does exactly that).  It links nothing of the library.
//  * the formatter against snprintf and the scanner against strtoull / strtoll restatements
//    written here, over every decimal width, the int64 edges and the sum-count edges;
//  * both kernels' unit logic run one lane after another -- the serialise units' byte counts,
//    their exclusive scan and each lane's offset; the parse units' comma counts, their scan and
//    mj::parse_lane for every byte -- against the one-shot host functions;
//  * every document and span sits at the END of a heap block of its exact size, so a read past it
//    (or before a span) is AddressSanitizer's finding.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../kraken_amd/csrc/metainfo_json_math.hpp"

namespace ih = krk::ih;
namespace mj = krk::mj;

static int g_bad = 0, g_checks = 0;
#define EXPECT(c)                                                  \
    do {                                                           \
        ++g_checks;                                                \
        if (!(c)) {                                                \
            ++g_bad;                                               \
            printf("MISMATCH %s:%d: %s\n", __FILE__, __LINE__, #c); \
        }                                                          \
    } while (0)

// ------------------------------------------------------------------ restatements
static std::string ref_doc(int64_t P, const std::vector<uint32_t>* sums, const std::string& name, int64_t L) {
    char b[64];
    std::string s = "{\"Info\":{\"PieceLength\":";
    snprintf(b, sizeof b, "%" PRId64, P);
    s += b;
    s += ",\"PieceSums\":";
    if (!sums) {
        s += "null";
    } else {
        s += "[";
        for (size_t i = 0; i < sums->size(); ++i) {
            snprintf(b, sizeof b, "%s%" PRIu32, i ? "," : "", (*sums)[i]);
            s += b;
        }
        s += "]";
    }
    s += ",\"Name\":\"" + name + "\",\"Length\":";
    snprintf(b, sizeof b, "%" PRId64, L);
    s += b;
    return s + "}}";
}

// A span by strtoull: U32(,U32)* or empty, nothing else.
static bool ref_body(const std::string& t, std::vector<uint32_t>* out) {
    out->clear();
    if (t.empty()) return true;
    size_t p = 0;
    for (;;) {
        size_t q = p;
        while (q < t.size() && t[q] >= '0' && t[q] <= '9') ++q;
        if (q == p || q - p > 10 || (q - p > 1 && t[p] == '0')) return false;
        const unsigned long long v = strtoull(t.substr(p, q - p).c_str(), nullptr, 10);
        if (v > 0xFFFFFFFFull) return false;
        out->push_back((uint32_t)v);
        if (q == t.size()) return true;
        if (t[q] != ',') return false;
        p = q + 1;
    }
}

// The bytes of s at the end of an exact-size heap block.
struct Exact {
    uint8_t* p;
    size_t n;
    explicit Exact(const std::string& s) : p((uint8_t*)malloc(s.size() ? s.size() : 1)), n(s.size()) {
        if (n) memcpy(p, s.data(), n);
    }
    ~Exact() { free(p); }
    const uint8_t* data() const { return n ? p : p + 1; }  // an empty span: one past the block
};

// ------------------------------------------------------------------ serialise, lane by lane
static std::string lanes_doc(int64_t P, const std::vector<uint32_t>* sums, const std::string& name, int64_t L) {
    const uint64_t n = sums ? sums->size() : 0, nu = mj::ser_units(n);
    // pass one: a unit's byte count; pass two: the exclusive scan
    std::vector<uint64_t> scan(nu + 1, 0);
    for (uint64_t u = 0; u < nu; ++u) {
        uint32_t bytes = 0;
        for (uint32_t k = 0; k < mj::kSerUnit / 64; ++k)
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint64_t i = u * mj::kSerUnit + k * 64 + lane;
                if (i < n) bytes += mj::sum_bytes((*sums)[i], i + 1 == n);
            }
        scan[u + 1] = scan[u] + bytes;
    }
    const uint64_t body = scan[nu];
    std::vector<uint8_t> out(mj::doc_bytes(P, L, body, !sums), 0xA5);
    EXPECT(out.size() <= mj::bound(n));
    std::vector<uint8_t> stored(out.size(), 0);
    auto put = [&](uint64_t at, uint8_t c) {
        EXPECT(at < out.size());
        if (at >= out.size()) return;
        EXPECT(!stored[at]);  // no byte is written twice
        stored[at] = 1;
        out[at] = c;
    };
    // pass three: 64 sums a step at the offsets a scan of the lanes' byte counts gives
    const uint64_t arr = mj::kHeadA + mj::i64_len(P) + mj::kHeadB + 1;
    for (uint64_t u = 0; u < nu; ++u) {
        uint64_t dst = arr + scan[u];
        for (uint32_t k = 0; k < mj::kSerUnit / 64 && u * mj::kSerUnit + k * 64 < n; ++k) {
            uint32_t off = 0;
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint64_t i = u * mj::kSerUnit + k * 64 + lane;
                if (i >= n) break;
                const uint32_t v = (*sums)[i], nd = ih::digits(v);
                mj::emit_sum(v, nd, i + 1 == n, dst + off, put);
                off += nd + (i + 1 != n);
            }
            dst += off;
        }
    }
    // pass four: the envelope
    uint64_t at = mj::emit_head(P, 0, put);
    if (!sums) {
        at += ih::emit_text("null", 4, at, put);
    } else {
        put(at++, '[');
        at += body;
        put(at++, ']');
    }
    at += mj::emit_tail(reinterpret_cast<const uint8_t*>(name.data()), L, at, put);
    EXPECT(at == out.size());
    for (uint8_t s : stored) EXPECT(s);  // every byte is written
    return std::string(out.begin(), out.end());
}

// ------------------------------------------------------------------ parse, lane by lane
// status and sums as the kernels leave them; sums beyond the ones stored stay 0xFFFFFFFF.
static uint32_t lanes_parse(const uint8_t* t, uint64_t len, uint64_t expect_n, std::vector<uint32_t>* sums) {
    const uint64_t nu = mj::parse_units(len);
    std::vector<uint64_t> scan(nu + 1, 0);
    for (uint64_t u = 0; u < nu; ++u) {
        uint32_t commas = 0;
        for (uint64_t p = u * mj::kParseUnit; p < (u + 1) * mj::kParseUnit && p < len; ++p) commas += t[p] == ',';
        scan[u + 1] = scan[u] + commas;
    }
    sums->assign(expect_n, 0xFFFFFFFFu);
    uint32_t st = 0;
    for (uint64_t u = 0; u < nu; ++u) {
        uint64_t rank = scan[u];
        for (uint64_t p = u * mj::kParseUnit; p < (u + 1) * mj::kParseUnit && p < len; ++p) {
            bool start = false;
            uint32_t v = 0;
            if (mj::parse_lane(t, len, p, &start, &v)) st |= mj::kStatusForm;
            if (start && rank < expect_n) (*sums)[rank] = v;
            rank += t[p] == ',';
        }
    }
    if (mj::numbers_in(scan[nu], len) != expect_n) st |= mj::kStatusCount;
    return st;
}

static void check_span(const std::string& text) {
    Exact e(text);
    std::vector<uint32_t> want, got;
    const bool ok = ref_body(text, &want);
    std::vector<uint32_t> one(text.size() / 2 + 1);
    uint64_t n = 0, err = 0;
    const bool host = mj::scan_body(e.data(), e.n, one.data(), one.size(), &n, &err);
    EXPECT(host == ok);
    if (ok) {
        one.resize(n);
        EXPECT(one == want);
    }
    // the lanes: status 0 exactly for a canonical span with the expected count
    for (int64_t d = -1; d <= 1; ++d) {
        const int64_t en = (int64_t)want.size() + d;
        if (en < 0) continue;
        const uint32_t st = lanes_parse(e.data(), e.n, (uint64_t)en, &got);
        EXPECT((st == 0) == (ok && d == 0));
        EXPECT(((st & mj::kStatusForm) != 0) == !ok);
        if (st == 0) EXPECT(got == want);
    }
}

static void check_doc(int64_t P, const std::vector<uint32_t>* sums, const std::string& name, int64_t L) {
    const std::string want = ref_doc(P, sums, name, L);
    EXPECT(lanes_doc(P, sums, name, L) == want);
    Exact e(want);
    mj::Envelope env;
    uint64_t err = 0;
    EXPECT(mj::scan_envelope(e.data(), e.n, &env, &err));
    EXPECT(env.piece_length == P && env.length == L && env.sums_null == (sums ? 0u : 1u));
    EXPECT(memcmp(env.name, name.data(), 64) == 0);
    const size_t a = want.find("\"PieceSums\":") + 12 + (sums ? 1 : 4);
    EXPECT(env.arr_begin == a && env.arr_end == (sums ? want.find(']') : a));
    check_span(want.substr(env.arr_begin, env.arr_end - env.arr_begin));
    // every truncation and every one-byte extension is refused or is another canonical document;
    // all of them are read inside their exact-size block
    for (size_t cut = 0; cut < want.size(); cut += (want.size() > 400 ? 37 : 1)) {
        Exact t(want.substr(0, cut));
        EXPECT(!mj::scan_envelope(t.data(), t.n, &env, &err));
        Exact h(want.substr(cut));
        if (cut) EXPECT(!mj::scan_envelope(h.data(), h.n, &env, &err));
    }
    Exact more(want + "}");
    EXPECT(!mj::scan_envelope(more.data(), more.n, &env, &err));
}

int main() {
    const std::string lower = "0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef";
    const std::string upper = "0123456789ABCDEF0123456789ABCDEF0123456789ABCDEF0123456789ABCDEF";
    // int64: 0, +-1, every digit count, the extremes -- formatter and scanner against snprintf / strtoll
    std::vector<int64_t> edges = {0, 1, -1, INT64_MAX, INT64_MIN};
    for (int64_t p = 1, k = 1; k <= 18; ++k) {
        p *= 10;  // 10^1 .. 10^18
        edges.push_back(p - 1);
        edges.push_back(p);
        edges.push_back(-p);
        edges.push_back(-(p - 1));
    }
    for (int64_t v : edges) {
        char want[32];
        const int n = snprintf(want, sizeof want, "%" PRId64, v);
        uint8_t got[32];
        const uint32_t m = ih::emit_i64(v, 0, [&](uint64_t at, uint8_t c) { got[at] = c; });
        EXPECT((int)m == n && (int)mj::i64_len(v) == n && memcmp(got, want, n) == 0);
        Exact e(std::string(want, n));
        uint64_t pos = 0;
        int64_t back = 0;
        EXPECT(mj::scan_i64(e.data(), e.n, &pos, &back) && pos == (uint64_t)n && back == strtoll(want, nullptr, 10));
    }
    for (const char* bad : {"", "-", "-0", "00", "01", "-01", "9223372036854775808", "-9223372036854775809",
                            "10000000000000000000", "99999999999999999999", "+1", " 1"}) {
        Exact e{std::string(bad)};
        uint64_t pos = 0;
        int64_t v = 0;
        EXPECT(!mj::scan_i64(e.data(), e.n, &pos, &v));
    }
    // uint32: every width's edges
    std::vector<uint32_t> ladder = {0, 1, 9, 0xFFFFFFFFu, 0xFFFFFFFEu};
    for (uint32_t p = 1, k = 1; k <= 9; ++k) {
        p *= 10;
        ladder.push_back(p - 1);
        ladder.push_back(p);
    }
    for (uint32_t v : ladder) {
        char want[16];
        const int n = snprintf(want, sizeof want, "%" PRIu32, v);
        EXPECT((int)ih::digits(v) == n && (int)mj::sum_bytes(v, true) == n && (int)mj::sum_bytes(v, false) == n + 1);
    }
    // documents: the sum-count edges crossed with the value kinds, headers walking the edges
    const uint32_t U = mj::kSerUnit;
    uint64_t lcg = 20261020;
    auto rnd = [&] {
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(lcg >> 32) >> ((lcg >> 27) & 31);  // every width is likely
    };
    size_t k = 0;
    check_doc(4, nullptr, lower, 0);
    for (size_t n : {(size_t)0, (size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)U - 1, (size_t)U, (size_t)U + 1,
                     (size_t)2 * U + 1})
        for (int kind = 0; kind < 4; ++kind) {
            std::vector<uint32_t> s(n);
            for (size_t i = 0; i < n; ++i)
                s[i] = kind == 0 ? (uint32_t)(i % 10) : kind == 1 ? 0xFFFFFFFFu : kind == 2 ? ladder[i % ladder.size()] : rnd();
            check_doc(edges[k % edges.size()], &s, k & 1 ? upper : lower, edges[(7 * k + 3) % edges.size()]);
            ++k;
        }
    for (size_t i = 0; i < edges.size(); ++i) {
        std::vector<uint32_t> s = {rnd(), rnd(), rnd()};
        check_doc(edges[i], i % 3 ? &s : nullptr, lower, edges[edges.size() - 1 - i]);
    }
    // spans: the refusals, and a ten-digit number at every phase across a parse-unit edge
    for (const char* t : {"0", "00", "01", "1,02", "4294967295", "4294967296", "10000000000", "99999999999", ",", ",,",
                          "1,,2", ",1", "1,", "1 ,2", " 1", "1 ", "-1", "1.0", "1e3", "1,2,3", "0,0,0", "1]", "[1",
                          "12345678901234567890123"})
        check_span(t);
    for (uint32_t ph = 0; ph <= 12; ++ph) {
        std::string t;
        while (t.size() + 2 <= mj::kParseUnit - ph) t += "7,";
        if (t.size() < mj::kParseUnit - ph) t += "8";  // an odd phase: one two-digit number, "7,87,..."
        if (t.back() != ',') t += ",";
        const size_t at = t.size();
        t += "4294967295,12,0";
        // the number starts at the edge, straddles it at some phase, or its comma ends on it
        EXPECT(at + 12 >= mj::kParseUnit && at <= mj::kParseUnit);
        check_span(t);
        check_span(t.substr(0, at + 10));       // ends with the number
        check_span(t.substr(0, at + 9) + "6");  // 4294967296 across the edge
        check_span(t.substr(0, at) + "04294967295");
    }
    printf("metainfo_json_math: %d checks, %d mismatches\n", g_checks, g_bad);
    return g_bad ? 1 : 0;
}
