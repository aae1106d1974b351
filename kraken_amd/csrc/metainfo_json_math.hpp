// metainfo_json_math.hpp -- the arithmetic of the _torrentmeta JSON codec (MetaInfo.Serialize /
// DeserializeMetaInfo, core/metainfo.go:125-155), host and device: the document's fixed texts and
// sizes, the int64 formatter, the canonical-form scanner, and the per-lane steps of the two
// kernels of metainfo_json.hip.  The decimal digit ladder and the multiply-high digit emit are
// info_hash_math.hpp's.  The host ABI (metainfo_json.cpp) runs these one-shot, the kernels 64
// lanes at a time, tests/native/metainfo_json_main.cpp one lane after another on the CPU.
// Nothing here needs the HIP headers.
//
// The canonical form -- exactly what Go's json.Marshal(&metaInfoJSON{info}) emits:
//   {"Info":{"PieceLength":I64,"PieceSums":ARR,"Name":"H64","Length":I64}}
//   I64 = -?(0|[1-9][0-9]{0,18}) in int64 range, never "-0"
//   ARR = null | [] | [U32(,U32)*]      U32 = 0|[1-9][0-9]{0,9}, <= 4294967295
//   H64 = 64 hex digits, either case
// no whitespace, no trailing bytes.
#pragma once
#include <stdint.h>

#include "info_hash_math.hpp"

#define KRK_MJ_HD KRK_IH_HD

namespace krk {
namespace mj {

constexpr uint32_t kSerUnit = 256;     // sums of ONE blob a serialise unit (one wave) formats
constexpr uint32_t kParseUnit = 1024;  // span bytes of ONE blob a parse unit (one wave) reads
constexpr uint32_t kMaxSumBytes = 11;  // ten digits and a comma
constexpr uint32_t kNameLen = 64;

// The fixed texts, in document order.
constexpr uint32_t kHeadA = 23, kHeadB = 13, kTailA = 9, kTailB = 11, kTailC = 2;
KRK_MJ_HD const char* head_a() { return "{\"Info\":{\"PieceLength\":"; }
KRK_MJ_HD const char* head_b() { return ",\"PieceSums\":"; }
KRK_MJ_HD const char* tail_a() { return ",\"Name\":\""; }
KRK_MJ_HD const char* tail_b() { return "\",\"Length\":"; }
KRK_MJ_HD const char* tail_c() { return "}}"; }

// ------------------------------------------------------------------ sizes
KRK_MJ_HD uint32_t i64_len(int64_t v) {
    const uint64_t m = v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v;
    return (v < 0) + ih::digits(m);
}
// A sum's bytes inside the array: its digits, and the comma after every sum but the last.
KRK_MJ_HD uint32_t sum_bytes(uint32_t v, bool last) { return ih::digits(v) + (last ? 0u : 1u); }
// `null`, or the brackets around `body` bytes.
KRK_MJ_HD uint64_t array_bytes(uint64_t body, bool is_null) { return is_null ? 4 : 2 + body; }
KRK_MJ_HD uint64_t doc_bytes(int64_t piece_length, int64_t length, uint64_t body, bool is_null) {
    return kHeadA + i64_len(piece_length) + kHeadB + array_bytes(body, is_null) + kTailA + kNameLen + kTailB +
           i64_len(length) + kTailC;
}
// Upper bound from the sum count alone: two 20-byte integers, eleven bytes a sum.
KRK_MJ_HD uint64_t bound(uint64_t n_sums) {
    return kHeadA + 20 + kHeadB + 4 + kTailA + kNameLen + kTailB + 20 + kTailC + kMaxSumBytes * n_sums;
}

// ------------------------------------------------------------------ emit
// {"Info":{"PieceLength":<P>,"PieceSums":   Returns the bytes.
template <class Put>
KRK_MJ_HD uint32_t emit_head(int64_t piece_length, uint64_t at, Put&& put) {
    uint32_t n = ih::emit_text(head_a(), kHeadA, at, put);
    n += ih::emit_i64(piece_length, at + n, put);
    n += ih::emit_text(head_b(), kHeadB, at + n, put);
    return n;
}
// ,"Name":"<64 bytes>","Length":<L>}}   Returns the bytes.
template <class Put>
KRK_MJ_HD uint32_t emit_tail(const uint8_t* name, int64_t length, uint64_t at, Put&& put) {
    uint32_t n = ih::emit_text(tail_a(), kTailA, at, put);
    for (uint32_t k = 0; k < kNameLen; ++k) put(at + n + k, name[k]);
    n += kNameLen;
    n += ih::emit_text(tail_b(), kTailB, at + n, put);
    n += ih::emit_i64(length, at + n, put);
    n += ih::emit_text(tail_c(), kTailC, at + n, put);
    return n;
}
// One sum of the array at `at`: nd = digits(v) digits, then the comma unless it is the last.
template <class Put>
KRK_MJ_HD void emit_sum(uint32_t v, uint32_t nd, bool last, uint64_t at, Put&& put) {
    ih::emit(v, nd, at, put);
    if (!last) put(at + nd, (uint8_t)',');
}

// ------------------------------------------------------------------ character classes
KRK_MJ_HD bool is_digit(uint8_t c) { return (uint8_t)(c - '0') < 10; }
KRK_MJ_HD bool is_hex(uint8_t c) {
    return is_digit(c) || (uint8_t)((c | 0x20) - 'a') < 6;
}
KRK_MJ_HD bool name_ok(const uint8_t* name, uint64_t n) {
    if (n != kNameLen) return false;
    bool ok = true;
    for (uint32_t k = 0; k < kNameLen; ++k) ok = ok && is_hex(name[k]);
    return ok;
}

// ------------------------------------------------------------------ the scanner
// data[*pos, len) starts with the n bytes of s: advances *pos.
KRK_MJ_HD bool match(const uint8_t* data, uint64_t len, uint64_t* pos, const char* s, uint32_t n) {
    if (len - *pos < n) return false;  // *pos <= len
    for (uint32_t k = 0; k < n; ++k)
        if (data[*pos + k] != (uint8_t)s[k]) return false;
    *pos += n;
    return true;
}
// A canonical I64 at *pos, ending at the first byte that is no digit (or at len): advances *pos.
KRK_MJ_HD bool scan_i64(const uint8_t* data, uint64_t len, uint64_t* pos, int64_t* out) {
    uint64_t p = *pos;
    const bool neg = p < len && data[p] == '-';
    p += neg;
    if (p >= len || !is_digit(data[p])) return false;
    uint64_t m = 0;
    uint32_t nd = 0;
    while (p < len && is_digit(data[p])) {
        if (++nd > 19) return false;  // 19 digits stay below 2^64
        m = m * 10 + (uint64_t)(data[p] - '0');
        ++p;
    }
    if (nd > 1 && data[*pos + neg] == '0') return false;  // leading zero
    if (neg ? (m == 0 || m > (1ull << 63)) : m > (1ull << 63) - 1) return false;  // "-0", range
    *out = neg ? (int64_t)((uint64_t)0 - m) : (int64_t)m;
    *pos = p;
    return true;
}

// The envelope of a document: O(1) work, the span between the brackets is not looked at.
struct Envelope {
    int64_t piece_length, length;
    uint64_t arr_begin, arr_end;  // the bytes strictly between '[' and ']' (equal for [] and null)
    uint32_t sums_null;
    uint8_t name[kNameLen];
};
// True for a canonical envelope; else *err_at is the byte offset where the form breaks.
KRK_MJ_HD bool scan_envelope(const uint8_t* data, uint64_t len, Envelope* e, uint64_t* err_at) {
    uint64_t p = 0;
    *err_at = 0;
    if (!match(data, len, &p, head_a(), kHeadA)) return false;
    *err_at = p;
    if (!scan_i64(data, len, &p, &e->piece_length)) return false;
    *err_at = p;
    if (!match(data, len, &p, head_b(), kHeadB)) return false;
    *err_at = p;
    uint64_t q = p;
    e->sums_null = match(data, len, &q, "null", 4) ? 1u : 0u;
    if (!e->sums_null) {
        if (p >= len || data[p] != '[') return false;
        q = p + 1;
    }
    const uint64_t front = q;  // null: where the tail must start; else the span's first byte
    // From the back: }} , the Length's digits and sign, the fixed-size rest of the tail.
    *err_at = len;
    if (len - front < kTailC || data[len - 2] != '}' || data[len - 1] != '}') return false;
    uint64_t b = len - kTailC;  // one past the Length
    uint32_t nd = 0;
    while (b > front && nd < 19 && is_digit(data[b - 1])) {
        --b;
        ++nd;
    }
    if (b > front && data[b - 1] == '-') --b;
    *err_at = b;
    uint64_t t = b;
    if (!scan_i64(data, len - kTailC, &t, &e->length) || t != len - kTailC) return false;
    constexpr uint32_t fixed = kTailA + kNameLen + kTailB;
    const uint32_t close = e->sums_null ? 0u : 1u;  // the ']'
    if (b - front < fixed + close) {
        *err_at = front;
        return false;
    }
    uint64_t s = b - fixed;  // the tail's comma
    if (e->sums_null ? s != front : data[s - 1] != ']') {
        *err_at = e->sums_null ? front : s - 1;
        return false;
    }
    e->arr_begin = front;
    e->arr_end = e->sums_null ? front : s - 1;
    *err_at = s;
    if (!match(data, len, &s, tail_a(), kTailA)) return false;
    for (uint32_t k = 0; k < kNameLen; ++k) {
        *err_at = s + k;
        if (!is_hex(data[s + k])) return false;
        e->name[k] = data[s + k];
    }
    s += kNameLen;
    *err_at = s;
    return match(data, len, &s, tail_b(), kTailB);  // s == b now
}

// The span between the brackets, one shot: U32(,U32)* or empty.  The first min(count, cap) values
// go to out; *n_out is the count.  False with *err_at (relative to text) where the form breaks.
KRK_MJ_HD bool scan_body(const uint8_t* text, uint64_t len, uint32_t* out, uint64_t cap, uint64_t* n_out,
                         uint64_t* err_at) {
    uint64_t p = 0, n = 0;
    *n_out = 0;
    *err_at = 0;
    if (!len) return true;
    for (;;) {
        *err_at = p;
        if (p >= len || !is_digit(text[p])) return false;
        const uint64_t first = p;
        uint64_t v = 0;
        while (p < len && is_digit(text[p])) {
            if (p - first >= 10) return false;  // an eleventh digit
            v = v * 10 + (uint64_t)(text[p] - '0');
            ++p;
        }
        if ((p - first > 1 && text[first] == '0') || v > 0xFFFFFFFFull) return false;
        if (n < cap) out[n] = (uint32_t)v;
        ++n;
        if (p == len) break;
        *err_at = p;
        if (text[p] != ',') return false;
        ++p;
    }
    *n_out = n;
    return true;
}

// ------------------------------------------------------------------ the parse kernel's lane
// Span byte p (p < len), looked at by its own lane.  Returns true when the byte breaks the form:
// it is neither digit nor comma, a comma without a digit on both sides, or the first byte of a
// number (a digit at 0 or after a comma) that is not a canonical U32 followed by a comma or the
// span's end.  *is_start / *value: p starts a number and its value (valid when the lane is not
// bad).  The lane reads text[p - 1 .. p + 10] inside [0, len) only.
KRK_MJ_HD bool parse_lane(const uint8_t* text, uint64_t len, uint64_t p, bool* is_start, uint32_t* value) {
    *is_start = false;
    *value = 0;
    const uint8_t c = text[p];
    if (c == ',') return !(p > 0 && p + 1 < len && is_digit(text[p - 1]) && is_digit(text[p + 1]));
    if (!is_digit(c)) return true;
    if (p > 0 && text[p - 1] != ',') return false;  // inside a run (its start checks it), or after a bad byte
    *is_start = true;
    uint64_t v = 0;
    uint32_t nd = 0;
    for (; nd < 11 && p + nd < len && is_digit(text[p + nd]); ++nd) v = v * 10 + (uint64_t)(text[p + nd] - '0');
    *value = (uint32_t)v;
    // a terminator other than a comma is that byte's own finding
    return nd > 10 || (nd > 1 && c == '0') || v > 0xFFFFFFFFull;
}
// Commas count a number's rank: the number that starts at p is number (commas in [0, p)).
KRK_MJ_HD uint64_t numbers_in(uint64_t commas, uint64_t len) { return len ? commas + 1 : 0; }

constexpr uint32_t kStatusForm = 1;   // the span is not canonical
constexpr uint32_t kStatusCount = 2;  // it does not hold expect_n numbers

KRK_MJ_HD uint64_t ser_units(uint64_t n_sums) { return n_sums / kSerUnit + (n_sums % kSerUnit != 0); }
KRK_MJ_HD uint64_t parse_units(uint64_t text_len) { return text_len / kParseUnit + (text_len % kParseUnit != 0); }

}  // namespace mj
}  // namespace krk
