// metainfo_json.cpp -- the _torrentmeta sidecar's JSON (MetaInfo.Serialize / DeserializeMetaInfo,
// core/metainfo.go:125-155) on the calling thread, no device: the serialiser, the parser of the
// canonical form and the O(1) envelope reader the device parse starts from, all through
// metainfo_json_math.hpp (the arithmetic metainfo_json.hip runs as well).
#include "metainfo_json_math.hpp"
#include "runtime.hpp"

using namespace krk;

extern "C" {

uint64_t krk_metainfo_json_bound(uint64_t n_sums) { return mj::bound(n_sums); }

int krk_metainfo_serialize(int64_t piece_length, const uint32_t* sums, uint64_t n_sums, int sums_null,
                           const char* name, uint64_t name_len, int64_t length, uint8_t* out, uint64_t cap,
                           uint64_t* len) {
    KRK_CHECK(len && (!n_sums || sums) && (!name_len || name), KRK_EINVAL, "metainfo_serialize: null argument");
    KRK_CHECK(!(sums_null && n_sums), KRK_EINVAL, "metainfo_serialize: a null PieceSums with %llu sums",
              (unsigned long long)n_sums);
    KRK_CHECK(n_sums < (1ull << 59), KRK_EINVAL, "metainfo_serialize: sum count out of range");
    KRK_CHECK(mj::name_ok(reinterpret_cast<const uint8_t*>(name), name_len), KRK_EINVAL,
              "metainfo_serialize: name is not 64 hex digits");
    uint64_t body = 0;
    for (uint64_t i = 0; i < n_sums; ++i) body += mj::sum_bytes(sums[i], i + 1 == n_sums);
    const uint64_t need = mj::doc_bytes(piece_length, length, body, sums_null != 0);
    *len = need;
    KRK_CHECK(cap >= need, KRK_ERANGE, "metainfo_serialize: room for %llu bytes, %llu needed", (unsigned long long)cap,
              (unsigned long long)need);
    KRK_CHECK(out, KRK_EINVAL, "metainfo_serialize: null argument");
    auto put = [&](uint64_t at, uint8_t c) { out[at] = c; };
    uint64_t at = mj::emit_head(piece_length, 0, put);
    if (sums_null) {
        at += ih::emit_text("null", 4, at, put);
    } else {
        put(at++, (uint8_t)'[');
        for (uint64_t i = 0; i < n_sums; ++i) {
            const uint32_t nd = ih::digits(sums[i]);
            const bool last = i + 1 == n_sums;
            mj::emit_sum(sums[i], nd, last, at, put);
            at += nd + !last;
        }
        put(at++, (uint8_t)']');
    }
    at += mj::emit_tail(reinterpret_cast<const uint8_t*>(name), length, at, put);
    return KRK_OK;  // at == need
}

int krk_metainfo_json_envelope(const uint8_t* data, uint64_t len, int64_t* piece_length, uint64_t* arr_begin,
                               uint64_t* arr_end, int* sums_null, char name_out[64], int64_t* length) {
    KRK_CHECK((data || !len) && piece_length && arr_begin && arr_end && sums_null && name_out && length, KRK_EINVAL,
              "metainfo_json_envelope: null argument");
    mj::Envelope e;
    uint64_t at = 0;
    KRK_CHECK(mj::scan_envelope(data, len, &e, &at), KRK_EFORMAT,
              "metainfo json: not the canonical form at byte %llu of %llu", (unsigned long long)at,
              (unsigned long long)len);
    *piece_length = e.piece_length;
    *length = e.length;
    *arr_begin = e.arr_begin;
    *arr_end = e.arr_end;
    *sums_null = (int)e.sums_null;
    memcpy(name_out, e.name, mj::kNameLen);
    return KRK_OK;
}

int krk_metainfo_parse(const uint8_t* data, uint64_t len, int64_t* piece_length, uint32_t* sums_out,
                       uint64_t sums_cap, uint64_t* n_sums, int* sums_null, char name_out[64], int64_t* length) {
    KRK_CHECK(n_sums, KRK_EINVAL, "metainfo_parse: null argument");
    uint64_t a = 0, b = 0;
    const int r = krk_metainfo_json_envelope(data, len, piece_length, &a, &b, sums_null, name_out, length);
    if (r) return r;
    uint64_t n = 0, at = 0;
    KRK_CHECK(mj::scan_body(data + a, b - a, sums_out, sums_out ? sums_cap : 0, &n, &at), KRK_EFORMAT,
              "metainfo json: not the canonical form at byte %llu of %llu", (unsigned long long)(a + at),
              (unsigned long long)len);
    *n_sums = n;
    KRK_CHECK(n <= sums_cap, KRK_ERANGE, "metainfo_parse: room for %llu sums, %llu needed", (unsigned long long)sums_cap,
              (unsigned long long)n);
    return KRK_OK;
}

}  // extern "C"
