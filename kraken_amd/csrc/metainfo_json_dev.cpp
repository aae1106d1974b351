// metainfo_json_dev.cpp -- the C ABI's device _torrentmeta codec: krk_metainfo_serialize_batch_dev
// (sums in device memory -> whole documents) and krk_metainfo_parse_sums_batch_dev (the spans
// between the brackets -> sums), metainfo_json.hip behind both.  Every refusal comes before a
// launch; descriptors are staged before a call returns.
#include "metainfo_json_math.hpp"
#include "runtime.hpp"

using namespace krk;

extern "C" {

int krk_metainfo_serialize_batch_dev(const krk_metainfo_json_blob* blobs_host, uint64_t n, const uint32_t* sums_dev,
                                     uint8_t* out, uint64_t* out_len, void* stream) {
    if (!n) return KRK_OK;
    KRK_CHECK(blobs_host && out && out_len, KRK_EINVAL, "metainfo_serialize_batch_dev: null argument");
    KRK_CHECK(n < (1ull << 32), KRK_EINVAL, "more than 2^32 blobs in one call");
    std::vector<MjSerBlob> desc(n);
    uint64_t units = 0, rlo = UINT64_MAX, rhi = 0, wlo = UINT64_MAX, whi = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const krk_metainfo_json_blob& b = blobs_host[i];
        KRK_CHECK(mj::name_ok(reinterpret_cast<const uint8_t*>(b.name), mj::kNameLen), KRK_EINVAL,
                  "metainfo_serialize_batch_dev: name of blob %llu is not 64 hex digits", (unsigned long long)i);
        KRK_CHECK(!(b.sums_null && b.n_sums), KRK_EINVAL,
                  "metainfo_serialize_batch_dev: blob %llu has a null PieceSums with %llu sums", (unsigned long long)i,
                  (unsigned long long)b.n_sums);
        KRK_CHECK(b.sums_off < (1ull << 56) && b.n_sums < (1ull << 56) && b.out_off < (1ull << 60), KRK_EINVAL,
                  "metainfo_serialize_batch_dev: range of blob %llu is out of range", (unsigned long long)i);
        MjSerBlob& d = desc[i];
        d = MjSerBlob{};
        d.first_sum = b.n_sums ? b.sums_off : 0;
        d.n_sums = b.n_sums;
        d.out_off = b.out_off;
        d.first_unit = units;
        d.piece_length = b.piece_length;
        d.length = b.length;
        d.sums_null = b.sums_null ? 1u : 0u;
        memcpy(d.name, b.name, mj::kNameLen);
        units += mj::ser_units(b.n_sums);
        wlo = std::min(wlo, b.out_off);
        whi = std::max(whi, b.out_off + mj::bound(b.n_sums));
        if (!b.n_sums) continue;
        rlo = std::min(rlo, b.sums_off);
        rhi = std::max(rhi, b.sums_off + b.n_sums);
    }
    KRK_DEVICE(D);
    KRK_CHECK(rhi <= rlo || (sums_dev && device_writable(sums_dev + rlo, (rhi - rlo) * 4)), KRK_EINVAL,
              "metainfo_serialize_batch_dev: sums_dev must be device memory or page-locked host memory");
    KRK_CHECK(device_writable(out + wlo, whi - wlo) && device_writable(out_len, 8 * n), KRK_EINVAL,
              "metainfo_serialize_batch_dev: out and out_len must be device memory or page-locked host memory");
    KRK_CHECK(!(reinterpret_cast<uintptr_t>(out_len) & 7), KRK_EINVAL,
              "metainfo_serialize_batch_dev: out_len must be 8-byte aligned");
    hipStream_t s = pick(D, stream);
    void* d_desc = nullptr;
    int r = upload(D, desc.data(), n * sizeof(MjSerBlob), &d_desc, s);
    if (r) return r;
    void* d_scratch = nullptr;
    hipError_t e = scratch_alloc(D, &d_scratch, mj_ser_scratch_bytes(units), s);
    if (e == hipSuccess)
        e = timed(K_MJSER, s, [&] {
            return launch_metainfo_serialize(static_cast<const MjSerBlob*>(d_desc), n, units, sums_dev, out, out_len,
                                             d_scratch, s);
        });
    scratch_free(D, d_scratch, s);
    scratch_free(D, d_desc, s);
    KRK_CHECK(e == hipSuccess, KRK_EHIP, "metainfo_serialize launch: %s", launch_error_text(e));
    return KRK_OK;
}

int krk_metainfo_parse_sums_batch_dev(const krk_metainfo_json_span* spans_host, uint64_t n, const uint8_t* text_dev,
                                      uint32_t* sums_out, uint32_t* status, void* stream) {
    if (!n) return KRK_OK;
    KRK_CHECK(spans_host && status, KRK_EINVAL, "metainfo_parse_sums_batch_dev: null argument");
    KRK_CHECK(n < (1ull << 32), KRK_EINVAL, "more than 2^32 blobs in one call");
    std::vector<MjParseBlob> desc(n);
    uint64_t units = 0, rlo = UINT64_MAX, rhi = 0, wlo = UINT64_MAX, whi = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const krk_metainfo_json_span& b = spans_host[i];
        KRK_CHECK(b.text_off < (1ull << 60) && b.text_len < (1ull << 60) && b.sums_off < (1ull << 56) &&
                      b.expect_n < (1ull << 56),
                  KRK_EINVAL, "metainfo_parse_sums_batch_dev: range of blob %llu is out of range",
                  (unsigned long long)i);
        desc[i] = MjParseBlob{b.text_len ? b.text_off : 0, b.text_len, b.expect_n ? b.sums_off : 0, b.expect_n, units, 0};
        units += mj::parse_units(b.text_len);
        if (b.text_len) {
            rlo = std::min(rlo, b.text_off);
            rhi = std::max(rhi, b.text_off + b.text_len);
        }
        if (b.expect_n) {
            wlo = std::min(wlo, b.sums_off);
            whi = std::max(whi, b.sums_off + b.expect_n);
        }
    }
    KRK_DEVICE(D);
    KRK_CHECK(rhi <= rlo || (text_dev && device_writable(text_dev + rlo, rhi - rlo)), KRK_EINVAL,
              "metainfo_parse_sums_batch_dev: text_dev must be device memory or page-locked host memory");
    KRK_CHECK((whi <= wlo || (sums_out && device_writable(sums_out + wlo, (whi - wlo) * 4))) &&
                  device_writable(status, 4 * n),
              KRK_EINVAL,
              "metainfo_parse_sums_batch_dev: sums_out and status must be device memory or page-locked host memory");
    hipStream_t s = pick(D, stream);
    void* d_desc = nullptr;
    int r = upload(D, desc.data(), n * sizeof(MjParseBlob), &d_desc, s);
    if (r) return r;
    void* d_scratch = nullptr;
    hipError_t e = scratch_alloc(D, &d_scratch, mj_parse_scratch_bytes(units), s);
    if (e == hipSuccess)
        e = timed(K_MJPARSE, s, [&] {
            return launch_metainfo_parse_sums(static_cast<const MjParseBlob*>(d_desc), n, units, text_dev, sums_out,
                                              status, d_scratch, s);
        });
    scratch_free(D, d_scratch, s);
    scratch_free(D, d_desc, s);
    KRK_CHECK(e == hipSuccess, KRK_EHIP, "metainfo_parse_sums launch: %s", launch_error_text(e));
    return KRK_OK;
}

int krk_metainfo_json_geometry(uint64_t* serialize_unit_sums, uint64_t* parse_unit_bytes) {
    KRK_CHECK(serialize_unit_sums && parse_unit_bytes, KRK_EINVAL, "metainfo_json_geometry: null argument");
    *serialize_unit_sums = mj::kSerUnit;
    *parse_unit_bytes = mj::kParseUnit;
    return KRK_OK;
}

int krk_metainfo_json_scan_geometry(uint64_t* counts_per_pass, uint64_t* max_workgroups) {
    KRK_CHECK(counts_per_pass && max_workgroups, KRK_EINVAL, "metainfo_json_scan_geometry: null argument");
    *counts_per_pass = (uint64_t)mj::kScanBlock * mj::kScanPer;
    *max_workgroups = mj::kMaxBlocks;
    return KRK_OK;
}

}  // extern "C"
