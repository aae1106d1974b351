// digest_hex.cpp -- cleanup plans from a raw cache listing: the SHA-256 hex codec
// (core.NewSHA256DigestFromHex / ValidateSHA256 / Digest.Hex(), core/digest.go:57-68,143-161), the
// expiry bits of maybeDelete (origin/blobserver/server.go:686-759) and of readyForDeletion
// (lib/store/cleanup.go:112-155), and `expired || !owns` over the names and mtimes themselves.
// The host forms (krk_digest_parse_hex, krk_digest_format_hex, krk_expiry_bits, krk_cleanup_plan:
// digest_hex_math.hpp on the calling thread, no device) and the device forms (digest_hex.hip
// computing the same bytes, bits, count and index list).
#include "digest_hex_math.hpp"
#include "ring_select_math.hpp"
#include "runtime.hpp"

using namespace krk;

extern "C" {

int krk_digest_parse_hex(const uint8_t* names, const uint64_t* off, uint64_t n, uint8_t* digests32_out,
                         uint32_t* status_out, uint64_t* valid_out) {
    KRK_CHECK(!n || (names && off && digests32_out), KRK_EINVAL, "digest_parse_hex: null argument");
    dh::parse_listing(names, off, n, digests32_out, status_out, valid_out);
    return KRK_OK;
}

int krk_digest_format_hex(const uint8_t* digests32, uint64_t n, uint8_t* hex_out) {
    KRK_CHECK(!n || (digests32 && hex_out), KRK_EINVAL, "digest_format_hex: null argument");
    dh::format_listing(digests32, n, hex_out);
    return KRK_OK;
}

int krk_expiry_bits(const int64_t* mtime_ns, const int64_t* atime_ns, uint64_t n, int64_t now_ns, int64_t ttl_ns,
                    int64_t tti_ns, uint64_t* bits_out) {
    KRK_CHECK(!n || bits_out, KRK_EINVAL, "expiry_bits: null argument");
    dh::expiry_bits(mtime_ns, atime_ns, n, now_ns, ttl_ns, tti_ns, bits_out);
    return KRK_OK;
}

int krk_cleanup_plan(const uint8_t* names, const uint64_t* off, uint64_t n, const int64_t* mtime_ns, int64_t now_ns,
                     int64_t ttl_ns, const uint64_t* mask, int invert, uint64_t* bits_out, uint64_t* valid_out,
                     uint64_t* idx_out, uint64_t idx_cap, uint64_t* count_out) {
    KRK_CHECK(mask && count_out && (!n || (names && off && bits_out)), KRK_EINVAL, "cleanup_plan: null argument");
    KRK_CHECK(idx_out || !idx_cap, KRK_EINVAL, "cleanup_plan: idx_out is NULL with idx_cap %llu",
              (unsigned long long)idx_cap);
    *count_out = dh::cleanup_plan(names, off, n, mtime_ns, now_ns, ttl_ns, mask, invert != 0, bits_out, valid_out,
                                  idx_out, idx_cap);
    return KRK_OK;
}

int krk_digest_parse_hex_dev(const uint8_t* names_dev, const uint64_t* off_dev, uint64_t n, uint8_t* digests32_dev,
                             uint32_t* status_dev, uint64_t* valid_dev, void* stream) {
    KRK_CHECK(!n || (names_dev && off_dev && digests32_dev), KRK_EINVAL, "digest_parse_hex_dev: null argument");
    KRK_CHECK(n / kDhexW < 0x7FFFFFFFull, KRK_ERANGE, "digest_parse_hex_dev: %llu names in one call",
              (unsigned long long)n);
    KRK_DEVICE(D);
    if (!n) return KRK_OK;
    KRK_CHECK(!((uintptr_t)off_dev & 7) && !((uintptr_t)valid_dev & 7) && !((uintptr_t)status_dev & 3), KRK_EINVAL,
              "digest_parse_hex_dev: off_dev and valid_dev must be 8-byte aligned, status_dev 4-byte aligned");
    KRK_CHECK(device_writable(names_dev, 1) && device_writable(off_dev, 8 * (n + 1)) &&
                  device_writable(digests32_dev, 32 * n) && (!status_dev || device_writable(status_dev, 4 * n)) &&
                  (!valid_dev || device_writable(valid_dev, 8 * dh::words(n))),
              KRK_EINVAL,
              "digest_parse_hex_dev: names, off, digests, status and valid must be device memory or page-locked "
              "host memory");
    hipStream_t s = pick(D, stream);
    const hipError_t e = timed(K_DHEXPARSE, s, [&] {
        return launch_digest_parse_hex(names_dev, off_dev, n, digests32_dev, status_dev, valid_dev, s);
    });
    KRK_CHECK(e == hipSuccess, KRK_EHIP, "digest_parse_hex launch: %s", launch_error_text(e));
    return KRK_OK;
}

int krk_digest_format_hex_dev(const uint8_t* digests32_dev, uint64_t n, uint8_t* hex_dev, void* stream) {
    KRK_CHECK(!n || (digests32_dev && hex_dev), KRK_EINVAL, "digest_format_hex_dev: null argument");
    KRK_CHECK(n / kDhexW < 0x7FFFFFFFull, KRK_ERANGE, "digest_format_hex_dev: %llu digests in one call",
              (unsigned long long)n);
    KRK_DEVICE(D);
    if (!n) return KRK_OK;
    KRK_CHECK(device_writable(digests32_dev, 32 * n) && device_writable(hex_dev, 64 * n), KRK_EINVAL,
              "digest_format_hex_dev: digests and hex must be device memory or page-locked host memory");
    hipStream_t s = pick(D, stream);
    const hipError_t e =
        timed(K_DHEXFMT, s, [&] { return launch_digest_format_hex(digests32_dev, n, hex_dev, s); });
    KRK_CHECK(e == hipSuccess, KRK_EHIP, "digest_format_hex launch: %s", launch_error_text(e));
    return KRK_OK;
}

int krk_cleanup_plan_dev(const uint8_t* names_dev, const uint64_t* off_dev, uint64_t n, const int64_t* mtime_ns_dev,
                         int64_t now_ns, int64_t ttl_ns, const uint64_t* mask_host, int invert, uint64_t* bits_out,
                         uint64_t* valid_out, uint64_t* idx_out, uint64_t idx_cap, uint64_t* count_out, void* stream) {
    KRK_CHECK(mask_host && count_out && (!n || (names_dev && off_dev && bits_out)), KRK_EINVAL,
              "cleanup_plan_dev: null argument");
    KRK_CHECK(idx_out || !idx_cap, KRK_EINVAL, "cleanup_plan_dev: idx_out is NULL with idx_cap %llu",
              (unsigned long long)idx_cap);
    KRK_CHECK(ring_select_workgroups(n) <= 0x7FFFFFFFull, KRK_ERANGE, "cleanup_plan_dev: %llu names in one call",
              (unsigned long long)n);
    KRK_DEVICE(D);
    const uint64_t words = dh::words(n);
    KRK_CHECK(!((uintptr_t)bits_out & 7) && !((uintptr_t)valid_out & 7) && !((uintptr_t)idx_out & 7) &&
                  !((uintptr_t)count_out & 7) && !((uintptr_t)off_dev & 7) && !((uintptr_t)mtime_ns_dev & 7),
              KRK_EINVAL,
              "cleanup_plan_dev: off_dev, mtime_ns_dev, bits_out, valid_out, idx_out and count_out must be 8-byte "
              "aligned");
    KRK_CHECK(device_writable(count_out, 8) &&
                  (!n || (device_writable(names_dev, 1) && device_writable(off_dev, 8 * (n + 1)) &&
                          device_writable(bits_out, 8 * words) &&
                          (!mtime_ns_dev || device_writable(mtime_ns_dev, 8 * n)) &&
                          (!valid_out || device_writable(valid_out, 8 * words)))) &&
                  (!idx_cap || device_writable(idx_out, 8 * idx_cap)),
              KRK_EINVAL,
              "cleanup_plan_dev: names, off, mtime, bits_out, valid_out, idx_out and count_out must be device memory "
              "or page-locked host memory");
    hipStream_t s = pick(D, stream);
    void* d_mask = nullptr;  // copied into the library's pinned staging before this returns
    int r = upload(D, mask_host, rs::kMaskWords * 8, &d_mask, s);
    if (r) return r;
    void* d_scratch = nullptr;
    if (scratch_alloc(D, &d_scratch, ring_select_scratch_bytes(n), s) != hipSuccess) {
        scratch_free(D, d_mask, s);
        set_error(KRK_ENOMEM, "cleanup_plan_dev: scan scratch");
        return KRK_ENOMEM;
    }
    const hipError_t e = timed(K_CLEANPLAN, s, [&] {
        return launch_cleanup_plan(names_dev, off_dev, n, mtime_ns_dev, now_ns, ttl_ns,
                                   static_cast<const uint32_t*>(d_mask), invert, bits_out, valid_out, idx_out, idx_cap,
                                   count_out, d_scratch, s);
    });
    scratch_free(D, d_scratch, s);
    scratch_free(D, d_mask, s);
    KRK_CHECK(e == hipSuccess, KRK_EHIP, "cleanup_plan launch: %s", launch_error_text(e));
    return KRK_OK;
}

int krk_digest_hex_geometry(uint64_t* names_per_workgroup) {
    KRK_CHECK(names_per_workgroup, KRK_EINVAL, "digest_hex_geometry: null argument");
    *names_per_workgroup = kDhexW;
    return KRK_OK;
}

}  // extern "C"
