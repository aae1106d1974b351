// repiece.cpp -- stored piece sums re-pieced to a coarser piece length without a blob byte
// read (the regeneration a changed piece-length table asks of every _torrentmeta, and of
// overwriteMetaInfo, origin/blobserver/server.go:344-360): the host forms (krk_repiece_sums,
// krk_repiece_batch, repiece_math.hpp on the calling thread) and the device-resident batch
// (krk_repiece_batch_dev, piece_repiece.hip running the same arithmetic).
#include "repiece_math.hpp"
#include "runtime.hpp"

using namespace krk;

namespace {

// Every refusal of a batch, before anything is written or launched.
int validate_repiece(const krk_repiece_blob* blobs, uint64_t n) {
    KRK_CHECK(n == 0 || blobs, KRK_EINVAL, "blobs is NULL");
    for (uint64_t i = 0; i < n; ++i) {
        const krk_repiece_blob& b = blobs[i];
        KRK_CHECK(b.piece_length > 0 && b.new_piece_length > 0, KRK_EINVAL, "piece length must be positive");
        KRK_CHECK(b.new_piece_length % b.piece_length == 0, KRK_EINVAL,
                  "new piece length %lld is not a multiple of piece length %lld", (long long)b.new_piece_length,
                  (long long)b.piece_length);
        KRK_CHECK(b.length >= 0, KRK_EINVAL, "blob %llu: negative length", (unsigned long long)i);
    }
    return KRK_OK;
}

}  // namespace

extern "C" {

int krk_repiece_batch(const krk_repiece_blob* blobs, uint64_t n, const uint32_t* sums, uint32_t* out) {
    const int r = validate_repiece(blobs, n);
    if (r) return r;
    for (uint64_t i = 0; i < n; ++i)
        KRK_CHECK(blobs[i].length == 0 || (sums && out), KRK_EINVAL, "repiece_batch: null argument");
    const uint32_t* xp = x8().v;
    for (uint64_t i = 0; i < n; ++i) {
        const krk_repiece_blob& b = blobs[i];
        rp::repiece(sums + b.sums_offset, (uint64_t)b.length, (uint64_t)b.piece_length,
                    (uint64_t)(b.new_piece_length / b.piece_length), out + b.out_offset, xp);
    }
    return KRK_OK;
}

int krk_repiece_sums(const uint32_t* sums, uint64_t n_sums, int64_t length, int64_t piece_length,
                     int64_t new_piece_length, uint32_t* out, uint64_t n_out) {
    const krk_repiece_blob b{length, piece_length, new_piece_length, 0, 0};
    const int r = validate_repiece(&b, 1);
    if (r) return r;
    const uint64_t n_old = krk_num_pieces((uint64_t)length, piece_length);
    KRK_CHECK(n_sums == n_old, KRK_EINVAL, "%llu piece sums for %llu pieces", (unsigned long long)n_sums,
              (unsigned long long)n_old);
    const uint64_t n_new = krk_num_pieces((uint64_t)length, new_piece_length);
    KRK_CHECK(n_out >= n_new, KRK_ERANGE, "repiece_sums: room for %llu sums, %llu needed", (unsigned long long)n_out,
              (unsigned long long)n_new);
    return krk_repiece_batch(&b, 1, sums, out);
}

int krk_repiece_batch_dev(const krk_repiece_blob* blobs_host, uint64_t n, const uint32_t* sums_dev, uint32_t* out_dev,
                          void* stream) {
    if (!n) return KRK_OK;
    int r = validate_repiece(blobs_host, n);
    if (r) return r;
    KRK_DEVICE(D);
    // The descriptors, and the spans of sums_dev read and of out_dev written.
    std::vector<RepieceBlob> desc(n);
    uint64_t units = 0, rlo = UINT64_MAX, rhi = 0, wlo = UINT64_MAX, whi = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const krk_repiece_blob& b = blobs_host[i];
        const uint64_t k = (uint64_t)(b.new_piece_length / b.piece_length);
        const uint64_t n_old = rp::num_pieces((uint64_t)b.length, (uint64_t)b.piece_length);
        const uint64_t n_new = rp::num_pieces((uint64_t)b.length, (uint64_t)b.new_piece_length);
        desc[i] = RepieceBlob{n_old ? b.sums_offset : 0, n_old ? b.out_offset : 0, (uint64_t)b.length,
                              (uint64_t)b.piece_length, k, units};
        units += rp::units(n_new, k);
        if (!n_old) continue;
        KRK_CHECK(b.sums_offset < (1ull << 60) && b.out_offset < (1ull << 60) && n_old < (1ull << 60), KRK_EINVAL,
                  "repiece_batch_dev: sums range of blob %llu is out of range", (unsigned long long)i);
        rlo = std::min(rlo, b.sums_offset);
        rhi = std::max(rhi, b.sums_offset + n_old);
        wlo = std::min(wlo, b.out_offset);
        whi = std::max(whi, b.out_offset + n_new);
    }
    if (!units) return KRK_OK;
    KRK_CHECK(sums_dev && out_dev, KRK_EINVAL, "repiece_batch_dev: null argument");
    KRK_CHECK(device_writable(sums_dev + rlo, (rhi - rlo) * 4) && device_writable(out_dev + wlo, (whi - wlo) * 4),
              KRK_EINVAL, "repiece_batch_dev: sums and out must be device memory or page-locked host memory");
    hipStream_t s = pick(D, stream);
    void* d_desc = nullptr;  // copied into the library's pinned staging before this returns
    r = upload(D, desc.data(), n * sizeof(RepieceBlob), &d_desc, s);
    if (r) return r;
    const hipError_t e = timed(K_REPIECE, s, [&] {
        return launch_piece_repiece(static_cast<const RepieceBlob*>(d_desc), n, units, D->d_tabs + kTabX8Pow, sums_dev,
                                    out_dev, s);
    });
    scratch_free(D, d_desc, s);
    KRK_CHECK(e == hipSuccess, KRK_EHIP, "piece_repiece launch: %s", launch_error_text(e));
    return KRK_OK;
}

}  // extern "C"
