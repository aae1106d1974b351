// ring_select_abi.cpp -- ring ownership and membership-change selection as bitsets: which of these
// blobs belong on this origin, and which change hands when the ring changes (maybeDelete's
// `owns`, origin/blobserver/server.go:686-759; applyToReplicas' replica set, 426-454).  The
// shard masks and the host selection (krk_ring_mask_owns, krk_ring_mask_moved, krk_ring_select:
// ring_select_math.hpp on the calling thread, no device) and the device-resident selection
// (krk_ring_select_dev, ring_select.hip computing the same bits, count and index list).
#include "ring_select_math.hpp"
#include "runtime.hpp"

using namespace krk;

extern "C" {

int krk_ring_mask_owns(const int32_t* locs, const uint8_t* counts, uint32_t row, int32_t node, uint64_t* mask_out) {
    KRK_CHECK(locs && counts && mask_out, KRK_EINVAL, "ring_mask_owns: null argument");
    KRK_CHECK(row > 0, KRK_EINVAL, "ring_mask_owns: row is 0");
    KRK_CHECK(rs::mask_owns(locs, counts, row, node, mask_out), KRK_EINVAL,
              "ring_mask_owns: a shard has more owners than the row holds");
    return KRK_OK;
}

int krk_ring_mask_moved(const int32_t* locs_a, const uint8_t* counts_a, uint32_t row_a, const int32_t* locs_b,
                        const uint8_t* counts_b, uint32_t row_b, const int32_t* b_to_a, uint32_t n_nodes_b,
                        uint64_t* mask_out) {
    KRK_CHECK(locs_a && counts_a && locs_b && counts_b && mask_out, KRK_EINVAL, "ring_mask_moved: null argument");
    KRK_CHECK(row_a > 0 && row_b > 0, KRK_EINVAL, "ring_mask_moved: row is 0");
    KRK_CHECK(rs::mask_moved(locs_a, counts_a, row_a, locs_b, counts_b, row_b, b_to_a, n_nodes_b, mask_out), KRK_EINVAL,
              "ring_mask_moved: an owner of membership B is outside [0, %u), or a shard has more owners than its row holds",
              n_nodes_b);
    return KRK_OK;
}

int krk_ring_select(const uint8_t* digests32, uint64_t n, const uint64_t* mask, int invert, const uint64_t* or_bits,
                    uint64_t* bits_out, uint64_t* idx_out, uint64_t idx_cap, uint64_t* count_out) {
    KRK_CHECK(mask && count_out && (!n || (digests32 && bits_out)), KRK_EINVAL, "ring_select: null argument");
    KRK_CHECK(idx_out || !idx_cap, KRK_EINVAL, "ring_select: idx_out is NULL with idx_cap %llu",
              (unsigned long long)idx_cap);
    *count_out = rs::select(digests32, n, mask, invert != 0, or_bits, bits_out, idx_out, idx_cap);
    return KRK_OK;
}

int krk_ring_select_dev(const uint8_t* digests32_dev, uint64_t n, const uint64_t* mask_host, int invert,
                        const uint64_t* or_bits_dev, uint64_t* bits_out, uint64_t* idx_out, uint64_t idx_cap,
                        uint64_t* count_out, void* stream) {
    KRK_CHECK(mask_host && count_out && (!n || (digests32_dev && bits_out)), KRK_EINVAL,
              "ring_select_dev: null argument");
    KRK_CHECK(idx_out || !idx_cap, KRK_EINVAL, "ring_select_dev: idx_out is NULL with idx_cap %llu",
              (unsigned long long)idx_cap);
    KRK_CHECK(ring_select_workgroups(n) <= 0x7FFFFFFFull, KRK_ERANGE, "ring_select_dev: %llu digests in one call",
              (unsigned long long)n);
    KRK_DEVICE(D);
    const uint64_t words = rs::words(n);
    KRK_CHECK(!((uintptr_t)bits_out & 7) && !((uintptr_t)idx_out & 7) && !((uintptr_t)count_out & 7) &&
                  !((uintptr_t)or_bits_dev & 7),
              KRK_EINVAL, "ring_select_dev: bits_out, idx_out, count_out and or_bits_dev must be 8-byte aligned");
    KRK_CHECK(device_writable(count_out, 8) && (!n || device_writable(digests32_dev, 32 * n)) &&
                  (!words || device_writable(bits_out, 8 * words)) && (!idx_cap || device_writable(idx_out, 8 * idx_cap)) &&
                  (!or_bits_dev || !words || device_writable(or_bits_dev, 8 * words)),
              KRK_EINVAL,
              "ring_select_dev: digests, or_bits, bits_out, idx_out and count_out must be device memory or "
              "page-locked host memory");
    hipStream_t s = pick(D, stream);
    void* d_mask = nullptr;  // copied into the library's pinned staging before this returns
    int r = upload(D, mask_host, rs::kMaskWords * 8, &d_mask, s);
    if (r) return r;
    void* d_scratch = nullptr;
    if (scratch_alloc(D, &d_scratch, ring_select_scratch_bytes(n), s) != hipSuccess) {
        scratch_free(D, d_mask, s);
        set_error(KRK_ENOMEM, "ring_select_dev: scan scratch");
        return KRK_ENOMEM;
    }
    const hipError_t e = timed(K_RSELECT, s, [&] {
        return launch_ring_select(digests32_dev, n, static_cast<const uint32_t*>(d_mask), invert, or_bits_dev, bits_out,
                                  idx_out, idx_cap, count_out, d_scratch, s);
    });
    scratch_free(D, d_scratch, s);
    scratch_free(D, d_mask, s);
    KRK_CHECK(e == hipSuccess, KRK_EHIP, "ring_select launch: %s", launch_error_text(e));
    return KRK_OK;
}

int krk_ring_select_geometry(uint64_t* digests_per_workgroup, uint64_t* scan_tile_workgroups) {
    KRK_CHECK(digests_per_workgroup && scan_tile_workgroups, KRK_EINVAL, "ring_select_geometry: null argument");
    *digests_per_workgroup = kSelectW;
    *scan_tile_workgroups = kSelectT;
    return KRK_OK;
}

}  // extern "C"
