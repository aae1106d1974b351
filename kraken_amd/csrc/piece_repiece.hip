// piece_repiece.hip -- a batch's stored piece sums re-pieced to a coarser piece length (a
// multiple k of the stored one) from the sums alone: new piece j's sum is the XOR over the old
// pieces i it covers of shift(old_sum_i, d_i) (repiece_math.hpp, the arithmetic the host entry
// points run as well).
//
// A wave works inside ONE blob.  k <= 64: a unit is g = 64 / k consecutive new pieces, lane l
// holds old piece l of the unit's g k (g k > 32: more than half the wave is busy), a segmented
// XOR over __shfl_down steps that stay inside a lane's segment of k (k need not be a power of
// two) leaves each new piece's sum in its segment's first lane, which stores it.  k > 64: a unit
// is one new piece, the lanes stride its old pieces by 64 and XOR their terms, one wave
// reduction, lane 0 stores.  The unit's blob is found by a search over the blobs' first units
// (ascending; a blob without pieces owns no unit).  Every output sum is stored by the launch
// itself -- no atomics, nothing pre-zeroed.  All index and distance arithmetic is 64-bit.
#include "device_util.hpp"
#include "kernels.hpp"
#include "repiece_math.hpp"

namespace krk {

namespace {

constexpr uint32_t kWaves = 4;            // waves a workgroup
constexpr uint32_t kMaxBlocks = 1u << 16;  // beyond: the waves stride

// The blob that owns unit u: the last one whose first unit is <= u.  Blobs without pieces share
// the next blob's first unit and come before it, so the last of equals owns it.
__device__ __forceinline__ uint64_t unit_owner(const RepieceBlob* __restrict__ blobs, uint64_t n_blobs, uint64_t u) {
    uint64_t lo = 0, hi = n_blobs;  // first_unit[lo] <= u < first_unit[hi]
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (blobs[mid].first_unit <= u) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(64 * kWaves)
piece_repiece_kernel(const RepieceBlob* __restrict__ blobs, uint64_t n_blobs, uint64_t n_units,
                     const uint32_t* __restrict__ x8pow, const uint32_t* __restrict__ sums,
                     uint32_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * kWaves;
    for (uint64_t u = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); u < n_units; u += stride) {  // wave-uniform
        const RepieceBlob B = blobs[unit_owner(blobs, n_blobs, u)];
        const uint64_t n_old = rp::num_pieces(B.length, B.po), n_new = rp::num_pieces(B.length, B.po * B.k);
        const uint64_t ul = u - B.first_unit;
        if (B.k <= rp::kLanes) {
            const uint32_t k = (uint32_t)B.k, g = 64 / k;
            const uint32_t seg = lane / k, pos = lane - seg * k;
            const uint64_t j = ul * g + seg, i = j * k + pos;
            const bool live = seg < g && j < n_new;
            uint32_t v = live && i < n_old ? rp::term(sums[B.first_old + i], i, B.po, B.k, B.length, x8pow) : 0u;
            for (uint32_t d = 1; d < k; d <<= 1) {  // lane pos: the XOR of its segment's [pos, pos + 2d)
                const uint32_t t = __shfl_down(v, d, 64);
                if (pos + d < k) v ^= t;
            }
            if (live && pos == 0) out[B.first_new + j] = v;
        } else {
            const uint64_t first = ul * B.k, m = n_old - first < B.k ? n_old - first : B.k;
            uint32_t v = 0;
            for (uint64_t q = lane; q < m; q += 64)
                v ^= rp::term(sums[B.first_old + first + q], first + q, B.po, B.k, B.length, x8pow);
#pragma unroll
            for (uint32_t d = 32; d; d >>= 1) v ^= __shfl_xor(v, d, 64);
            if (lane == 0) out[B.first_new + ul] = v;
        }
    }
}

}  // namespace

hipError_t launch_piece_repiece(const RepieceBlob* blobs, uint64_t n_blobs, uint64_t n_units, const uint32_t* x8pow,
                                const uint32_t* sums, uint32_t* out, hipStream_t s) {
    if (!n_blobs || !n_units) return hipSuccess;
    const hipError_t pre = launch_precheck();
    if (pre != hipSuccess) return pre;
    t_launch_plan = 0;
    t_launch_units = n_units;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_units + kWaves - 1) / kWaves, kMaxBlocks);
    hipLaunchKernelGGL(piece_repiece_kernel, dim3(blocks), dim3(64 * kWaves), 0, s, blobs, n_blobs, n_units, x8pow, sums,
                       out);
    return hipGetLastError();
}

}  // namespace krk
