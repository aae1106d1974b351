// metainfo_json.hip -- the _torrentmeta sidecar's JSON on the device, both directions
// (metainfo_json_math.hpp: the grammar and the per-lane arithmetic the host ABI runs as well).
//
// Serialise: piece sums in device memory -> whole documents.  A unit is kSerUnit consecutive
// sums of ONE blob, one wave (a one-wave workgroup) a unit; its blob is found by the
// last-of-equals search over the blobs' first units (a blob without sums owns no unit).
//  1 count    the unit's text bytes (digits, and a comma after every sum but the blob's last):
//             a wave reduction, lane 0 stores it.
//  2 scan     an exclusive 64-bit scan of all units' byte counts (one workgroup, 64-bit carry).
//  3 format   the unit's text starts at the array's first byte + scan[u] - scan[blob's first
//             unit].  64 sums a step: a wave scan of the lanes' byte counts gives each lane's
//             offset, the lanes put their bytes into LDS at the destination's phase inside a
//             dword, and the step goes out as contiguous dword stores; only the step's unaligned
//             head and tail bytes are byte stores, so no dword is written by two lanes or waves.
//  4 envelope one lane a blob: the header through '[' (or `null`), ']' and the trailer behind
//             the body, whose size is the scan's difference over the blob's units, and out_len.
// Parse: the span between the brackets -> sums.  A unit is kParseUnit span bytes of ONE blob.
//  1 count    the unit's commas (ballot + popcount).
//  2 scan     the same scan: a number's rank is the commas before its first byte.
//  3 check    every byte's lane runs mj::parse_lane (it reads at most 11 bytes ahead and one
//             behind, inside the span; across a unit edge it only reads); the lane at a number's
//             first byte stores the value at sums_off + rank when rank < expect_n.  The unit's
//             flag (any lane found a break) is stored.
//  4 status   one wave a blob ORs its units' flags and compares the number count with expect_n.
// Every output is stored by the launches themselves: no atomics, nothing pre-zeroed.  All
// offsets are 64-bit.
#include "device_util.hpp"
#include "kernels.hpp"
#include "metainfo_json_math.hpp"

namespace krk {

namespace {

using mj::kMaxBlocks;  // kernels.hpp
using mj::kScanBlock;
using mj::kScanPer;
constexpr uint32_t kStageWords = (3 + 64 * mj::kMaxSumBytes + 3) / 4;  // a step's bytes at any phase

// The blob that owns unit u: the last one whose first unit is <= u (piece_repiece.hip).
template <class Blob>
__device__ __forceinline__ uint64_t unit_owner(const Blob* __restrict__ blobs, uint64_t n_blobs, uint64_t u) {
    uint64_t lo = 0, hi = n_blobs;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (blobs[mid].first_unit <= u) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_inclusive(uint32_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// out[i] = counts[0] + .. + counts[i - 1] for i in [0, n]: one workgroup, kScanBlock kScanPer
// counts a pass, a 64-bit carry between passes.
__global__ void __launch_bounds__(kScanBlock)
mj_scan_kernel(const uint32_t* __restrict__ counts, uint64_t n, uint64_t* __restrict__ out) {
    __shared__ uint32_t wsum[kScanBlock / 64];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint64_t carry = 0;
    for (uint64_t base = 0; base < n; base += kScanBlock * kScanPer) {  // uniform trip count
        const uint64_t i0 = base + (uint64_t)threadIdx.x * kScanPer;
        uint32_t c[kScanPer], mine = 0;
#pragma unroll
        for (uint32_t k = 0; k < kScanPer; ++k) {
            c[k] = i0 + k < n ? counts[i0 + k] : 0;  // a pass sums < 2^32: 2,048 counts of <= 2,816
            mine += c[k];
        }
        const uint32_t inc = wave_inclusive(mine, lane);
        __syncthreads();  // wsum's readers of the pass before are done
        if (lane == 63) wsum[wv] = inc;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t k = 0; k < kScanBlock / 64; ++k) {
            before += k < wv ? wsum[k] : 0;
            all += wsum[k];
        }
        uint64_t at = carry + before + (inc - mine);
#pragma unroll
        for (uint32_t k = 0; k < kScanPer; ++k) {
            if (i0 + k < n) out[i0 + k] = at;
            at += c[k];
        }
        carry += all;
    }
    if (threadIdx.x == 0) out[n] = carry;
}

// ------------------------------------------------------------------ serialise
__global__ void __launch_bounds__(64)
mj_ser_count_kernel(const MjSerBlob* __restrict__ blobs, uint64_t n_blobs, uint64_t n_units,
                    const uint32_t* __restrict__ sums, uint32_t* __restrict__ unit_bytes) {
    const uint32_t lane = threadIdx.x;
    for (uint64_t u = blockIdx.x; u < n_units; u += gridDim.x) {
        const MjSerBlob& B = blobs[unit_owner(blobs, n_blobs, u)];
        const uint64_t n = B.n_sums, i0 = (u - B.first_unit) * mj::kSerUnit;
        uint32_t bytes = 0;
#pragma unroll
        for (uint32_t k = 0; k < mj::kSerUnit / 64; ++k) {
            const uint64_t i = i0 + k * 64 + lane;
            if (i < n) bytes += mj::sum_bytes(sums[B.first_sum + i], i + 1 == n);
        }
        bytes = wave_sum(bytes);
        if (lane == 0) unit_bytes[u] = bytes;
    }
}

__global__ void __launch_bounds__(64)
mj_ser_format_kernel(const MjSerBlob* __restrict__ blobs, uint64_t n_blobs, uint64_t n_units,
                     const uint32_t* __restrict__ sums, const uint64_t* __restrict__ scan,
                     uint8_t* __restrict__ out) {
    __shared__ uint32_t stage[kStageWords];
    uint8_t* stage8 = reinterpret_cast<uint8_t*>(stage);
    const uint32_t lane = threadIdx.x;
    for (uint64_t u = blockIdx.x; u < n_units; u += gridDim.x) {  // workgroup-uniform
        const MjSerBlob& B = blobs[unit_owner(blobs, n_blobs, u)];
        const uint64_t n = B.n_sums, i0 = (u - B.first_unit) * mj::kSerUnit;
        // the array's first byte follows the header and '['
        uint64_t dst = B.out_off + mj::kHeadA + mj::i64_len(B.piece_length) + mj::kHeadB + 1 +
                       (scan[u] - scan[B.first_unit]);
        for (uint32_t k = 0; k < mj::kSerUnit / 64 && i0 + k * 64 < n; ++k) {
            const uint64_t i = i0 + k * 64 + lane;
            const bool live = i < n, last = i + 1 == n;
            const uint32_t v = live ? sums[B.first_sum + i] : 0;
            const uint32_t nd = ih::digits(v), w = live ? nd + !last : 0;
            const uint32_t inc = wave_inclusive(w, lane);
            const uint32_t total = __shfl(inc, 63, 64);
            uint8_t* g = out + dst;  // the step's first byte
            const uint32_t phase = (uint32_t)(reinterpret_cast<uintptr_t>(g) & 3);
            __syncthreads();  // the step before has read the stage
            if (live)
                mj::emit_sum(v, nd, last, phase + (inc - w), [&](uint64_t at, uint8_t c) { stage8[at] = c; });
            __syncthreads();
            // stage byte b is destination byte g - phase + b, for b in [phase, phase + total)
            const uint32_t end = phase + total;
            const uint32_t w0 = phase ? 1 : 0, w1 = end >> 2;  // the whole dwords
            uint32_t* g32 = reinterpret_cast<uint32_t*>(g - phase);
            for (uint32_t j = w0 + lane; j < w1; j += 64) g32[j] = stage[j];
            if (w1 >= w0) {
                if (phase && lane >= phase && lane < 4) g[lane - phase] = stage8[lane];      // head: w0 == 1 <= w1
                if (lane < (end & 3)) g[(w1 << 2) + lane - phase] = stage8[(w1 << 2) + lane];  // tail
            } else if (lane >= phase && lane < end) {  // the step lies inside one dword
                g[lane - phase] = stage8[lane];
            }
            dst += total;
        }
    }
}

__global__ void __launch_bounds__(256)
mj_ser_envelope_kernel(const MjSerBlob* __restrict__ blobs, uint64_t n_blobs, const uint64_t* __restrict__ scan,
                       uint8_t* __restrict__ out, uint64_t* __restrict__ out_len) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_blobs; i += stride) {
        const MjSerBlob& B = blobs[i];
        uint8_t* o = out + B.out_off;
        auto put = [&](uint64_t at, uint8_t c) { o[at] = c; };
        uint64_t at = mj::emit_head(B.piece_length, 0, put);
        if (B.sums_null) {
            at += ih::emit_text("null", 4, at, put);
        } else {
            put(at++, (uint8_t)'[');
            if (B.n_sums) at += scan[B.first_unit + mj::ser_units(B.n_sums)] - scan[B.first_unit];
            put(at++, (uint8_t)']');
        }
        at += mj::emit_tail(B.name, B.length, at, put);
        out_len[i] = at;
    }
}

// ------------------------------------------------------------------ parse
__global__ void __launch_bounds__(64)
mj_parse_count_kernel(const MjParseBlob* __restrict__ blobs, uint64_t n_blobs, uint64_t n_units,
                      const uint8_t* __restrict__ text, uint32_t* __restrict__ unit_commas) {
    const uint32_t lane = threadIdx.x;
    for (uint64_t u = blockIdx.x; u < n_units; u += gridDim.x) {
        const MjParseBlob& B = blobs[unit_owner(blobs, n_blobs, u)];
        const uint8_t* t = text + B.text_off;
        const uint64_t p0 = (u - B.first_unit) * mj::kParseUnit;
        uint32_t commas = 0;  // wave-uniform
#pragma unroll
        for (uint32_t k = 0; k < mj::kParseUnit / 64; ++k) {
            const uint64_t p = p0 + k * 64 + lane;
            commas += (uint32_t)__popcll(__ballot(p < B.text_len && t[p] == ','));
        }
        if (lane == 0) unit_commas[u] = commas;
    }
}

__global__ void __launch_bounds__(64)
mj_parse_check_kernel(const MjParseBlob* __restrict__ blobs, uint64_t n_blobs, uint64_t n_units,
                      const uint8_t* __restrict__ text, const uint64_t* __restrict__ scan,
                      uint32_t* __restrict__ sums_out, uint32_t* __restrict__ unit_flag) {
    const uint32_t lane = threadIdx.x;
    for (uint64_t u = blockIdx.x; u < n_units; u += gridDim.x) {
        const MjParseBlob& B = blobs[unit_owner(blobs, n_blobs, u)];
        const uint8_t* t = text + B.text_off;
        const uint64_t p0 = (u - B.first_unit) * mj::kParseUnit;
        uint64_t rank0 = scan[u] - scan[B.first_unit];  // commas before the step; wave-uniform
        bool bad = false;
        for (uint32_t k = 0; k < mj::kParseUnit / 64 && p0 + k * 64 < B.text_len; ++k) {
            const uint64_t p = p0 + k * 64 + lane;
            const bool live = p < B.text_len;
            bool start = false;
            uint32_t v = 0;
            if (live) bad |= mj::parse_lane(t, B.text_len, p, &start, &v);
            const uint64_t commas = __ballot(live && t[p] == ',');
            if (start) {
                const uint64_t rank = rank0 + (uint32_t)__popcll(commas & ((1ull << lane) - 1));
                if (rank < B.expect_n) sums_out[B.first_sum + rank] = v;
            }
            rank0 += (uint32_t)__popcll(commas);
        }
        const uint64_t any = __ballot(bad);
        if (lane == 0) unit_flag[u] = any ? mj::kStatusForm : 0u;
    }
}

// One wave a blob: the OR of its units' flags, and the number count against expect_n.
__global__ void __launch_bounds__(64)
mj_parse_status_kernel(const MjParseBlob* __restrict__ blobs, uint64_t n_blobs, const uint64_t* __restrict__ scan,
                       const uint32_t* __restrict__ unit_flag, uint32_t* __restrict__ status) {
    const uint32_t lane = threadIdx.x;
    for (uint64_t i = blockIdx.x; i < n_blobs; i += gridDim.x) {
        const MjParseBlob& B = blobs[i];
        const uint64_t nu = mj::parse_units(B.text_len);
        uint32_t f = 0;
        for (uint64_t k = lane; k < nu; k += 64) f |= unit_flag[B.first_unit + k];
        uint32_t st = __ballot(f != 0) ? mj::kStatusForm : 0u;
        const uint64_t commas = nu ? scan[B.first_unit + nu] - scan[B.first_unit] : 0;
        if (mj::numbers_in(commas, B.text_len) != B.expect_n) st |= mj::kStatusCount;
        if (lane == 0) status[i] = st;
    }
}

inline uint32_t grid_for(uint64_t n) { return (uint32_t)std::min<uint64_t>(n, kMaxBlocks); }

}  // namespace

hipError_t launch_metainfo_serialize(const MjSerBlob* blobs, uint64_t n_blobs, uint64_t n_units, const uint32_t* sums,
                                     uint8_t* out, uint64_t* out_len, void* scratch, hipStream_t s) {
    if (!n_blobs) return hipSuccess;
    const hipError_t pre = launch_precheck();
    if (pre != hipSuccess) return pre;
    t_launch_plan = 0;
    t_launch_units = n_units;
    // scratch: [scan u64 x (n_units + 1)][unit bytes u32 x n_units]
    uint64_t* scan = static_cast<uint64_t*>(scratch);
    uint32_t* unit_bytes = reinterpret_cast<uint32_t*>(scan + n_units + 1);
    hipError_t e;
    if (n_units) {
        hipLaunchKernelGGL(mj_ser_count_kernel, dim3(grid_for(n_units)), dim3(64), 0, s, blobs, n_blobs, n_units, sums,
                           unit_bytes);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(mj_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, unit_bytes, n_units, scan);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (n_units) {
        hipLaunchKernelGGL(mj_ser_format_kernel, dim3(grid_for(n_units)), dim3(64), 0, s, blobs, n_blobs, n_units, sums,
                           scan, out);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(mj_ser_envelope_kernel, dim3(grid_for((n_blobs + 255) / 256)), dim3(256), 0, s, blobs, n_blobs,
                       scan, out, out_len);
    return hipGetLastError();
}

hipError_t launch_metainfo_parse_sums(const MjParseBlob* blobs, uint64_t n_blobs, uint64_t n_units,
                                      const uint8_t* text, uint32_t* sums_out, uint32_t* status, void* scratch,
                                      hipStream_t s) {
    if (!n_blobs) return hipSuccess;
    const hipError_t pre = launch_precheck();
    if (pre != hipSuccess) return pre;
    t_launch_plan = 0;
    t_launch_units = n_units;
    // scratch: [scan u64 x (n_units + 1)][unit commas u32 x n_units][unit flags u32 x n_units]
    uint64_t* scan = static_cast<uint64_t*>(scratch);
    uint32_t* unit_commas = reinterpret_cast<uint32_t*>(scan + n_units + 1);
    uint32_t* unit_flag = unit_commas + n_units;
    hipError_t e;
    if (n_units) {
        hipLaunchKernelGGL(mj_parse_count_kernel, dim3(grid_for(n_units)), dim3(64), 0, s, blobs, n_blobs, n_units, text,
                           unit_commas);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(mj_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, unit_commas, n_units, scan);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (n_units) {
        hipLaunchKernelGGL(mj_parse_check_kernel, dim3(grid_for(n_units)), dim3(64), 0, s, blobs, n_blobs, n_units, text,
                           scan, sums_out, unit_flag);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(mj_parse_status_kernel, dim3(grid_for(n_blobs)), dim3(64), 0, s, blobs, n_blobs, scan, unit_flag,
                       status);
    return hipGetLastError();
}

}  // namespace krk
