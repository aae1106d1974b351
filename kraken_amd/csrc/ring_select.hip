// ring_select.hip -- a 65,536-bit shard predicate (ring_select_math.hpp: "this origin owns the
// shard", "its owner set changed", ...) applied to n device-resident digests, answered as a
// bitset and as the ascending list of the selected indices: maybeDelete's `expired || !owns`
// (origin/blobserver/server.go:686-759) and applyToReplicas' set question (426-454) for a whole
// cache listing at once.
//
// Three phases, all index arithmetic 64-bit, every output stored by the launches themselves
// (plain vector stores, no atomics, nothing pre-zeroed):
//  1 bits     a workgroup copies the 8 KiB mask into LDS once and takes kSelectW consecutive
//             digests.  A wave takes 64 of them a step: lane l reads the two ShardID bytes of
//             record 64 w + l (one instruction reads 64 consecutive 32-byte records), looks its
//             bit up in LDS, and the ballot IS bitset word w; lane 0 ORs in the caller's or_bits
//             word, clears the bits past n and stores it.  Wave v's step k is word 4 k + v, so
//             adjacent waves store adjacent words.  The workgroup's popcounts add up to its count.
//  2 scan     the workgroup counts get an exclusive scan in tiles of kSelectT: one workgroup a
//             tile leaves each count's offset inside its tile and the tile's sum, then one
//             workgroup scans the tile sums (n / (kSelectW kSelectT) of them, 256 a pass, a
//             64-bit carry between passes) and stores the total: *count_out.
//  3 scatter  workgroup b again owns words [16 b, 16 b + 16): one wave scans their popcounts,
//             then every set lane stores its index at base(b) + bits before its word + bits
//             below its lane, when that is below idx_cap.
// No thread leaves before its kernel's last barrier.
#include "device_util.hpp"
#include "kernels.hpp"

namespace krk {

namespace {

constexpr uint32_t kWaves = 4;
constexpr uint32_t kBlock = 64 * kWaves;
constexpr uint32_t kSteps = kSelectW / kBlock;    // steps of 64 digests a wave
constexpr uint32_t kWgWords = kSelectW / 64;      // bitset words a workgroup
constexpr uint32_t kMaskU32 = 65536 / 32;
static_assert(kSelectW % kBlock == 0 && kWgWords <= 64, "one wave scans a workgroup's word popcounts");
static_assert(kSelectT == kBlock, "one count a thread in a scan tile");

// Exclusive prefix of v over the workgroup's kBlock threads (thread order) and their total.
// Every thread calls it; two barriers.
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* wsum, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();  // wsum's readers of the call before are done
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t k = 0; k < kWaves; ++k) {
        before += k < wv ? wsum[k] : 0;
        all += wsum[k];
    }
    *total = all;
    return before + inc - v;
}

__global__ void __launch_bounds__(kBlock)
ring_select_bits_kernel(const uint8_t* __restrict__ digests32, uint64_t n, const uint32_t* __restrict__ mask,
                        uint32_t invert, const uint64_t* __restrict__ or_bits, uint64_t* __restrict__ bits,
                        uint32_t* __restrict__ wg_count) {
    __shared__ uint32_t m[kMaskU32];
    __shared__ uint32_t wsum[kWaves];
    for (uint32_t i = threadIdx.x; i < kMaskU32; i += kBlock) m[i] = mask[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * kSelectW;
    uint32_t cnt = 0;  // wave-uniform
#pragma unroll
    for (uint32_t k = 0; k < kSteps; ++k) {
        const uint64_t d0 = base + (uint64_t)(k * kWaves + wv) * 64;  // wave-uniform
        const uint64_t d = d0 + lane;
        bool sel = false;
        if (d < n) {
            const uint32_t shard = (uint32_t)digests32[32 * d] << 8 | digests32[32 * d + 1];
            sel = (((m[shard >> 5] >> (shard & 31)) & 1u) ^ invert) != 0;
        }
        uint64_t word = __ballot(sel);
        if (d0 < n) {
            if (or_bits) {
                const uint64_t left = n - d0;
                word |= or_bits[d0 >> 6] & (left >= 64 ? ~0ull : (1ull << left) - 1);
            }
            if (lane == 0) bits[d0 >> 6] = word;
            cnt += (uint32_t)__popcll(word);
        }
    }
    if (lane == 0) wsum[wv] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t all = 0;
#pragma unroll
        for (uint32_t k = 0; k < kWaves; ++k) all += wsum[k];
        wg_count[blockIdx.x] = all;
    }
}

// Tile t: counts[t kSelectT + i] becomes the sum of the tile's counts before it (< 2^32: a tile
// holds kSelectT kSelectW digests), tile_sum[t] the tile's sum.
__global__ void __launch_bounds__(kBlock)
ring_select_scan_tiles_kernel(uint32_t* __restrict__ counts, uint64_t n_wg, uint32_t* __restrict__ tile_sum) {
    __shared__ uint32_t wsum[kWaves];
    const uint64_t i = (uint64_t)blockIdx.x * kSelectT + threadIdx.x;
    const uint32_t v = i < n_wg ? counts[i] : 0;
    uint32_t total;
    const uint32_t ex = block_exclusive_scan(v, wsum, &total);
    if (i < n_wg) counts[i] = ex;
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// One workgroup: tile_base[t] = the selected digests before tile t, *count_out = all of them.
__global__ void __launch_bounds__(kBlock)
ring_select_scan_sums_kernel(const uint32_t* __restrict__ tile_sum, uint64_t n_tiles, uint64_t* __restrict__ tile_base,
                             uint64_t* __restrict__ count_out) {
    __shared__ uint32_t wsum[kWaves];
    uint64_t carry = 0;
    for (uint64_t t0 = 0; t0 < n_tiles; t0 += kBlock) {  // uniform trip count
        const uint64_t t = t0 + threadIdx.x;
        const uint32_t v = t < n_tiles ? tile_sum[t] : 0;  // 256 sums of <= kSelectT kSelectW each: < 2^32
        uint32_t total;
        const uint32_t ex = block_exclusive_scan(v, wsum, &total);
        if (t < n_tiles) tile_base[t] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *count_out = carry;
}

__global__ void __launch_bounds__(kBlock)
ring_select_scatter_kernel(const uint64_t* __restrict__ bits, uint64_t n_words, const uint32_t* __restrict__ wg_off,
                           const uint64_t* __restrict__ tile_base, uint64_t* __restrict__ idx, uint64_t idx_cap) {
    __shared__ uint32_t before[kWgWords];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t w0 = (uint64_t)blockIdx.x * kWgWords;
    if (wv == 0) {
        const uint32_t pc = lane < kWgWords && w0 + lane < n_words ? (uint32_t)__popcll(bits[w0 + lane]) : 0;
        uint32_t inc = pc;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(inc, d, 64);
            if (lane >= d) inc += o;
        }
        if (lane < kWgWords) before[lane] = inc - pc;
    }
    __syncthreads();
    const uint64_t base = tile_base[blockIdx.x / kSelectT] + wg_off[blockIdx.x];
    for (uint32_t k = wv; k < kWgWords; k += kWaves) {
        const uint64_t w = w0 + k;
        if (w >= n_words) break;  // wave-uniform, past the last barrier
        const uint64_t word = bits[w];
        if ((word >> lane) & 1) {
            const uint64_t pos = base + before[k] + (uint32_t)__popcll(word & ((1ull << lane) - 1));
            if (pos < idx_cap) idx[pos] = w * 64 + lane;
        }
    }
}

}  // namespace

hipError_t launch_select_scan_scatter(uint64_t n, const uint64_t* bits, uint64_t* idx, uint64_t idx_cap,
                                      uint64_t* count_out, void* scratch, hipStream_t s) {
    const uint64_t n_wg = ring_select_workgroups(n), n_tiles = ring_select_tiles(n);
    const SelectScratch sc = select_scratch(scratch, n);
    if (n_wg) {
        hipLaunchKernelGGL(ring_select_scan_tiles_kernel, dim3((uint32_t)n_tiles), dim3(kBlock), 0, s, sc.wg_count, n_wg,
                           sc.tile_sum);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(ring_select_scan_sums_kernel, dim3(1), dim3(kBlock), 0, s, sc.tile_sum, n_tiles, sc.tile_base,
                       count_out);  // n == 0: stores the 0
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !n_wg || !idx_cap) return e;
    hipLaunchKernelGGL(ring_select_scatter_kernel, dim3((uint32_t)n_wg), dim3(kBlock), 0, s, bits, (n + 63) / 64,
                       sc.wg_count, sc.tile_base, idx, idx_cap);
    return hipGetLastError();
}

hipError_t launch_ring_select(const uint8_t* digests32, uint64_t n, const uint32_t* mask, int invert,
                              const uint64_t* or_bits, uint64_t* bits, uint64_t* idx, uint64_t idx_cap,
                              uint64_t* count_out, void* scratch, hipStream_t s) {
    const uint64_t n_wg = ring_select_workgroups(n);
    if (n_wg > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const hipError_t pre = launch_precheck();
    if (pre != hipSuccess) return pre;
    t_launch_plan = 0;
    t_launch_units = n;
    if (n_wg) {
        hipLaunchKernelGGL(ring_select_bits_kernel, dim3((uint32_t)n_wg), dim3(kBlock), 0, s, digests32, n, mask,
                           invert ? 1u : 0u, or_bits, bits, select_scratch(scratch, n).wg_count);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return launch_select_scan_scatter(n, bits, idx, idx_cap, count_out, scratch, s);
}

}  // namespace krk
