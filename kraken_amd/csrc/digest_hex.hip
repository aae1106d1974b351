// digest_hex.hip -- a cache listing's text on the device (digest_hex_math.hpp's arithmetic): the
// SHA-256 hex codec (core.NewSHA256DigestFromHex / Digest.Hex(), core/digest.go:57-68,143-161)
// and maybeDelete's `expired || !owns` (origin/blobserver/server.go:686-759) answered from the
// hex names and mtimes themselves.
//
//  parse   a workgroup of 4 waves takes kDhexW consecutive names; a wave takes 64 of them a step,
//          lane l name 64 w + l, wave v's step k word 4 k + v.  The lane reads its two offsets,
//          and only for a length of 64 the name's bytes: four 16-byte loads where the name is
//          16-byte aligned, aligned dword loads where those dwords lie wholly inside
//          names[off[0], off[n]), byte by byte at a misaligned listing's two ends otherwise, so no
//          byte outside the listing is read at any alignment.  The ballot of
//          "valid" IS word w of the valid bitset (bits past n are 0: those lanes vote 0).
//  format  the same geometry, lane l digest 64 w + l.
//  plan    phase 1 of ring_select.hip fused with the parse: the same geometry and scratch
//          (kSelectW names a workgroup, the mask in LDS, a workgroup count), sel = valid &
//          ((mask[ShardID] ^ invert) | expired(now, mtime, ttl)); the ballots of sel and valid are
//          stored, no digest, status or expired array is.  The scan and scatter are
//          ring_select.hip's (launch_select_scan_scatter).
// Plain vector stores, no atomics, nothing pre-zeroed, all offsets 64-bit.  No thread leaves
// before its kernel's last barrier (only the plan kernel has any).
#include "device_util.hpp"
#include "digest_hex_math.hpp"
#include "kernels.hpp"

namespace krk {

namespace {

constexpr uint32_t kWaves = 4;
constexpr uint32_t kBlock = 64 * kWaves;
constexpr uint32_t kSteps = kDhexW / kBlock;
constexpr uint32_t kMaskU32 = 65536 / 32;
static_assert(kDhexW % kBlock == 0 && kSelectW % kBlock == 0, "whole steps of 64 names a wave");

// The 64 bytes at a as 16 little-endian words; [lo, hi) are the listing's bytes.
__device__ __forceinline__ void load_name(uint64_t a, uint64_t lo, uint64_t hi, uint32_t w[16]) {
    if ((a & 15) == 0) {  // the name itself, a 16-byte word a load: wholly inside whatever surrounds it
        gptr<u32x4> q = as_global<u32x4>(a);
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const u32x4 v = q[k];
            w[4 * k] = v.x, w[4 * k + 1] = v.y, w[4 * k + 2] = v.z, w[4 * k + 3] = v.w;
        }
    } else if ((a & ~uint64_t(3)) >= lo && ((a + 67) & ~uint64_t(3)) <= hi) {
        load_bytes64(a, 64, w, lo, hi);
    } else {
        gptr<uint8_t> p = as_global<uint8_t>(a);
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k)
            w[k] = (uint32_t)p[4 * k] | (uint32_t)p[4 * k + 1] << 8 | (uint32_t)p[4 * k + 2] << 16 |
                   (uint32_t)p[4 * k + 3] << 24;
    }
}

// kWords words to p at any alignment.
template <uint32_t kWords>
__device__ __forceinline__ void store_words(uint8_t* p, const uint32_t* v) {
    if (((uint64_t)p & 3) == 0) {
        uint32_t* q = reinterpret_cast<uint32_t*>(p);
#pragma unroll
        for (uint32_t j = 0; j < kWords; ++j) q[j] = v[j];
    } else {
#pragma unroll
        for (uint32_t j = 0; j < kWords; ++j) {
            p[4 * j] = (uint8_t)v[j], p[4 * j + 1] = (uint8_t)(v[j] >> 8);
            p[4 * j + 2] = (uint8_t)(v[j] >> 16), p[4 * j + 3] = (uint8_t)(v[j] >> 24);
        }
    }
}

// Name i's status and digest words (zero unless valid).
__device__ __forceinline__ uint32_t parse_at(const uint8_t* names, const uint64_t* off, uint64_t i, uint64_t lo,
                                             uint64_t hi, uint32_t d[8]) {
    const uint64_t o = off[i];
    const uint32_t ls = dh::len_status(off[i + 1] - o);
    if (ls) {
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) d[j] = 0;
        return ls;
    }
    uint32_t w[16];
    load_name((uint64_t)names + o, lo, hi, w);
    return dh::parse_words(w, d);
}

__global__ void __launch_bounds__(kBlock)
digest_parse_hex_kernel(const uint8_t* __restrict__ names, const uint64_t* __restrict__ off, uint64_t n,
                        uint8_t* __restrict__ digests32, uint32_t* __restrict__ status, uint64_t* __restrict__ valid) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * kDhexW;
    const uint64_t lo = (uint64_t)names + off[0], hi = (uint64_t)names + off[n];
    for (uint32_t k = 0; k < kSteps; ++k) {
        const uint64_t i0 = base + (uint64_t)(k * kWaves + wv) * 64;  // wave-uniform
        if (i0 >= n) break;
        const uint64_t i = i0 + lane;
        bool ok = false;
        if (i < n) {
            uint32_t d[8];
            const uint32_t st = parse_at(names, off, i, lo, hi, d);
            store_words<8>(digests32 + 32 * i, d);
            if (status) status[i] = st;
            ok = st == 0;
        }
        const uint64_t word = __ballot(ok);
        if (valid && lane == 0) valid[i0 >> 6] = word;
    }
}

__global__ void __launch_bounds__(kBlock)
digest_format_hex_kernel(const uint8_t* __restrict__ digests32, uint64_t n, uint8_t* __restrict__ hex) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * kDhexW;
    for (uint32_t k = 0; k < kSteps; ++k) {
        const uint64_t i = base + (uint64_t)(k * kWaves + wv) * 64 + lane;
        if (i >= n) break;
        const uint8_t* p = digests32 + 32 * i;
        uint32_t d[8], h[16];
        if (((uint64_t)p & 3) == 0) {
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j) d[j] = reinterpret_cast<const uint32_t*>(p)[j];
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j)
                d[j] = (uint32_t)p[4 * j] | (uint32_t)p[4 * j + 1] << 8 | (uint32_t)p[4 * j + 2] << 16 |
                       (uint32_t)p[4 * j + 3] << 24;
        }
        dh::format_words(d, h);
        store_words<16>(hex + 64 * i, h);
    }
}

// Phase 1 of the plan: ring_select_bits_kernel's geometry and outputs, its digests parsed from
// the listing's text in registers.
__global__ void __launch_bounds__(kBlock)
cleanup_plan_bits_kernel(const uint8_t* __restrict__ names, const uint64_t* __restrict__ off, uint64_t n,
                         const int64_t* __restrict__ mtime, int64_t now, int64_t ttl, const uint32_t* __restrict__ mask,
                         uint32_t invert, uint64_t* __restrict__ bits, uint64_t* __restrict__ valid,
                         uint32_t* __restrict__ wg_count) {
    __shared__ uint32_t m[kMaskU32];
    __shared__ uint32_t wsum[kWaves];
    for (uint32_t i = threadIdx.x; i < kMaskU32; i += kBlock) m[i] = mask[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * kSelectW;
    const uint64_t lo = (uint64_t)names + off[0], hi = (uint64_t)names + off[n];
    uint32_t cnt = 0;  // wave-uniform
    for (uint32_t k = 0; k < kSelectW / kBlock; ++k) {
        const uint64_t i0 = base + (uint64_t)(k * kWaves + wv) * 64;  // wave-uniform
        const uint64_t i = i0 + lane;
        bool ok = false, sel = false;
        if (i < n) {
            uint32_t d[8];
            ok = parse_at(names, off, i, lo, hi, d) == 0;
            const uint32_t shard = (d[0] & 0xFF) << 8 | ((d[0] >> 8) & 0xFF);
            sel = (((m[shard >> 5] >> (shard & 31)) & 1u) ^ invert) != 0;
            if (mtime) sel = sel || dh::expired(now, mtime[i], ttl);
            sel = sel && ok;
        }
        const uint64_t word = __ballot(sel), vword = __ballot(ok);
        if (i0 < n) {
            if (lane == 0) {
                bits[i0 >> 6] = word;
                if (valid) valid[i0 >> 6] = vword;
            }
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

inline uint64_t dhex_workgroups(uint64_t n) { return n / kDhexW + (n % kDhexW != 0); }

}  // namespace

hipError_t launch_digest_parse_hex(const uint8_t* names, const uint64_t* off, uint64_t n, uint8_t* digests32,
                                   uint32_t* status, uint64_t* valid, hipStream_t s) {
    const uint64_t n_wg = dhex_workgroups(n);
    if (n_wg > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const hipError_t pre = launch_precheck();
    if (pre != hipSuccess) return pre;
    t_launch_plan = 0;
    t_launch_units = n;
    if (!n_wg) return hipSuccess;
    hipLaunchKernelGGL(digest_parse_hex_kernel, dim3((uint32_t)n_wg), dim3(kBlock), 0, s, names, off, n, digests32,
                       status, valid);
    return hipGetLastError();
}

hipError_t launch_digest_format_hex(const uint8_t* digests32, uint64_t n, uint8_t* hex, hipStream_t s) {
    const uint64_t n_wg = dhex_workgroups(n);
    if (n_wg > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const hipError_t pre = launch_precheck();
    if (pre != hipSuccess) return pre;
    t_launch_plan = 0;
    t_launch_units = n;
    if (!n_wg) return hipSuccess;
    hipLaunchKernelGGL(digest_format_hex_kernel, dim3((uint32_t)n_wg), dim3(kBlock), 0, s, digests32, n, hex);
    return hipGetLastError();
}

hipError_t launch_cleanup_plan(const uint8_t* names, const uint64_t* off, uint64_t n, const int64_t* mtime, int64_t now,
                               int64_t ttl, const uint32_t* mask, int invert, uint64_t* bits, uint64_t* valid,
                               uint64_t* idx, uint64_t idx_cap, uint64_t* count_out, void* scratch, hipStream_t s) {
    const uint64_t n_wg = ring_select_workgroups(n);
    if (n_wg > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const hipError_t pre = launch_precheck();
    if (pre != hipSuccess) return pre;
    t_launch_plan = 0;
    t_launch_units = n;
    if (n_wg) {
        hipLaunchKernelGGL(cleanup_plan_bits_kernel, dim3((uint32_t)n_wg), dim3(kBlock), 0, s, names, off, n, mtime, now,
                           ttl, mask, invert ? 1u : 0u, bits, valid, select_scratch(scratch, n).wg_count);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return launch_select_scan_scatter(n, bits, idx, idx_cap, count_out, scratch, s);
}

}  // namespace krk
