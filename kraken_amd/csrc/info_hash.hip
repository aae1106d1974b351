// info_hash.hip -- info.Hash() (core/metainfo.go:37-44) of many blobs from piece sums already
// in device memory: SHA-1 over the bencoded info{Length, Name, PieceLength, PieceSums}, the
// byte stream bencode_info (host_meta.cpp) writes, never materialised in global memory.
//
// One wave (one 64-thread workgroup) a blob.  A step formats 64 sums, one a lane: digit count
// from a compare ladder, digits by multiply-high (info_hash_math.hpp), each lane's byte offset
// from a wave-wide exclusive scan of the byte counts; the bytes go into a 1 KiB LDS ring
// (kRingBytes: the only LDS a workgroup holds, so the 32-wave cap and not LDS bounds the
// workgroups a CU takes).  The wave then compresses every complete 64-byte block of the ring:
// the chain is sequential, so all lanes read the same sixteen words (an LDS broadcast) and
// carry the same state -- a wave issues one instruction for 64 lanes or for one alike.  The
// header, the name's bytes, the closing "ee" and the SHA-1 padding go through the same ring.
// A workgroup is one wave, so its barriers order the ring's writes and reads at no cost.
// Jobs arrive longest first (info_hash_dev.cpp): the longest chains start first, and the
// launch ends with its longest chain.
#include "device_util.hpp"
#include "info_hash_math.hpp"
#include "kernels.hpp"

namespace krk {

namespace {

// Exclusive prefix sum of v over the wave's 64 lanes; *total = the wave's sum.
__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v, uint32_t lane, uint32_t* total) {
    uint32_t inc = v;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    *total = __shfl(inc, 63, 64);
    return inc - v;
}

__global__ void __launch_bounds__(64)
info_hash_kernel(const InfoHashJob* __restrict__ jobs, uint32_t n_jobs, const uint32_t* __restrict__ sums,
                 const uint8_t* __restrict__ names, uint8_t* __restrict__ out20) {
    __shared__ alignas(16) uint32_t ring[ih::kRingWords];
    uint8_t* ring8 = reinterpret_cast<uint8_t*>(ring);
    const uint32_t lane = threadIdx.x;
    gptr<uint32_t> gs = as_global<uint32_t>(reinterpret_cast<uint64_t>(sums));
    gptr<uint8_t> gn = as_global<uint8_t>(reinterpret_cast<uint64_t>(names));
    for (uint32_t j = blockIdx.x; j < n_jobs; j += gridDim.x) {  // uniform in the workgroup
        const InfoHashJob J = jobs[j];
        uint32_t h[5];
        ih::sha1_init(h);
        uint64_t pos = 0, done = 0;  // stream bytes written to the ring / compressed out of it
        auto put = [&](uint64_t at, uint8_t c) { ring8[ih::ring_byte(at)] = c; };
        auto put0 = [&](uint64_t at, uint8_t c) {  // text every lane computes alike: lane 0 stores it
            if (lane == 0) ring8[ih::ring_byte(at)] = c;
        };
        auto drain = [&]() {
            __syncthreads();
            while (pos - done >= 64) {
                uint32_t w[16];
                const uint32_t b = ih::ring_block(done);
#pragma unroll
                for (int i = 0; i < 16; ++i) w[i] = ring[b + i];
                ih::sha1_block(h, w);
                done += 64;
            }
            __syncthreads();
        };

        pos += ih::header_before_name(J.length, J.name_len, pos, put0);
        drain();
        for (uint64_t base = 0; base < J.name_len; base += 64) {  // 64 name bytes a step
            const uint64_t i = base + lane;
            if (i < J.name_len) put(pos + lane, gn[J.name_off + i]);
            pos += J.name_len - base < 64 ? J.name_len - base : 64;
            drain();
        }
        pos += ih::header_after_name(J.piece_length, pos, put0);
        drain();

        uint32_t v = lane < J.n_sums ? gs[J.first_sum + lane] : 0u;
        for (uint64_t base = 0; base < J.n_sums; base += 64) {
            const uint64_t i = base + lane;
            const bool act = i < J.n_sums;
            // the next step's sums are on their way while this step's blocks are compressed
            const uint32_t vn = i + 64 < J.n_sums ? gs[J.first_sum + i + 64] : 0u;
            const uint32_t nd = ih::digits(v);
            uint32_t total;
            const uint32_t off = wave_excl_scan(act ? nd + 2 : 0u, lane, &total);
            if (act) ih::emit_sum(v, nd, pos + off, put);
            pos += total;
            drain();
            v = vn;
        }

        if (lane < 2) put(pos + lane, (uint8_t)'e');
        pos += 2;
        const uint64_t total = pos;
        const uint32_t n_pad = ih::pad_bytes(total);
        for (uint32_t k = lane; k < n_pad; k += 64) put(total + k, ih::pad_byte(k, n_pad, total));
        pos += n_pad;
        drain();
        if (lane < 20) out20[20 * J.out + lane] = ih::digest_byte(h, lane);
    }
}

}  // namespace

hipError_t launch_info_hash(const InfoHashJob* jobs, uint32_t n_jobs, const uint32_t* sums, const uint8_t* names,
                            uint8_t* out20, hipStream_t s) {
    if (!n_jobs) return hipSuccess;
    const hipError_t pre = launch_precheck();
    if (pre != hipSuccess) return pre;
    t_launch_plan = 0;
    t_launch_units = n_jobs;
    hipLaunchKernelGGL(info_hash_kernel, dim3(std::min<uint32_t>(n_jobs, 1u << 20)), dim3(64), 0, s, jobs, n_jobs, sums,
                       names, out20);
    return hipGetLastError();
}

}  // namespace krk
