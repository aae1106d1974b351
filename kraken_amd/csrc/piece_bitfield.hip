// piece_bitfield.hip -- a batch's piece sums against the sums its metainfo stores, answered as
// the reference answers it: Torrent.Bitfield() (lib/torrent/storage/agentstorage/torrent.go:
// 130-140), a willf/bitset -- []uint64, piece i is bit i & 63 of word i >> 6, 1 = complete.
//
// A wave is 64 lanes, so one ballot over 64 consecutive pieces IS one bitset word: a wave takes
// one word of ONE blob (a blob's first piece is lane 0 of its first word, a word never spans two
// blobs), lane l compares piece 64 w + l, lane 0 stores the ballot.  Lanes past the blob's last
// piece vote 0, so the tail bits of a blob's last word are zero.  The word's blob is found by a
// search over the blobs' first words (ascending; a blob without pieces owns no word).  A second
// launch, one wave a blob, counts the set bits of the blob's words: n_bad = pieces - set bits.
// Every output word and count is stored by the launch itself -- no atomics, nothing pre-zeroed.
// All index arithmetic is 64-bit.
#include "device_util.hpp"
#include "kernels.hpp"

namespace krk {

namespace {

constexpr uint32_t kWaves = 4;            // waves a workgroup
constexpr uint32_t kMaxBlocks = 1u << 16;  // beyond: the waves stride

// The blob that owns bitfield word w: the last one whose first word is <= w.  Blobs without
// pieces share the next blob's first word and come before it, so the last of equals owns it.
__device__ __forceinline__ uint64_t word_owner(const BitfieldBlob* __restrict__ blobs, uint64_t n_blobs, uint64_t w) {
    uint64_t lo = 0, hi = n_blobs;  // first_word[lo] <= w < first_word[hi]
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (blobs[mid].first_word <= w) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(64 * kWaves)
piece_bitfield_kernel(const BitfieldBlob* __restrict__ blobs, uint64_t n_blobs, uint64_t n_words,
                      const uint32_t* __restrict__ sums, const uint32_t* __restrict__ expected,
                      uint64_t* __restrict__ bits) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * kWaves;
    for (uint64_t w = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); w < n_words; w += stride) {  // wave-uniform
        const BitfieldBlob B = blobs[word_owner(blobs, n_blobs, w)];
        const uint64_t piece = (w - B.first_word) * 64 + lane;
        const bool ok = piece < B.n_pieces && sums[B.first_sum + piece] == expected[B.first_sum + piece];
        const uint64_t word = __ballot(ok);
        if (lane == 0) bits[w] = word;
    }
}

__global__ void __launch_bounds__(64 * kWaves)
bitfield_count_kernel(const BitfieldBlob* __restrict__ blobs, uint64_t n_blobs, const uint64_t* __restrict__ bits,
                      uint32_t* __restrict__ n_bad) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * kWaves;
    for (uint64_t b = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); b < n_blobs; b += stride) {
        const BitfieldBlob B = blobs[b];
        const uint64_t words = (B.n_pieces + 63) / 64;
        uint32_t good = 0;  // n_pieces < 2^32
        for (uint64_t k = lane; k < words; k += 64) good += (uint32_t)__popcll(bits[B.first_word + k]);
#pragma unroll
        for (uint32_t d = 32; d; d >>= 1) good += __shfl_xor(good, d, 64);
        if (lane == 0) n_bad[b] = (uint32_t)B.n_pieces - good;
    }
}

// ok[i] = digests[32 i, +32) == expected[32 i, +32); both arrays 16-byte aligned.
__global__ void __launch_bounds__(256)
digest_equal_kernel(const u32x4* __restrict__ digests, const u32x4* __restrict__ expected, uint64_t n,
                    uint8_t* __restrict__ ok) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const u32x4 x = (digests[2 * i] ^ expected[2 * i]) | (digests[2 * i + 1] ^ expected[2 * i + 1]);
        ok[i] = (x.x | x.y | x.z | x.w) == 0;
    }
}

inline uint32_t blocks_for(uint64_t units, uint32_t per_block) {
    return (uint32_t)std::min<uint64_t>((units + per_block - 1) / per_block, kMaxBlocks);
}

}  // namespace

hipError_t launch_piece_bitfield(const BitfieldBlob* blobs, uint64_t n_blobs, uint64_t n_words, const uint32_t* sums,
                                 const uint32_t* expected, uint64_t* bits, uint32_t* n_bad, hipStream_t s) {
    if (!n_blobs) return hipSuccess;
    const hipError_t pre = launch_precheck();
    if (pre != hipSuccess) return pre;
    t_launch_plan = 0;
    t_launch_units = n_words;
    if (n_words) {
        hipLaunchKernelGGL(piece_bitfield_kernel, dim3(blocks_for(n_words, kWaves)), dim3(64 * kWaves), 0, s, blobs,
                           n_blobs, n_words, sums, expected, bits);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(bitfield_count_kernel, dim3(blocks_for(n_blobs, kWaves)), dim3(64 * kWaves), 0, s, blobs, n_blobs,
                       bits, n_bad);
    return hipGetLastError();
}

hipError_t launch_digest_equal(const uint8_t* digests, const uint8_t* expected, uint64_t n, uint8_t* ok,
                               hipStream_t s) {
    if (!n) return hipSuccess;
    const hipError_t pre = launch_precheck();
    if (pre != hipSuccess) return pre;
    hipLaunchKernelGGL(digest_equal_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s,
                       reinterpret_cast<const u32x4*>(digests), reinterpret_cast<const u32x4*>(expected), n, ok);
    return hipGetLastError();
}

}  // namespace krk
