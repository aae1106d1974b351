// piece_request.hip -- one piece request round for a batch of torrents: the availability counts
// numPeersByPiece (lib/torrent/scheduler/dispatch/dispatcher.go:257-284) and
// piecerequest.Manager.ReservePieces (piecerequest/manager.go:101-137) for every peer of every
// torrent, as piece_request_math.hpp defines them and bit for bit what it computes.
//
//  counts  one lane a piece.  A workgroup pass covers kPrG = 256 pieces of ONE torrent: wave v
//          takes bitset word 4 u + v of every peer row (a wave-uniform word), lane l adds its
//          bit, and the 64 counts go out as one coalesced store of 32-bit values.  Lanes past
//          the torrent's last piece store nothing, so tail bits are never counted.  The unit's
//          torrent is found by a search over the torrents' first units.
//  round   one workgroup a torrent, its peers in order because `taken` carries from one peer to
//          the next.  A pick is the workgroup-wide minimum of the packed key
//          (uint64)key(i) << 32 | i over the lanes whose piece is a candidate
//          (bits_p & ~have & ~blocked_p & ~taken) and whose packed key is above the pick before
//          it: one lane a piece again (a scan step covers kPrPass = 4,096 pieces, wave v taking
//          words 4 k + v, k < 16, with every load of the step in flight at once: the scan is a
//          chain of memory latencies, one a step), the wave minimum by shuffles, the four wave
//          minima through LDS.  Thread 0 stores the pick and sets its bit in the torrent's `taken` row (device
//          scratch, zeroed by the workgroup itself); the barrier that ends the pass makes it
//          visible to the next scan.  min(quota, candidates) passes a peer: the pass that finds
//          no candidate ends the peer for every thread alike.
// Plain vector stores, no atomics; all index arithmetic on the offsets is 64-bit; every trip
// count and every break is uniform over the workgroup, so no thread leaves before its kernel's
// last barrier.
#include "device_util.hpp"
#include "kernels.hpp"
#include "piece_request_math.hpp"

namespace krk {

namespace {

constexpr uint32_t kWaves = 4;
constexpr uint32_t kBlock = 64 * kWaves;
constexpr uint32_t kWords = kPrPass / kPrG;  // bitset words a wave takes in one step of the selection scan
static_assert(kBlock == kPrG && kPrPass % kPrG == 0, "one piece a thread in a count unit, whole strides in a scan step");

// The torrent that owns count unit u: the last one whose first unit is <= u (torrents without
// pieces share the next torrent's first unit and come before it).
__device__ __forceinline__ uint64_t unit_owner(const PrTorrent* __restrict__ tors, uint64_t n_tors, uint64_t u) {
    uint64_t lo = 0, hi = n_tors;  // first_unit[lo] <= u < first_unit[hi]
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (tors[mid].first_unit <= u) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(kBlock)
piece_request_counts_kernel(const PrTorrent* __restrict__ tors, uint64_t n_tors, uint64_t n_units,
                            const uint64_t* __restrict__ bits, uint32_t* __restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint64_t u = blockIdx.x; u < n_units; u += gridDim.x) {  // workgroup-uniform
        const PrTorrent T = tors[unit_owner(tors, n_tors, u)];
        const uint64_t W = (T.n_pieces + 63) >> 6;
        const uint64_t w = (u - T.first_unit) * kWaves + wv;  // wave-uniform
        if (w >= W) continue;
        const uint64_t* row = bits + T.bits_off + W + w;  // peer 0's word
        uint32_t c = 0;
        for (uint32_t p = 0; p < T.n_peers; ++p, row += 2 * W) c += (uint32_t)(row[0] >> lane) & 1u;
        const uint64_t i = w * 64 + lane;
        if (i < T.n_pieces) counts[T.piece_off + i] = c;
    }
}

__global__ void __launch_bounds__(kBlock)
piece_request_round_kernel(const PrTorrent* __restrict__ tors, const uint64_t* __restrict__ bits,
                           const int32_t* __restrict__ quota, uint32_t limit, const uint32_t* counts,
                           uint64_t* taken_all, uint32_t* __restrict__ picks, uint32_t* __restrict__ n_picked) {
    __shared__ uint64_t wmin[kWaves];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const PrTorrent T = tors[blockIdx.x];
    const uint64_t W = (T.n_pieces + 63) >> 6;
    const bool dup = (T.flags & pr::kAllowDuplicates) != 0;
    const bool sample = (T.flags & pr::kPolicyMask) == pr::kSample;
    const uint64_t* have = bits + T.bits_off;
    uint64_t* taken = taken_all + T.taken_off;
    if (!dup)
        for (uint64_t w = threadIdx.x; w < W; w += kBlock) taken[w] = 0;
    __syncthreads();
    for (uint32_t p = 0; p < T.n_peers; ++p) {
        const uint64_t* row = have + (1 + 2 * (uint64_t)p) * W;
        const uint64_t* blk = row + W;
        const uint64_t po = T.peer_off + p;
        const int32_t qi = quota[po];
        const uint32_t q = qi <= 0 ? 0u : ((uint32_t)qi < limit ? (uint32_t)qi : limit);
        uint64_t bound = 0;  // packed keys below it are this peer's picks already
        uint32_t got = 0;
        while (got < q) {  // workgroup-uniform
            uint64_t best = ~0ull;  // no packed key has this value: i < 2^32 - 1
            for (uint64_t w0 = 0; w0 < W; w0 += kWaves * kWords) {  // uniform trip count
                // kWords words a wave a step, every load issued before the first use: a step costs
                // one memory latency, not kWords
                uint64_t word[kWords];
                uint32_t cnt[kWords];
#pragma unroll
                for (uint32_t u = 0; u < kWords; ++u) {
                    const uint64_t w = w0 + u * kWaves + wv;  // wave-uniform
                    word[u] = 0;
                    cnt[u] = 0;
                    if (w >= W) continue;
                    word[u] = row[w] & ~have[w] & ~blk[w];
                    if (!dup) word[u] &= ~taken[w];
                    const uint64_t i = w * 64 + lane;
                    if (!sample && i < T.n_pieces) cnt[u] = counts[T.piece_off + i];
                }
#pragma unroll
                for (uint32_t u = 0; u < kWords; ++u) {
                    const uint64_t i = (w0 + u * kWaves + wv) * 64 + lane;
                    if (((word[u] >> lane) & 1) && i < T.n_pieces) {
                        const uint32_t key = sample ? pr::sample_key(T.seed, p, (uint32_t)i) : cnt[u];
                        const uint64_t pk = (uint64_t)key << 32 | i;
                        if (pk >= bound && pk < best) best = pk;
                    }
                }
            }
#pragma unroll
            for (uint32_t d = 32; d; d >>= 1) {
                const uint64_t o = __shfl_xor(best, d, 64);
                best = o < best ? o : best;
            }
            __syncthreads();  // wmin's readers of the pass before are done
            if (lane == 0) wmin[wv] = best;
            __syncthreads();
            uint64_t m = wmin[0];
#pragma unroll
            for (uint32_t k = 1; k < kWaves; ++k) m = wmin[k] < m ? wmin[k] : m;
            if (m == ~0ull) break;  // no candidate left: the same m in every thread
            if (threadIdx.x == 0) {  // this peer's next scan skips the pick by `bound`, whichever taken word it reads
                const uint32_t i = (uint32_t)m;
                picks[po * limit + got] = i;
                if (!dup) taken[i >> 6] |= 1ull << (i & 63);
            }
            bound = m + 1;
            ++got;
        }
        if (threadIdx.x == 0) n_picked[po] = got;
        for (uint32_t j = got + threadIdx.x; j < limit; j += kBlock) picks[po * limit + j] = pr::kNone;
        __syncthreads();  // thread 0's taken bits, before the next peer's scan
    }
}

}  // namespace

hipError_t launch_piece_request(const PrTorrent* tors, uint64_t n_tors, uint64_t n_units, const uint64_t* bits,
                                const int32_t* quota, uint32_t limit, uint32_t* counts, uint64_t* taken,
                                uint32_t* picks, uint32_t* n_picked, hipStream_t s) {
    if (!n_tors) return hipSuccess;
    if (n_tors > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const hipError_t pre = launch_precheck();
    if (pre != hipSuccess) return pre;
    t_launch_plan = 0;
    t_launch_units = n_tors;
    if (counts && n_units) {
        hipLaunchKernelGGL(piece_request_counts_kernel, dim3((uint32_t)std::min<uint64_t>(n_units, kPrMaxBlocks)),
                           dim3(kBlock), 0, s, tors, n_tors, n_units, bits, counts);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(piece_request_round_kernel, dim3((uint32_t)n_tors), dim3(kBlock), 0, s, tors, bits, quota, limit,
                       counts, taken, picks, n_picked);
    return hipGetLastError();
}

}  // namespace krk
