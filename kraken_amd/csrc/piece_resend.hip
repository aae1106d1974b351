// piece_resend.hip -- one resend round for a batch of torrents: every failed piece request placed
// on the first peer that may take it (Dispatcher.resendFailedPieceRequests,
// lib/torrent/scheduler/dispatch/dispatcher.go:401-434), as piece_resend_math.hpp defines it and
// bit for bit what it computes.
//
// One workgroup a torrent, its failed entries in order because the quota left and the same-piece
// state carry from one entry to the next.  One lane takes one peer, kRsS = 256 peers a pass: thread
// t owns peers t, t + kRsS, t + 2 kRsS, ... and nobody else reads or writes their state.  The first
// of them (every peer of a torrent with up to kRsS peers) has its quota left and its mark in
// registers, and its words bits_p[i >> 6] and blocked_p[i >> 6] for entry f + 1 -- two strided
// 8-byte gathers whose addresses do not depend on entry f's outcome -- are issued, with the
// wave-uniform have[i >> 6] and the entry f + 2 itself, before entry f resolves: an entry costs
// about one memory latency, not two.  The further peers' state is the thread's own words of `left`
// (quota_left_out or scratch) and `mark` (scratch), loaded in the pass that reaches them: only
// when no peer of the passes before is eligible.
// The first eligible peer: a ballot and first-set a wave, the minimum of the four waves through
// LDS (two buffers in turn, so a pass has one barrier), and the pass loop ends at the first pass
// that finds one -- the same answer in every thread.  The same-piece state is the piece last
// resent (without duplicates: uniform) or last resent to each peer (mark, with them); the list
// ascends by piece, so an equal piece means "an earlier entry of this run".
// Plain vector stores, no atomics; all index arithmetic on the offsets is 64-bit; every trip
// count and every break is uniform over the workgroup, so no thread leaves before the last
// barrier.
#include "device_util.hpp"
#include "kernels.hpp"
#include "piece_resend_math.hpp"

namespace krk {

namespace {

constexpr uint32_t kWaves = 4;
constexpr uint32_t kBlock = 64 * kWaves;
static_assert(kBlock == kRsS, "one peer a thread in a pass");

__global__ void __launch_bounds__(kBlock)
piece_resend_kernel(const RsTorrent* __restrict__ tors, const uint64_t* __restrict__ bits,
                    const int32_t* __restrict__ quota, const rs::Failed* __restrict__ failed, int32_t* left_all,
                    uint32_t* mark_all, uint32_t* __restrict__ target_out, uint32_t* __restrict__ n_resent) {
    __shared__ uint32_t wmin[2][kWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const RsTorrent T = tors[blockIdx.x];
    const uint64_t W = (T.n_pieces + 63) >> 6, P = T.n_peers, F = T.n_failed;
    const bool dup = (T.flags & pr::kAllowDuplicates) != 0;
    const uint64_t* have = bits + T.bits_off;
    const int32_t* q = quota + T.peer_off;
    int32_t* left = left_all + T.left_off;
    uint32_t* mark = mark_all + T.mark_off;
    const rs::Failed* list = failed + T.list_off;
    uint32_t* target = target_out + T.failed_off;

    const bool own0 = tid < P;
    const uint64_t* row0 = have + (1 + 2 * (uint64_t)tid) * W;  // read only under own0
    int32_t left0 = own0 ? rs::quota_left(q[tid]) : 0;
    uint32_t mark0 = pr::kNone;  // no piece has this index: n_pieces < 2^32
    for (uint64_t p = (uint64_t)tid + kRsS; p < P; p += kRsS) {
        left[p] = rs::quota_left(q[p]);
        if (dup) mark[p] = pr::kNone;
    }

    rs::Failed e1 = {0, pr::kNone, rs::kUnsent}, e2 = e1;  // entries f + 1 and f + 2
    uint64_t hv1 = 0, b1 = 0, k1 = 0;                     // entry f + 1's words: have, bits_p, blocked_p of peer tid
    if (F > 0) e1 = list[0];
    if (F > 1) e2 = list[1];
    if (F > 0) {
        const uint64_t w = e1.piece >> 6;
        hv1 = have[w];
        if (own0) b1 = row0[w], k1 = row0[W + w];
    }
    uint32_t last = pr::kNone, resent = 0, par = 0;  // the same in every thread
    for (uint64_t f = 0; f < F; ++f) {               // workgroup-uniform
        const rs::Failed e = e1;
        const uint64_t hv = hv1, b = b1, k = k1;
        e1 = e2;
        if (f + 2 < F) e2 = list[f + 2];
        if (f + 1 < F) {  // in flight while entry f resolves
            const uint64_t w = e1.piece >> 6;
            hv1 = have[w];
            if (own0) b1 = row0[w], k1 = row0[W + w];
        }
        const uint32_t i = e.piece, sh = i & 63;
        uint64_t tgt = pr::kNone;
        if (!((hv >> sh) & 1) && (dup || last != i)) {  // uniform
            const bool excl = rs::excludes_own_peer(e.status);
            for (uint64_t p0 = 0; p0 < P; p0 += kRsS) {  // uniform trip count, uniform break
                const uint64_t p = p0 + tid;
                bool ok = false;
                if (p0 == 0) {
                    ok = own0 && (((b & ~k) >> sh) & 1) && left0 > 0 && !(excl && p == e.peer) && !(dup && mark0 == i);
                } else if (p < P) {
                    const uint64_t* row = have + (1 + 2 * p) * W + (i >> 6);
                    ok = (((row[0] & ~row[W]) >> sh) & 1) && left[p] > 0 && !(excl && p == e.peer) &&
                         !(dup && mark[p] == i);
                }
                const uint64_t bal = __ballot(ok);
                if (lane == 0) wmin[par][wv] = bal ? wv * 64 + (uint32_t)__builtin_ctzll(bal) : pr::kNone;
                __syncthreads();  // the buffer of the pass before last is free: its readers are past that pass's barrier
                uint32_t m = wmin[par][0];
#pragma unroll
                for (uint32_t v = 1; v < kWaves; ++v) m = wmin[par][v] < m ? wmin[par][v] : m;
                par ^= 1;
                if (m != pr::kNone) {  // the same m in every thread
                    tgt = p0 + m;
                    if (tid == m) {  // the peer's owner
                        if (p0 == 0) {
                            --left0;
                            mark0 = i;
                        } else {
                            --left[tgt];
                            if (dup) mark[tgt] = i;
                        }
                    }
                    break;
                }
            }
            if (tgt != pr::kNone) {
                last = i;
                ++resent;
            }
        }
        if (tid == 0) target[f] = (uint32_t)tgt;
    }
    if (own0) left[tid] = left0;
    if (tid == 0) n_resent[blockIdx.x] = resent;
}

}  // namespace

hipError_t launch_piece_resend(const RsTorrent* tors, uint64_t n_tors, const uint64_t* bits, const int32_t* quota,
                               const rs::Failed* failed, int32_t* left, uint32_t* mark, uint32_t* target,
                               uint32_t* n_resent, hipStream_t s) {
    if (!n_tors) return hipSuccess;
    if (n_tors > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const hipError_t pre = launch_precheck();
    if (pre != hipSuccess) return pre;
    t_launch_plan = 0;
    t_launch_units = n_tors;
    hipLaunchKernelGGL(piece_resend_kernel, dim3((uint32_t)n_tors), dim3(kBlock), 0, s, tors, bits, quota, failed, left,
                       mark, target, n_resent);
    return hipGetLastError();
}

}  // namespace krk
