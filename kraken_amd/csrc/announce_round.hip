// announce_round.hip -- one announce round for a batch of announces: every announcer written into
// the current peer-set window of its torrent (UpdatePeer, tracker/peerstore/redis.go:126-153), then
// every announce's handout -- GetPeers (:155-196), the origins, SortPeers
// (tracker/peerhandoutpolicy/peerhandoutpolicy.go:65-99) -- as announce_math.hpp defines it and bit
// for bit what it computes.
//
// Two launches.  The update is one thread an announce: an atomic or a bit (several announces may
// set the same bit, or bits of one word).  The handout is one wave64 workgroup an announce, over the
// updated rows.
//
// The selection within a window -- the `need` <= 64 members with the smallest composite
// (pkey << 32 | i) -- is a threshold scheme.  The wave keeps its 64 smallest composites so far one a
// lane, ascending by lane (`best`, ~0 where there is none yet), and the need-th of them as a
// wave-uniform cut.  Each lane walks the row's words at stride 64 and pops the set bits of its word
// with ctz; a candidate below the cut is appended to a pending list in LDS (ballot + prefix count).
// When 64 are pending they are sorted descending by an in-wave bitonic network (shuffles), the
// lane-wise minimum with `best` is the 64 smallest of the 128 and bitonic, and a six-stage bitonic
// merge puts it in order again; the cut tightens.  A candidate that is not below the cut cannot be
// among the need smallest, so nothing is lost; one that was below an older cut and no longer is
// loses in the merge.  The rest of the list is merged at the window's end.
// `selected` and its complete flags are at most 64 entries in LDS, never P-bit rows: a sampled
// peer is looked up among them, sets its entry's complete flag or is appended (ballot + prefix
// count), in sample order as the host form does.  The final order ranks each of the at most 72
// entries against all others (keys are distinct: c is) and stores it at its rank.
// Plain vector stores for the outputs; every trip count around a barrier is uniform over the wave;
// all index arithmetic on the offsets is 64-bit.
#include "announce_math.hpp"
#include "device_util.hpp"
#include "kernels.hpp"

namespace krk {

namespace {

constexpr uint32_t kUpdateBlock = 256;
constexpr uint64_t kEmpty = ~0ull;  // no composite: a peer's index is below 2^30

__global__ void __launch_bounds__(kUpdateBlock)
announce_update_kernel(const an::Torrent* __restrict__ tors, const an::Announce* __restrict__ anns, uint64_t n_anns,
                       uint64_t* bits) {
    const uint64_t a = (uint64_t)blockIdx.x * kUpdateBlock + threadIdx.x;
    if (a >= n_anns) return;
    const an::Announce A = anns[a];
    const an::Torrent T = tors[A.torrent];
    const uint64_t wp = (T.n_peers + 63) >> 6;
    unsigned long long* member = reinterpret_cast<unsigned long long*>(bits) + T.bits_off +
                                 an::row_off(wp, an::ring_row(T.cur_row, 0, T.n_windows));
    const unsigned long long b = 1ull << (A.peer & 63);
    atomicOr(member + (A.peer >> 6), b);
    if (A.flags & an::kComplete) atomicOr(member + wp + (A.peer >> 6), b);
}

// One compare-exchange stage of a bitonic network over the wave: the lane with bit j clear keeps the
// smaller of the pair when `up`.
__device__ __forceinline__ uint64_t cmpx(uint64_t v, uint32_t lane, uint32_t j, bool up) {
    const uint64_t o = __shfl_xor((unsigned long long)v, (int)j);
    const bool keep_min = ((lane & j) == 0) == up;
    return keep_min ? (o < v ? o : v) : (o > v ? o : v);
}
__device__ __forceinline__ uint64_t sort_desc(uint64_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t k = 2; k <= 64; k <<= 1)
#pragma unroll
        for (uint32_t j = k >> 1; j; j >>= 1) v = cmpx(v, lane, j, (lane & k) != 0);
    return v;
}
// best ascending by lane, c in any order: the 64 smallest of both, ascending by lane.
__device__ __forceinline__ uint64_t merge_best(uint64_t best, uint64_t c, uint32_t lane) {
    c = sort_desc(c, lane);
    uint64_t v = c < best ? c : best;  // bitonic, and the 64 smallest of the 128
#pragma unroll
    for (uint32_t j = 32; j; j >>= 1) v = cmpx(v, lane, j, true);
    return v;
}

__global__ void __launch_bounds__(64)
announce_handout_kernel(const an::Torrent* __restrict__ tors, const an::Announce* __restrict__ anns,
                        const uint64_t* __restrict__ bits, uint32_t limit, uint32_t policy,
                        uint32_t* __restrict__ handout, uint32_t* __restrict__ n_out, uint32_t* __restrict__ labels) {
    __shared__ uint64_t pend[128];  // candidates below the cut, not yet merged: fewer than 64 between two pops
    __shared__ uint32_t sel_c[an::kMaxLimit], sel_f[an::kMaxLimit];  // selected: peer, complete flag
    __shared__ uint64_t fk[an::kMaxEntries];                         // final order: priority << 32 | okey
    __shared__ uint32_t fv[an::kMaxEntries];                         // ... and the output word
    const uint32_t lane = threadIdx.x;
    const uint64_t lt = (1ull << lane) - 1;
    const uint64_t a = blockIdx.x;
    const an::Announce A = anns[a];
    const an::Torrent T = tors[A.torrent];
    const uint32_t cap = limit + an::kMaxOrigins;
    uint32_t* out = handout + a * cap;
    if (A.flags & an::kComplete) {  // uniform: before any barrier
        for (uint32_t j = lane; j < cap; j += 64) out[j] = an::kNone;
        if (lane == 0) n_out[a] = 0;
        if (lane < 3) labels[a * 3 + lane] = 0;
        return;
    }
    const uint64_t P = T.n_peers, wp = (P + 63) >> 6;
    const uint32_t W = T.n_windows;
    const uint64_t* rows = bits + T.bits_off;

    // the windows in ascending (wkey(w), w): lane w ranks its own
    const uint64_t wk = lane < W ? (uint64_t)an::wkey(A.seed, lane) << 32 | lane : kEmpty;
    uint32_t wrank = 0;
#pragma unroll
    for (uint32_t v = 0; v < an::kMaxWindows; ++v) wrank += __shfl((unsigned long long)wk, (int)v) < wk;

    uint32_t n_sel = 0;  // uniform
    for (uint32_t t = 0; t < W && n_sel < limit; ++t) {
        const uint32_t w = (uint32_t)__builtin_ctzll(__ballot(lane < W && wrank == t));
        const uint64_t* member = rows + an::row_off(wp, an::ring_row(T.cur_row, w, W));
        const uint32_t need = limit - n_sel;
        uint64_t best = kEmpty, cut = kEmpty;
        uint32_t n_pend = 0;  // uniform
        for (uint64_t base = 0; base < wp; base += 64) {
            const uint64_t x = base + lane;
            uint64_t word = x < wp ? member[x] & an::live_bits(P, x) : 0;
            while (__ballot(word != 0)) {  // uniform
                uint64_t cand = kEmpty;
                if (word) {
                    const uint32_t i = (uint32_t)(x * 64 + (uint64_t)__builtin_ctzll(word));
                    word &= word - 1;
                    cand = (uint64_t)an::pkey(A.seed, w, i) << 32 | i;
                }
                const bool below = cand < cut;
                const uint64_t bal = __ballot(below);
                if (!bal) continue;
                if (below) pend[n_pend + __popcll(bal & lt)] = cand;
                n_pend += (uint32_t)__popcll(bal);
                if (n_pend >= 64) {
                    __syncthreads();
                    const uint64_t c = pend[lane];
                    const uint64_t rest = pend[64 + lane];  // read by the lanes below n_pend - 64 only
                    __syncthreads();
                    best = merge_best(best, c, lane);
                    n_pend -= 64;
                    if (lane < n_pend) pend[lane] = rest;
                    cut = __shfl((unsigned long long)best, (int)(need - 1));
                }
            }
        }
        __syncthreads();
        if (n_pend) best = merge_best(best, lane < n_pend ? pend[lane] : kEmpty, lane);
        const uint32_t have = (uint32_t)__popcll(__ballot(best != kEmpty));
        const uint32_t m = need < have ? need : have;
        // the sample is lanes [0, m): look each up among the selected
        const bool in_s = lane < m;
        const uint32_t i = (uint32_t)best;
        const uint32_t c = in_s ? (uint32_t)((member[wp + (i >> 6)] >> (i & 63)) & 1) : 0;
        bool fresh = in_s;
        if (in_s)
            for (uint32_t s = 0; s < n_sel; ++s)
                if (sel_c[s] == i) {  // at most one lane an entry: a sample holds no peer twice
                    fresh = false;
                    if (c) sel_f[s] = 1;
                }
        const uint64_t nb = __ballot(fresh);
        if (fresh) {
            const uint32_t at = n_sel + (uint32_t)__popcll(nb & lt);  // < limit: the sample has at most `need`
            sel_c[at] = i;
            sel_f[at] = c;
        }
        n_sel += (uint32_t)__popcll(nb);
        __syncthreads();  // the entries, before the next window reads them; pend, before it is written again
    }

    // origins appended, source dropped, then (priority, okey(c), c) ascending
    const uint32_t O = T.n_origins;
    const uint32_t pc = lane < n_sel ? sel_c[lane] : an::kNone;
    const bool pcomp = lane < n_sel && sel_f[lane] != 0;
    const bool keep = lane < n_sel && pc != A.source;
    const uint32_t pprio = an::priority(policy, false, pcomp), oprio = an::priority(policy, true, true);
    const uint64_t kb = __ballot(keep);
    const uint32_t n_keep = (uint32_t)__popcll(kb), n = n_keep + O;
    if (keep) {
        const uint32_t e = (uint32_t)__popcll(kb & lt);
        fk[e] = (uint64_t)pprio << 32 | an::okey(A.seed, pc);
        fv[e] = pc | (pcomp ? an::kCompleteBit : 0);
    }
    if (lane < O) {
        const uint32_t oc = an::kOrigin | lane;
        fk[n_keep + lane] = (uint64_t)oprio << 32 | an::okey(A.seed, oc);
        fv[n_keep + lane] = oc;
    }
    uint32_t cnt[3];
#pragma unroll
    for (uint32_t p = 0; p < 3; ++p)
        cnt[p] = (uint32_t)__popcll(__ballot(keep && pprio == p)) + (oprio == p ? O : 0);
    __syncthreads();
    for (uint32_t e = lane; e < n; e += 64) {  // n <= 72: two entries for the first eight lanes at most
        const uint64_t k = fk[e];
        const uint32_t v = fv[e], cc = v & ~an::kCompleteBit;
        uint32_t rank = 0;
        for (uint32_t f = 0; f < n; ++f) {
            const uint64_t kf = fk[f];
            rank += kf < k || (kf == k && (fv[f] & ~an::kCompleteBit) < cc);
        }
        out[rank] = v;
    }
    for (uint32_t j = n + lane; j < cap; j += 64) out[j] = an::kNone;
    if (lane == 0) {
        n_out[a] = n;
        labels[a * 3 + 0] = cnt[0];
        labels[a * 3 + 1] = cnt[1];
        labels[a * 3 + 2] = cnt[2];
    }
}

}  // namespace

hipError_t launch_announce_round(const an::Torrent* tors, const an::Announce* anns, uint64_t n_anns, uint64_t* bits,
                                 uint32_t limit, uint32_t policy, uint32_t* handout, uint32_t* n_out, uint32_t* labels,
                                 hipStream_t s) {
    if (!n_anns) return hipSuccess;
    if (n_anns > 0x7FFFFFFFull || limit < 1 || limit > an::kMaxLimit) return hipErrorInvalidValue;
    const hipError_t pre = launch_precheck();
    if (pre != hipSuccess) return pre;
    t_launch_plan = 0;
    t_launch_units = n_anns;
    hipLaunchKernelGGL(announce_update_kernel, dim3((uint32_t)((n_anns + kUpdateBlock - 1) / kUpdateBlock)),
                       dim3(kUpdateBlock), 0, s, tors, anns, n_anns, bits);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(announce_handout_kernel, dim3((uint32_t)n_anns), dim3(64), 0, s, tors, anns,
                       static_cast<const uint64_t*>(bits), limit, policy, handout, n_out, labels);
    return hipGetLastError();
}

}  // namespace krk
