// conn_round.hip -- one connection round for a batch of torrents (connstate.State,
// lib/torrent/scheduler/connstate/state.go, driven by lib/torrent/scheduler/events.go:125-285) and
// the preemption sweep (events.go:370-392), as conn_math.hpp defines them and bit for bit what it
// computes: rows, expiries, capacities and every output.
//
// The round is one wave64 a torrent: no barrier, no LDS.  The capacity, the admitted and the freed
// counts are wave-uniform registers; lane 0 stores them at the end.
// Phase 1, transitions: one lane an entry, 64 entries a step.  The peers of a list are distinct,
// so an entry's bit is its lane's alone in this phase: the lane reads its words, clears and sets
// its bit with 64-bit atomics (two entries may share a word) and writes its own expiry.  The
// step's frees are the popcount of a ballot.
// Phase 2, incoming handshakes, in list order.  Lane l owns words l, l + 64, ... of the active
// and pending rows: for P <= 4096 one register each a lane, and an admission sets its bit in the
// owning lane's register with no memory round trip between entries; past that the owning lane
// rereads and rewrites its own further words, so program order suffices.  An entry's own bits are
// a shuffle from the owning lane; its mutual count is a per-lane popcount of
// neigh & (active | pending), tail-masked, and a wave reduction.  Entry f + 1's neighbour word
// and entry f + 2 itself are loaded before entry f resolves.  The pending registers are written
// back once, at the end of the phase.
// Phase 3, dials: 64 candidates a step.  Each lane gathers its candidate's expiry and its pending
// and active words and classifies it; among the lanes of a step the first occurrence of a peer in
// list order is found with a readlane loop, never by the atomics' arrival order; the admissible
// first occurrences are ranked by ballot and prefix count and admitted while rank < capacity.
// The entry that takes the last slot cuts the step: every contender after it is AT_CAPACITY,
// everything before it keeps the status the sequential rule gives it.
// Ordering.  The rows are read with agent-scope atomic loads and changed with agent-scope atomic
// and / or, so no read is served by a stale line of the vector cache.  Between the phases, and
// between two steps of phase 3 -- where a later step must see the pending bits the other lanes of
// an earlier step set -- there is a sequentially consistent agent-scope fence: the atomics and
// stores before it have completed and the vector cache is invalidated before any load after it
// issues, and the compiler moves no load across it.
// All index arithmetic on the offsets is 64-bit; every trip count is wave-uniform.
#include "conn_math.hpp"
#include "device_util.hpp"
#include "kernels.hpp"

namespace krk {

namespace {

typedef unsigned long long ull;

__device__ __forceinline__ uint64_t ld(const uint64_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void set_bit(uint64_t* p, uint64_t b) {
    __hip_atomic_fetch_or(p, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void clear_bit(uint64_t* p, uint64_t b) {
    __hip_atomic_fetch_and(p, ~b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void phase_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent"); }
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int j = 32; j; j >>= 1) v += __shfl_xor(v, j);
    return v;
}

__global__ void __launch_bounds__(64)
conn_round_kernel(const CnTorrent* __restrict__ tors, const cn::Transition* __restrict__ trs,
                  const cn::Incoming* __restrict__ ins, const uint32_t* __restrict__ dials,
                  const uint64_t* __restrict__ neighbors, uint64_t* bits, int64_t* expiry, uint32_t* capacity,
                  const cn::Round R, uint32_t* __restrict__ tr_st, uint32_t* __restrict__ in_st,
                  uint32_t* __restrict__ dial_st, uint32_t* __restrict__ n_admitted, uint32_t* __restrict__ n_freed) {
    const uint32_t lane = threadIdx.x;
    const uint64_t lt = (1ull << lane) - 1;
    const CnTorrent T = tors[blockIdx.x];
    const uint64_t P = T.n_peers, W = (P + 63) >> 6;
    uint64_t* active = bits + T.bits_off;
    uint64_t* pending = active + W;
    int64_t* exp = expiry + T.peer_off;
    uint32_t cap = capacity[blockIdx.x];  // wave-uniform from here on

    // ---- phase 1: transitions
    uint32_t freed = 0;
    {
        const cn::Transition* list = trs + T.tr_at;
        uint32_t* st_out = tr_st + T.trans_off;
        for (uint64_t f0 = 0; f0 < T.n_trans; f0 += 64) {  // uniform
            const uint64_t f = f0 + lane;
            bool fr = false;
            if (f < T.n_trans) {
                const cn::Transition e = list[f];
                const uint64_t w = e.peer >> 6, b = 1ull << (e.peer & 63);
                uint64_t* row = cn::clears_active(e.kind) ? active : pending;
                const bool was = (ld(row + w) & b) != 0;  // this lane's bit alone: the list's peers are distinct
                if (was) clear_bit(row + w, b);
                if (was && e.kind == cn::kEstablished) set_bit(active + w, b);
                uint32_t st = cn::transition_status(e.kind, was);
                fr = (st & cn::kFreed) != 0;
                if (cn::blacklists(e.kind)) {
                    int64_t x = exp[e.peer];
                    const uint32_t add = cn::blacklist(&x, R);
                    if (add & cn::kBlacklistedNow) exp[e.peer] = x;
                    st |= add;
                }
                st_out[f] = st;
            }
            freed += (uint32_t)__popcll(__ballot(fr));
        }
        cap += freed;
    }
    phase_fence();

    // ---- phase 2: incoming handshakes, in list order
    uint32_t adm_in = 0;
    if (T.n_in) {  // uniform
        const cn::Incoming* list = ins + T.in_at;
        uint32_t* st_out = in_st + T.in_off;
        const bool own0 = lane < W;
        const uint64_t live0 = own0 ? cn::live_bits(P, lane) : 0;
        const uint64_t act0 = own0 ? ld(active + lane) : 0;
        uint64_t pend0 = own0 ? ld(pending + lane) : 0;
        const uint64_t pend_was = pend0;
        cn::Incoming e1 = list[0], e2 = e1;  // entries f + 1 and f + 2
        if (T.n_in > 1) e2 = list[1];
        uint64_t nb1 = 0;  // entry f + 1's neighbour word of this lane
        if (own0 && e1.neigh_off != cn::kNoRow) nb1 = neighbors[e1.neigh_off + lane];
        for (uint64_t f = 0; f < T.n_in; ++f) {  // uniform
            const cn::Incoming e = e1;
            const uint64_t nb = nb1;
            e1 = e2;
            if (f + 2 < T.n_in) e2 = list[f + 2];
            nb1 = 0;
            if (f + 1 < T.n_in && own0 && e1.neigh_off != cn::kNoRow) nb1 = neighbors[e1.neigh_off + lane];  // in flight
            const uint64_t w = e.peer >> 6, b = 1ull << (e.peer & 63);
            uint32_t st = cn::kAtCapacity;
            if (cap != 0) {  // uniform
                uint64_t pw, aw;
                if (w < 64) {  // uniform: e is
                    pw = __shfl((ull)pend0, (int)w);
                    aw = __shfl((ull)act0, (int)w);
                } else {  // the owning lane's word in memory, written by nobody else
                    uint64_t p_own = 0, a_own = 0;
                    if (lane == (w & 63)) p_own = pending[w], a_own = active[w];
                    pw = __shfl((ull)p_own, (int)(w & 63));
                    aw = __shfl((ull)a_own, (int)(w & 63));
                }
                uint64_t mutual = 0;
                if (!(pw & b) && !(aw & b) && e.neigh_off != cn::kNoRow) {  // uniform
                    uint32_t c = (uint32_t)__popcll(nb & (act0 | pend0) & live0);
                    for (uint64_t x0 = 64; x0 < W; x0 += 64) {  // uniform
                        const uint64_t x = x0 + lane;
                        if (x < W) c += (uint32_t)__popcll(neighbors[e.neigh_off + x] & (active[x] | pending[x]) & cn::live_bits(P, x));
                    }
                    mutual = wave_sum(c);
                }
                st = cn::add_pending_status(cap, (pw & b) != 0, (aw & b) != 0, mutual, R.max_mutual);
                if (!st) {
                    st = cn::kOk;
                    --cap;
                    ++adm_in;
                    if (lane == (w & 63)) {
                        if (w < 64) pend0 |= b;
                        else pending[w] = pw | b;
                    }
                }
            }
            if (lane == 0) st_out[f] = st;
        }
        if (own0 && pend0 != pend_was) pending[lane] = pend0;
    }
    phase_fence();

    // ---- phase 3: dials
    uint32_t adm_dial = 0;
    {
        const uint32_t* list = dials + T.dial_at;
        uint32_t* st_out = dial_st + T.dial_off;
        const bool complete = (T.flags & cn::kTorrentComplete) != 0;
        for (uint64_t d0 = 0; d0 < T.n_dial; d0 += 64) {  // uniform
            const uint64_t d = d0 + lane;
            const bool has = d < T.n_dial;
            if (complete) {  // uniform
                if (has) st_out[d] = cn::kTorrentIsComplete;
                continue;
            }
            const uint32_t p = has ? list[d] : cn::kNone;
            const uint64_t w = p >> 6, b = 1ull << (p & 63);
            uint32_t pre = 0;
            bool is_p = false, is_a = false;
            if (has) {
                pre = p == T.self_peer ? cn::kSelf : cn::blacklisted(exp[p], R.now) ? cn::kBlacklisted : 0;
                is_p = (ld(pending + w) & b) != 0;
                is_a = (ld(active + w) & b) != 0;
            }
            const bool reach = has && !pre;  // gets as far as AddPending
            const bool elig = reach && !is_p && !is_a;
            const uint64_t eb = __ballot(elig);
            bool dup = false;  // an earlier lane of this step holds the same peer and is eligible
            if (__popcll(eb) > 1)                    // uniform
                for (uint32_t j = 0; j < 63; ++j) {  // uniform
                    const uint32_t pj = (uint32_t)__builtin_amdgcn_readlane((int)p, (int)j);
                    dup |= j < lane && ((eb >> j) & 1) && pj == p;
                }
            const bool cont = elig && !dup;
            const uint64_t cb = __ballot(cont);
            const uint32_t rank = (uint32_t)__popcll(cb & lt), n_cont = (uint32_t)__popcll(cb);
            // the last lane that is not cut off: none when the capacity is 0, the contender that
            // takes the last slot when the step exhausts it, else every lane
            int32_t cut = 63;
            if (cap == 0) cut = -1;
            else if (n_cont >= cap) cut = (int32_t)__builtin_ctzll(__ballot(cont && rank == cap - 1));
            if (has) {
                uint32_t st;
                if (pre) st = pre;
                else if ((int32_t)lane > cut) st = cn::kAtCapacity;
                else if (is_p || dup) st = cn::kAlreadyPending;
                else if (is_a) st = cn::kAlreadyActive;
                else {
                    st = cn::kOk;
                    set_bit(pending + w, b);
                }
                st_out[d] = st;
            }
            const uint32_t took = n_cont < cap ? n_cont : cap;
            cap -= took;
            adm_dial += took;
            phase_fence();  // the next step's loads see this step's bits
        }
    }
    if (lane == 0) {
        capacity[blockIdx.x] = cap;
        n_admitted[2 * (uint64_t)blockIdx.x] = adm_in;
        n_admitted[2 * (uint64_t)blockIdx.x + 1] = adm_dial;
        n_freed[blockIdx.x] = freed;
    }
}

constexpr uint32_t kSweepWaves = 4;
constexpr uint32_t kSweepBlock = 64 * kSweepWaves;

// One workgroup a torrent: wave v takes words v, v + 4, ... of the active row, one lane a peer, one
// ballot and one 8-byte store a word.
__global__ void __launch_bounds__(kSweepBlock)
conn_preempt_kernel(const CnSweep* __restrict__ tors, const uint64_t* __restrict__ bits, const int64_t* __restrict__ created,
                    const int64_t* __restrict__ received, const int64_t* __restrict__ sent, int64_t now, int64_t tti,
                    int64_t ttl, uint64_t* __restrict__ close, uint32_t* __restrict__ n_close) {
    __shared__ uint32_t part[kSweepWaves];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const CnSweep T = tors[blockIdx.x];
    const uint64_t P = T.n_peers, W = (P + 63) >> 6;
    const uint64_t* active = bits + T.bits_off;
    uint32_t n = 0;  // uniform over the wave
    for (uint64_t w = wv; w < W; w += kSweepWaves) {  // uniform over the wave
        const uint64_t p = w * 64 + lane;
        bool out = false;
        if (p < P && ((active[w] >> lane) & 1)) {
            const uint64_t at = T.peer_off + p;
            out = cn::preempts(created[at], received[at], sent[at], now, tti, ttl);
        }
        const uint64_t word = __ballot(out);
        if (lane == 0) close[T.close_off + w] = word;
        n += (uint32_t)__popcll(word);
    }
    if (lane == 0) part[wv] = n;
    __syncthreads();
    if (threadIdx.x == 0) n_close[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

}  // namespace

hipError_t launch_conn_round(const CnTorrent* tors, uint64_t n_tors, const cn::Transition* tr, const cn::Incoming* in,
                             const uint32_t* dial, const uint64_t* neighbors, uint64_t* bits, int64_t* expiry,
                             uint32_t* capacity, const cn::Round& round, uint32_t* tr_st, uint32_t* in_st, uint32_t* dial_st,
                             uint32_t* n_admitted, uint32_t* n_freed, hipStream_t s) {
    if (!n_tors) return hipSuccess;
    if (n_tors > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const hipError_t pre = launch_precheck();
    if (pre != hipSuccess) return pre;
    t_launch_plan = 0;
    t_launch_units = n_tors;
    hipLaunchKernelGGL(conn_round_kernel, dim3((uint32_t)n_tors), dim3(64), 0, s, tors, tr, in, dial, neighbors, bits, expiry,
                       capacity, round, tr_st, in_st, dial_st, n_admitted, n_freed);
    return hipGetLastError();
}

hipError_t launch_conn_preempt(const CnSweep* tors, uint64_t n_tors, const uint64_t* bits, const int64_t* created,
                               const int64_t* received, const int64_t* sent, int64_t now, int64_t tti, int64_t ttl,
                               uint64_t* close, uint32_t* n_close, hipStream_t s) {
    if (!n_tors) return hipSuccess;
    if (n_tors > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const hipError_t pre = launch_precheck();
    if (pre != hipSuccess) return pre;
    t_launch_plan = 0;
    t_launch_units = n_tors;
    hipLaunchKernelGGL(conn_preempt_kernel, dim3((uint32_t)n_tors), dim3(kSweepBlock), 0, s, tors, bits, created, received,
                       sent, now, tti, ttl, close, n_close);
    return hipGetLastError();
}

}  // namespace krk
