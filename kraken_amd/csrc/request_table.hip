// request_table.hip -- one request table round for a batch of torrents: the piece request table
// (piecerequest.Manager's requests / requestsByPeer, piecerequest/manager.go) kept in device
// memory beside the rows of a request round, as request_table_math.hpp defines the round and bit
// for bit what it computes.
//
// One workgroup of four waves a torrent, the six steps in order:
//   rows     `arrived` into have and `holds` into bits_p as head-of-run read-modify-writes: both
//            lists ascend, so the elements that fall in one row word are adjacent, the first of a
//            run ORs the run together and is the word's one writer.  The `gone` rows are zeroed
//            between the two (a hold may land on a row just zeroed).
//   removal  a stable in-place compaction, kRtChunk = 256 entries a step in table order, one entry a
//            thread: its fate is a binary search of the staged `arrived` and `gone` lists, its new
//            position a ballot a wave plus a four-entry LDS prefix (block_rank).  The write index
//            never passes the read index, and a step's reads all precede its barrier, its writes
//            follow it.  The marks are applied on the way (the lists are short; a survivor scans them).
//   records  the explicit pairs land at their index; the picks of a request round are read where
//            they lie, 256 (peer, slot) pairs a step, ranked the same way.
//   derive   the table's keys staged in LDS (kRtTile = 4,096 keys of eight bytes, 32 KiB) and sorted
//            there, a bitonic network over the next power of two.  First (peer, piece) of the live
//            entries: a peer's quota is the length of its segment (two binary searches, one writer
//            a quota), and under allow-duplicates the entries of one blocked_p word are adjacent.
//            Then (piece, position) of all of them, the failed status in the low bits: without
//            duplicates the live entries of one row word are adjacent -- the head builds the word
//            once and stores it to every peer's row -- and the failed list is the entries that are
//            not live in sorted order, ranked like the compaction.  Every blocked row is zero-filled
//            with streaming stores first; after a barrier the heads store the words that are not zero.
// No atomics on global memory (the dropped count is an LDS counter), plain vector stores; all index
// arithmetic on the offsets is 64-bit; every trip count around a barrier is uniform over the
// workgroup.  An entry with a piece, peer or status out of range is dropped by the compaction, and
// a pick >= n_pieces is never recorded, so no row is indexed with a value the host did not check.
#include "device_util.hpp"
#include "kernels.hpp"
#include "request_table_math.hpp"

namespace krk {

namespace {

constexpr uint32_t kWaves = 4;
constexpr uint32_t kBlock = 64 * kWaves;
static_assert(kBlock == kRtChunk, "one entry a thread in a step");
static_assert((kRtTile & (kRtTile - 1)) == 0 && kRtTile >= kRtMaxEntries && kRtTile <= (1u << 12),
              "the tile is a power of two that holds a table, and a position fits 12 bits");
constexpr uint64_t kPad = ~0ull;  // sorts last: no entry has piece and peer 0xFFFFFFFF

// This thread's rank among the workgroup's set flags, and their number: one barrier.  The two
// buffers take turns, so the call after the next may write the one this call reads.
__device__ inline uint32_t block_rank(bool f, uint32_t (&wsum)[2][kWaves], uint32_t& par, uint32_t lane, uint32_t wv,
                                      uint32_t& total) {
    const uint64_t bal = __ballot(f);
    if (lane == 0) wsum[par][wv] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t v = 0; v < kWaves; ++v) {
        const uint32_t c = wsum[par][v];
        before += v < wv ? c : 0;
        all += c;
    }
    par ^= 1;
    total = all;
    return before + (uint32_t)__popcll(bal & ((1ull << lane) - 1));
}

__global__ void __launch_bounds__(kBlock)
request_table_kernel(const RtTorrent* __restrict__ tors, const uint32_t* __restrict__ arrived_all,
                     const uint32_t* __restrict__ gone_all, const rs::Failed* __restrict__ marks_all,
                     const rt::Pair* __restrict__ holds_all, const rt::Pair* __restrict__ records_all,
                     const uint32_t* __restrict__ picks_all, const uint32_t* __restrict__ n_picked_all, const rt::Round R,
                     uint64_t* bits, rt::Entry* entries, uint32_t* n_entries, int32_t* __restrict__ quota_all,
                     rs::Failed* __restrict__ failed_all, uint32_t* __restrict__ n_failed, uint32_t* __restrict__ n_dropped) {
    __shared__ uint64_t keys[kRtTile];
    __shared__ uint32_t wsum[2][kWaves];
    __shared__ uint32_t s_dropped;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const RtTorrent T = tors[blockIdx.x];
    const uint64_t N = T.n_pieces, W = (N + 63) >> 6, P = T.n_peers;
    const uint32_t cap = T.cap;
    const bool dup = (T.flags & pr::kAllowDuplicates) != 0;
    uint64_t* rows = bits + T.bits_off;
    rt::Entry* tab = entries + T.entry_off;
    const uint32_t* arrived = arrived_all + T.arrived_at;
    const uint32_t* gone = gone_all + T.gone_at;
    const rs::Failed* marks = marks_all + T.mark_at;
    const rt::Pair* holds = holds_all + T.hold_at;
    const rt::Pair* records = records_all + T.record_at;
    uint32_t par = 0, total = 0, dropped = 0;
    if (tid == 0) s_dropped = 0;

    // ---- rows: arrived into have, the gone rows zeroed, then the holds
    for (uint32_t k = tid; k < T.n_arrived; k += kBlock) {
        const uint32_t i = arrived[k];
        if (k && (arrived[k - 1] >> 6) == (i >> 6)) continue;  // not the head of its run
        uint64_t word = 1ull << (i & 63);
        for (uint32_t j = k + 1; j < T.n_arrived && (arrived[j] >> 6) == (i >> 6); ++j) word |= 1ull << (arrived[j] & 63);
        rows[i >> 6] |= word;
    }
    for (uint32_t g = 0; g < T.n_gone; ++g) {  // uniform
        uint64_t* row = rows + (1 + 2 * (uint64_t)gone[g]) * W;
        for (uint64_t w = tid; w < W; w += kBlock) row[w] = 0;
    }
    __syncthreads();
    for (uint32_t k = tid; k < T.n_holds; k += kBlock) {
        const rt::Pair h = holds[k];
        if (k && holds[k - 1].peer == h.peer && (holds[k - 1].piece >> 6) == (h.piece >> 6)) continue;
        uint64_t word = 1ull << (h.piece & 63);
        for (uint32_t j = k + 1; j < T.n_holds && holds[j].peer == h.peer && (holds[j].piece >> 6) == (h.piece >> 6); ++j)
            word |= 1ull << (holds[j].piece & 63);
        rows[(1 + 2 * (uint64_t)h.peer) * W + (h.piece >> 6)] |= word;
    }

    // ---- removal and marks: stable, in place
    const uint32_t n0 = n_entries[blockIdx.x], n = n0 < cap ? n0 : cap;
    uint32_t m = 0;  // the entries kept so far: the same in every thread
    for (uint32_t c = 0; c < n; c += kBlock) {  // uniform
        const uint32_t e = c + tid;
        rt::Entry x = {0, 0, 0, 0, 0};
        bool keep = false;
        if (e < n) {
            x = tab[e];
            keep = rt::entry_ok(x.piece, x.peer, x.status, N, T.n_peers) && !rt::contains(arrived, T.n_arrived, x.piece) &&
                   !rt::contains(gone, T.n_gone, x.peer);
            if (keep) x.status = rt::marked(marks, T.n_marks, x.piece, x.peer, x.status);
        }
        const uint32_t rank = block_rank(keep, wsum, par, lane, wv, total);
        if (keep) tab[m + rank] = x;  // m + rank <= e
        m += total;
    }

    // ---- records: the explicit pairs, then the picks where they lie
    for (uint32_t k = tid; k < T.n_records; k += kBlock) {
        const uint64_t pos = (uint64_t)m + k;
        if (pos < cap) tab[pos] = {records[k].piece, records[k].peer, rt::kPending, 0, R.now};
        else ++dropped;
    }
    m = (uint64_t)m + T.n_records < cap ? m + T.n_records : cap;
    if (picks_all) {
        const uint32_t* picks = picks_all + T.peer_off * R.limit;
        const uint32_t* n_picked = n_picked_all + T.peer_off;
        const uint64_t slots = P * R.limit;
        for (uint64_t c = 0; c < slots; c += kBlock) {  // uniform
            const uint64_t s = c + tid;
            uint32_t i = 0, p = 0;
            bool valid = false;
            if (s < slots) {
                p = (uint32_t)(s / R.limit);
                const uint32_t j = (uint32_t)(s - (uint64_t)p * R.limit), np = n_picked[p];
                if (j < (np < R.limit ? np : R.limit)) {
                    i = picks[s];
                    valid = i < N;
                    if (!valid) ++dropped;
                }
            }
            const uint32_t rank = block_rank(valid, wsum, par, lane, wv, total);
            if (valid) {
                if (m + rank < cap) tab[m + rank] = {i, p, rt::kPending, 0, R.now};
                else ++dropped;
            }
            m = m + total < cap ? m + total : cap;
        }
    }
    const uint32_t E = m;
    if (dropped) atomicAdd(&s_dropped, dropped);  // LDS
    __syncthreads();                              // the table is written; s_dropped is whole
    if (tid == 0) {
        n_entries[blockIdx.x] = E;
        n_dropped[blockIdx.x] = s_dropped;
    }

    // ---- derive: (peer, piece) of the live entries
    uint32_t n2 = 1;
    while (n2 < E) n2 <<= 1;
    for (uint32_t e = tid; e < n2; e += kBlock) {
        uint64_t key = kPad;
        if (e < E) {
            const rt::Entry x = tab[e];
            if (rt::live(R, x.status, x.sent_at)) key = (uint64_t)x.peer << 32 | x.piece;
        }
        keys[e] = key;
    }
    sort_keys<kBlock>(keys, n2, tid);
    int32_t* quota = quota_all + T.peer_off;
    for (uint64_t p = tid; p < P; p += kBlock) {
        const uint32_t cnt = lower_bound(keys, n2, (p + 1) << 32) - lower_bound(keys, n2, p << 32);
        quota[p] = cnt >= R.limit ? 0 : (int32_t)(R.limit - cnt);
    }
    if (W) {  // every blocked word zeroed: word x of the P * W is word w of peer p
        const uint64_t step_p = kBlock / W, step_w = kBlock % W;
        uint64_t p = tid / W, w = tid % W;
        while (p < P) {
            __builtin_nontemporal_store((uint64_t)0, rows + (2 + 2 * p) * W + w);
            p += step_p, w += step_w;
            if (w >= W) w -= W, ++p;
        }
    }
    // The heads' plain stores below hit words another thread has just zeroed.  What orders the two is
    // the barrier and the CU itself: the waves of a workgroup share one vector memory path, which keeps
    // stores to one address in issue order (the workgroup-scope fence of __syncthreads need not wait for
    // vmcnt outside tgsplit mode; this kernel is never built for it).  Non-temporal is a cache hint only.
    __syncthreads();
    if (dup) {
        const uint32_t L = lower_bound(keys, n2, kPad);  // the live entries
        for (uint32_t e = tid; e < L; e += kBlock) {
            const uint64_t key = keys[e];
            if (e && (keys[e - 1] >> 6) == (key >> 6)) continue;  // the same peer and word: not the head
            uint64_t word = 1ull << (key & 63);
            for (uint32_t j = e + 1; j < L && (keys[j] >> 6) == (key >> 6); ++j) word |= 1ull << (keys[j] & 63);
            rows[(2 + 2 * (key >> 32)) * W + ((uint32_t)key >> 6)] = word;
        }
    }
    if (dup && !failed_all) return;  // uniform

    // ---- derive: (piece, position) of every entry, the failed status below
    __syncthreads();  // the keys are read
    for (uint32_t e = tid; e < n2; e += kBlock) {
        uint64_t key = kPad;
        if (e < E) {
            const rt::Entry x = tab[e];
            const uint32_t st = rt::live(R, x.status, x.sent_at) ? 0 : rt::failed_status(x.status);
            key = (uint64_t)x.piece << 32 | e << 4 | st;
        }
        keys[e] = key;
    }
    sort_keys<kBlock>(keys, n2, tid);
    if (!dup) {
        for (uint32_t e = tid; e < E; e += kBlock) {
            const uint64_t key = keys[e], wi = key >> 38;
            if (e && (keys[e - 1] >> 38) == wi) continue;  // the same word: not the head
            uint64_t word = 0;
            for (uint32_t j = e; j < E && (keys[j] >> 38) == wi; ++j)
                if (!(keys[j] & 15)) word |= 1ull << ((keys[j] >> 32) & 63);
            if (word)  // built once, stored a peer: P stores on the head's lane (fine at the reference's 10 peers)
                for (uint64_t p = 0; p < P; ++p) rows[(2 + 2 * p) * W + wi] = word;
        }
    }
    if (!failed_all) return;  // uniform
    rs::Failed* failed = failed_all + T.entry_off;
    uint32_t nf = 0;
    for (uint32_t c = 0; c < E; c += kBlock) {  // uniform
        const uint32_t e = c + tid;
        const uint64_t key = e < E ? keys[e] : 0;
        const bool f = (key & 15) != 0;
        const uint32_t rank = block_rank(f, wsum, par, lane, wv, total);
        if (f) failed[nf + rank] = {(uint32_t)(key >> 32), tab[(key >> 4) & 0xFFF].peer, (uint32_t)(key & 15)};
        nf += total;
    }
    if (tid == 0) n_failed[blockIdx.x] = nf;
}

}  // namespace

hipError_t launch_request_table(const RtTorrent* tors, uint64_t n_tors, const uint32_t* arrived, const uint32_t* gone,
                                const rs::Failed* marks, const rt::Pair* holds, const rt::Pair* records,
                                const uint32_t* picks, const uint32_t* n_picked, const rt::Round& round, uint64_t* bits,
                                rt::Entry* entries, uint32_t* n_entries, int32_t* quota, rs::Failed* failed,
                                uint32_t* n_failed, uint32_t* n_dropped, hipStream_t s) {
    if (!n_tors) return hipSuccess;
    if (n_tors > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const hipError_t pre = launch_precheck();
    if (pre != hipSuccess) return pre;
    t_launch_plan = 0;
    t_launch_units = n_tors;
    hipLaunchKernelGGL(request_table_kernel, dim3((uint32_t)n_tors), dim3(kBlock), 0, s, tors, arrived, gone, marks, holds,
                       records, picks, n_picked, round, bits, entries, n_entries, quota, failed, n_failed, n_dropped);
    return hipGetLastError();
}

}  // namespace krk
