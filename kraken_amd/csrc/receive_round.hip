// receive_round.hip -- one receive round for a batch of torrents: every queued PiecePayloadMessage
// of a torrent judged against its resident `have` row and the MetaInfo's sums
// (Dispatcher.handlePiecePayload with Torrent.WritePiece), as receive_round_math.hpp defines the
// round and bit for bit what it computes.  Unlike a serve round, a payload's status depends on the
// payloads before it through the piece they share: the first full-shaped, good-summed payload of a
// piece not held writes it, the full-shaped ones before it are bad sums, those after it duplicates.
// errWritePieceConflict cannot arise: a round is one instant and its writes are serial.
//
// One workgroup of four waves a torrent, six steps in order:
//   count     the row's popcount before the round, strided, a wave reduction; n_complete after the
//             round is that plus the arrived pieces, so the row is never read back after a store.
//   classify  in arrival order, kRvChunk = 256 payloads a step, one payload a thread, loaded as one
//             16-byte load.  The `have` word, the payload's sum and the expected sum are issued
//             together; the shape status is computed in registers.  A payload that is full-shaped,
//             good-summed and not held drops the key  index << 12 | r  into an LDS tile of kRvTile
//             = 4,096 keys (32 KiB), every other one the pad; a provisional class (a byte) and the
//             sender (a word) a payload stay in LDS.
//   sort      one bitonic network in LDS (device_util.hpp).  The head of a piece run is that
//             piece's OK payload.
//   winners   a ballot scan over the run heads, wave totals through LDS (double buffered: one
//             barrier a step), compacts arrived_out / arrived_from_out: ascending by construction.
//             The head of a `have`-word run ORs its run's bits and does that word's one
//             read-modify-write.
//   resolve   in arrival order: a full-shaped, not-held payload does a lower_bound on index << 12
//             and reads the winner's arrival index w -- r == w OK, r > w DUPLICATE, else BAD_SUM.
//             Statuses and file offsets are stored coalesced; the mark predicate is scanned the
//             same way and marks_out compacted in arrival order.
//   counts    the tile refilled with  peer << 2 | (DUPLICATE)  for the OK and DUPLICATE payloads of
//             known senders and sorted again; one thread a slot, strided, takes n_good and
//             n_duplicate by three binary searches and stores `received` where n_good > 0.
//             Thread 0 stores the torrent's five totals.
// Plain vector stores, one writer a word; no atomics; all offset arithmetic is 64-bit; every trip
// count around a barrier is uniform over the workgroup.  The host checked every peer < n_peers or
// kNone and n_pays <= kRvTile; a row is indexed only by an index the kernel itself found inside
// [0, n_pieces).  LDS: 32 + 16 + 4 KiB and three small arrays.
#include "device_util.hpp"
#include "kernels.hpp"
#include "receive_round_math.hpp"

namespace krk {

namespace {

constexpr uint32_t kWaves = 4;
constexpr uint32_t kBlock = 64 * kWaves;
static_assert(kBlock == kRvChunk, "one payload a thread in a step");
static_assert((kRvTile & (kRvTile - 1)) == 0 && kRvTile >= rv::kMaxPayloads && kRvTile == 1u << 12,
              "the tile is a power of two that holds a list, and an arrival index is 12 bits of a key");
static_assert(sizeof(sv::Request) == 16, "one 16-byte load a payload");
constexpr uint64_t kPad = ~0ull;  // sorts last: an index is below 2^32, a slot below 2^30
// The provisional classes of a full-shaped payload (a shape status otherwise): held when the round
// began, a bad sum, or a candidate for its piece's OK.
constexpr uint32_t kHeld = rv::kDuplicate, kBad = rv::kBadSum, kCand = 5;

// The exclusive position of this thread among the workgroup's threads with `flag`, and *all, their
// count: a ballot inside the wave, the wave totals through cnt (one barrier).
__device__ __forceinline__ uint32_t block_rank(bool flag, uint32_t* cnt, uint32_t wv, uint32_t lane, uint32_t* all) {
    const uint64_t bal = __ballot(flag);
    if (lane == 0) cnt[wv] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t before = 0, sum = 0;
#pragma unroll
    for (uint32_t v = 0; v < kWaves; ++v) {
        const uint32_t k = cnt[v];
        sum += k;
        if (v < wv) before += k;
    }
    *all = sum;
    return before + (uint32_t)__popcll(bal & ((1ull << lane) - 1));
}

__global__ void __launch_bounds__(kBlock)
receive_round_kernel(const RvTorrent* __restrict__ tors, const sv::Request* __restrict__ pays_all, const int64_t now,
                     const RvArrays A) {
    __shared__ uint64_t keys[kRvTile];
    __shared__ uint32_t peers[kRvTile];
    __shared__ uint8_t cls[kRvTile];
    __shared__ uint32_t cnt[2][kWaves];
    __shared__ uint32_t held[kWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const RvTorrent T = tors[blockIdx.x];
    const uint64_t N = T.n_pieces, W = (N + 63) >> 6, P = T.n_peers;
    const uint32_t n = T.n_pays < kRvTile ? T.n_pays : kRvTile;
    uint64_t* have = A.bits + T.bits_off;
    const u32x4* pays = reinterpret_cast<const u32x4*>(pays_all + T.pay_at);
    const uint32_t* sums = A.sums + T.pay_off;
    const uint32_t* expected = A.expected + T.sum_off;

    // ---- count: the pieces held before the round
    uint32_t mine = 0;
    for (uint64_t w = tid; w < W; w += kBlock) mine += (uint32_t)__popcll(have[w] & pe::word_mask(N, w, W));
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if (lane == 0) held[wv] = mine;  // read by thread 0 after the barriers below

    // ---- classify, in arrival order
    for (uint32_t c = 0; c < n; c += kBlock) {
        const uint32_t r = c + tid;
        if (r >= n) continue;  // no barrier in this loop
        const u32x4 raw = pays[r];
        const sv::Request q = {raw.x, (int32_t)raw.y, (int32_t)raw.z, (int32_t)raw.w};
        uint32_t k = rv::shape(q, N, T.length, T.piece_length);
        if (k == rv::kOk) {  // index inside [0, N)
            const uint64_t hw = have[(uint32_t)q.index >> 6];
            const uint32_t got = sums[r], want = expected[(uint32_t)q.index];
            k = (hw >> (q.index & 63)) & 1 ? kHeld : got != want ? kBad : kCand;
        }
        cls[r] = (uint8_t)k;
        peers[r] = q.peer;
        keys[r] = k == kCand ? (uint64_t)(uint32_t)q.index << 12 | r : kPad;
    }
    uint32_t n2 = 1;
    while (n2 < n) n2 <<= 1;
    for (uint32_t e = n + tid; e < n2; e += kBlock) keys[e] = kPad;

    // ---- sort: (piece, arrival)
    sort_keys<kBlock>(keys, n2, tid);

    // ---- winners: the head of a piece run arrives, the head of a word run writes the word
    uint32_t n_arrived = 0, par = 0;       // the same in every thread
    for (uint32_t c = 0; c < n; c += kBlock, par ^= 1) {  // uniform
        const uint32_t e = c + tid;
        const uint64_t key = e < n ? keys[e] : kPad;
        const uint64_t prev = e && e < n ? keys[e - 1] : kPad;  // the pad when there is none: no piece, no word
        const bool head = key != kPad && (prev >> 12) != (key >> 12);
        uint32_t all;
        const uint32_t pos = n_arrived + block_rank(head, cnt[par], wv, lane, &all);
        if (head) {
            A.arrived[T.pay_off + pos] = (uint32_t)(key >> 12);
            A.arrived_from[T.pay_off + pos] = peers[key & (kRvTile - 1)];
            if ((prev >> 18) != (key >> 18)) {
                uint64_t word = 1ull << ((key >> 12) & 63);
                for (uint32_t j = e + 1; j < n && (keys[j] >> 18) == (key >> 18); ++j) word |= 1ull << ((keys[j] >> 12) & 63);
                have[key >> 18] |= word;  // key >> 18 < W: the index is inside [0, N)
            }
        }
        n_arrived += all;
    }
    __syncthreads();  // cnt is reused below

    // ---- resolve, in arrival order
    uint32_t n_marks = 0;
    par = 0;
    for (uint32_t c = 0; c < n; c += kBlock, par ^= 1) {  // uniform
        const uint32_t r = c + tid;
        const bool in = r < n;
        u32x4 raw = {0, 0, 0, 0};
        if (in) raw = pays[r];
        const sv::Request q = {raw.x, (int32_t)raw.y, (int32_t)raw.z, (int32_t)raw.w};
        uint32_t st = in ? cls[r] : rv::kIndex;
        if (st == kBad || st == kCand) {
            const uint32_t at = lower_bound(keys, n2, (uint64_t)(uint32_t)q.index << 12);
            const uint64_t k = at < n2 ? keys[at] : kPad;  // the pad's piece is no index
            st = rv::resolve(r, (k >> 12) == (uint32_t)q.index, (uint32_t)k & (kRvTile - 1));
        }
        const bool mk = in && rv::marks(st, q, N);
        uint32_t all;
        const uint32_t pos = n_marks + block_rank(mk, cnt[par], wv, lane, &all);
        if (in) {
            A.status[T.pay_off + r] = st;
            A.file_off[T.pay_off + r] = st == rv::kOk ? T.piece_length * (int64_t)q.index : 0;
            cls[r] = (uint8_t)st;
        }
        if (mk) A.marks[T.pay_off + pos] = {(uint32_t)q.index, q.peer, rv::kInvalid};
        n_marks += all;
    }
    __syncthreads();  // every search of the piece keys is done

    // ---- counts: (slot, duplicate) of the good and duplicate payloads; keys[n, n2) still hold the pad
    for (uint32_t r = tid; r < n; r += kBlock) {
        const uint32_t st = cls[r], p = peers[r];
        keys[r] = (st == rv::kOk || st == rv::kDuplicate) && p != rv::kNone ? (uint64_t)p << 2 | (st == rv::kDuplicate) : kPad;
    }
    sort_keys<kBlock>(keys, n2, tid);
    for (uint64_t p = tid; p < P; p += kBlock) {
        const uint32_t lo = lower_bound(keys, n2, p << 2), mid = lower_bound(keys, n2, p << 2 | 1),
                       hi = lower_bound(keys, n2, (p + 1) << 2);
        A.n_good[T.peer_off + p] = mid - lo;
        A.n_duplicate[T.peer_off + p] = hi - mid;
        if (mid > lo) A.received[T.peer_off + p] = now;
    }
    if (tid == 0) {
        uint64_t before = 0;
#pragma unroll
        for (uint32_t v = 0; v < kWaves; ++v) before += held[v];
        const uint64_t after = before + n_arrived;
        A.n_arrived[blockIdx.x] = n_arrived;
        A.n_marks[blockIdx.x] = n_marks;
        A.n_complete[blockIdx.x] = (uint32_t)after;
        A.bytes[blockIdx.x] = hv::bytes_downloaded(after, T.piece_length, T.length);
        A.flags[blockIdx.x] = rv::flags(before, after, N);
    }
}

}  // namespace

hipError_t launch_receive_round(const RvTorrent* tors, uint64_t n_tors, const sv::Request* pays, int64_t now, const RvArrays& a,
                                hipStream_t s) {
    if (!n_tors) return hipSuccess;
    if (n_tors > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const hipError_t pre = launch_precheck();
    if (pre != hipSuccess) return pre;
    t_launch_plan = 0;
    t_launch_units = n_tors;
    hipLaunchKernelGGL(receive_round_kernel, dim3((uint32_t)n_tors), dim3(kBlock), 0, s, tors, pays, now, a);
    return hipGetLastError();
}

}  // namespace krk
