// serve_round.hip -- one serve round for a batch of torrents: every queued PieceRequestMessage of a
// torrent answered against its resident rows (Dispatcher.handlePieceRequest), as
// serve_round_math.hpp defines the round and bit for bit what it computes.
//
// One workgroup of four waves a torrent, four steps in order:
//   classify  in arrival order, kSvChunk = 256 requests a step, one request a thread, loaded as one
//   and scan  16-byte load.  The `have` word and the live word are issued before the first use; the
//             status, file offset and length are computed in registers.  The pair (bytes, tokens) is
//             scanned as two 64-bit inclusive scans -- __shfl_up steps inside the wave, the four wave
//             totals through LDS (double buffered: one barrier a step) -- and the carry between steps
//             is uniform in registers.  A thread stores its five per-request outputs, coalesced, and
//             drops the key  peer << 33 | (status != OK) << 32 | (uint32)index  into an LDS tile of
//             kSvTile = 4,096 keys (32 KiB); the slots up to the next power of two get all-ones.
//   sort      one bitonic network in LDS (device_util.hpp, as request_table.hip sorts its keys).
//             After it a slot's requests are one segment, its OK requests the front of the segment
//             ascending by piece, repeats adjacent.
//   rows      a thread whose key is OK and is the first of its (peer, word) run ORs the run's bits:
//             it does that word's one read-modify-write and stores only if the word changes.
//   counts    one thread a slot, strided: three binary searches of the sorted tile give the slot's
//             received and sent counts; both are stored for every slot, `sent` only where something
//             was sent.  Thread 0 stores the torrent's totals from the scan's carry.
// Plain vector stores, one writer a word; no atomics; all offset arithmetic is 64-bit; every trip
// count around a barrier is uniform over the workgroup.  The host checked every peer < n_peers and
// n_reqs <= kSvTile; a row is indexed only by an index the kernel itself found inside [0, n_pieces).
#include "device_util.hpp"
#include "kernels.hpp"
#include "serve_round_math.hpp"

namespace krk {

namespace {

constexpr uint32_t kWaves = 4;
constexpr uint32_t kBlock = 64 * kWaves;
static_assert(kBlock == kSvChunk, "one request a thread in a step");
static_assert((kSvTile & (kSvTile - 1)) == 0 && kSvTile >= sv::kMaxRequests, "the tile is a power of two that holds a list");
static_assert(sizeof(sv::Request) == 16, "one 16-byte load a request");
constexpr uint64_t kPad = ~0ull;  // sorts last: a slot is below 2^30

// The inclusive sum of x over the lanes of the wave up to this one.
__device__ __forceinline__ uint64_t wave_scan(uint64_t x, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint64_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

__global__ void __launch_bounds__(kBlock)
serve_round_kernel(const SvTorrent* __restrict__ tors, const sv::Request* __restrict__ reqs_all,
                   const uint64_t* __restrict__ live_all, const int64_t now, const uint64_t token_size, const SvArrays A) {
    __shared__ uint64_t keys[kSvTile];
    __shared__ uint64_t tot[2][kWaves][2];  // a step's wave totals: bytes, tokens
    __shared__ uint32_t oks[2][kWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const SvTorrent T = tors[blockIdx.x];
    const uint64_t N = T.n_pieces, W = (N + 63) >> 6, P = T.n_peers;
    const uint32_t n = T.n_reqs < kSvTile ? T.n_reqs : kSvTile;
    uint64_t* rows = A.bits + T.bits_off;
    const u32x4* reqs = reinterpret_cast<const u32x4*>(reqs_all + T.req_at);
    const uint64_t* live = live_all + T.live_at;

    // ---- classify and scan, in arrival order
    uint64_t c_bytes = 0, c_tokens = 0;  // the carry: the same in every thread
    uint32_t c_ok = 0, par = 0;
    for (uint32_t c = 0; c < n; c += kBlock, par ^= 1) {  // uniform
        const uint32_t r = c + tid;
        const bool in = r < n;
        u32x4 raw = {0, 0, 0, 0};
        if (in) raw = reqs[r];
        const sv::Request q = {raw.x, (int32_t)raw.y, (int32_t)raw.z, (int32_t)raw.w};
        const uint32_t shape = in ? sv::shape_status(q, N, T.length, T.piece_length) : sv::kChunk;
        const uint64_t hw = in && !shape ? rows[(uint32_t)q.index >> 6] : 0;  // index inside [0, N)
        const uint64_t lw = in ? live[q.peer >> 6] : 0;                        // peer < n_peers
        const uint32_t st = sv::status(shape, (hw >> (q.index & 63)) & 1, (lw >> (q.peer & 63)) & 1);
        const bool ok = in && st == sv::kOk;
        const uint32_t len = ok ? (uint32_t)q.length : 0;
        const uint64_t tk = ok && token_size ? sv::tokens(len, token_size) : 0;
        const uint64_t ib = wave_scan(len, lane), it = wave_scan(tk, lane);
        const uint64_t bal = __ballot(ok);
        if (lane == 63) tot[par][wv][0] = ib, tot[par][wv][1] = it;
        if (lane == 0) oks[par][wv] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint64_t b_before = 0, b_all = 0, t_before = 0, t_all = 0;
        uint32_t ok_all = 0;
#pragma unroll
        for (uint32_t v = 0; v < kWaves; ++v) {
            const uint64_t b = tot[par][v][0], t = tot[par][v][1];
            b_all += b, t_all += t, ok_all += oks[par][v];
            if (v < wv) b_before += b, t_before += t;
        }
        if (in) {
            const uint64_t at = T.req_off + r;
            A.status[at] = st;
            A.file_off[at] = ok ? T.piece_length * (int64_t)q.index : 0;
            A.len[at] = len;
            A.send_off[at] = ok ? c_bytes + b_before + ib - len : 0;
            if (token_size) A.token_off[at] = ok ? c_tokens + t_before + it - tk : 0;
            keys[r] = (uint64_t)q.peer << 33 | (uint64_t)(st != sv::kOk) << 32 | (uint32_t)q.index;
        }
        c_bytes += b_all, c_tokens += t_all, c_ok += ok_all;
    }
    uint32_t n2 = 1;
    while (n2 < n) n2 <<= 1;
    for (uint32_t e = n + tid; e < n2; e += kBlock) keys[e] = kPad;

    // ---- sort: (peer, refused, piece)
    sort_keys<kBlock>(keys, n2, tid);

    // ---- rows: the head of a (peer, word) run of OK keys is the word's one writer
    for (uint32_t e = tid; e < n; e += kBlock) {
        const uint64_t key = keys[e];
        if (key >> 32 & 1) continue;                          // refused, or the pad
        if (e && (keys[e - 1] >> 6) == (key >> 6)) continue;  // the same peer, OK and word: not the head
        uint64_t word = 1ull << (key & 63);
        for (uint32_t j = e + 1; j < n && (keys[j] >> 6) == (key >> 6); ++j) word |= 1ull << (keys[j] & 63);
        uint64_t* at = rows + (1 + 2 * (key >> 33)) * W + ((uint32_t)key >> 6);
        const uint64_t old = *at;
        if ((old | word) != old) *at = old | word;
    }

    // ---- counts: a slot's segment, and the OK front of it
    for (uint64_t p = tid; p < P; p += kBlock) {
        const uint32_t lo = lower_bound(keys, n2, p << 33), mid = lower_bound(keys, n2, p << 33 | 1ull << 32),
                       hi = lower_bound(keys, n2, (p + 1) << 33);
        A.n_received[T.peer_off + p] = hi - lo;
        A.n_sent[T.peer_off + p] = mid - lo;
        if (mid > lo) A.sent[T.peer_off + p] = now;
    }
    if (tid == 0) {
        A.n_ok[blockIdx.x] = c_ok;
        A.bytes[blockIdx.x] = c_bytes;
        if (token_size) A.tokens[blockIdx.x] = c_tokens;
    }
}

}  // namespace

hipError_t launch_serve_round(const SvTorrent* tors, uint64_t n_tors, const sv::Request* reqs, const uint64_t* live,
                              int64_t now, uint64_t token_size, const SvArrays& a, hipStream_t s) {
    if (!n_tors) return hipSuccess;
    if (n_tors > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const hipError_t pre = launch_precheck();
    if (pre != hipSuccess) return pre;
    t_launch_plan = 0;
    t_launch_units = n_tors;
    hipLaunchKernelGGL(serve_round_kernel, dim3((uint32_t)n_tors), dim3(kBlock), 0, s, tors, reqs, live, now, token_size, a);
    return hipGetLastError();
}

}  // namespace krk
