// peer_round.hip -- one peer round for a batch of torrents: Dispatcher.AddPeer from the handshake's
// wire bytes, handleComplete, and the progress derived from the rows (remaining pieces, endgame,
// torrent complete, each slot's held and wanted counts and its close / notify action), as
// peer_round_math.hpp defines the round and bit for bit what it computes.
//
// One wave a row, nothing shared.  A unit is one row of one torrent -- `have`, or a slot's bits_p --
// and a workgroup of four waves takes four consecutive units; the unit's torrent is found by a
// search over the torrents' first units.  Beyond kPeUnitCap units the waves stride.
//   peer wave  finds its slot in the staged join and full lists (binary searches), decides
//              well-formedness from the span's length field and wire_len BEFORE any store, then
//              walks the row in lane-strided order, kPeLaneWords words a lane a step (a wave covers
//              256 words, 2 KiB of each array), every load of the step -- the row word, the `have`
//              word, the three aligned dwords around each wire word -- issued before the first use.
//              The new word is the old one, the decoded wire word or all ones, the last word
//              masked; a word that changed is stored once, coalesced.  popcount(word),
//              popcount(word & ~have) and popcount(have) accumulate in registers and are summed
//              over the wave by xor shuffles; lane 0 stores the slot's three outputs.
//   have wave  the same walk over `have` alone; lane 0 stores the torrent's two outputs.
// Every peer wave recomputes the torrent's remaining count from the `have` words it reads anyway
// (the re-reads hit L2), so no wave waits for another: no LDS, no barrier, no atomics.  A wire word
// lies at any byte: the dwords that hold it are read aligned, joined by v_alignbyte and byte-swapped
// (v_perm); a dword that the span covers only in part -- its first and its last -- is read byte by
// byte, so that nothing outside the span is touched.  Plain vector stores, one writer a word; all
// index arithmetic on the offsets is 64-bit.
#include "device_util.hpp"
#include "kernels.hpp"
#include "peer_round_math.hpp"

namespace krk {

namespace {

constexpr uint32_t kWaves = 4;
constexpr uint32_t kBlock = 64 * kWaves;
constexpr uint32_t kS = kPeLaneWords;
static_assert(kPeUnitCap % kWaves == 0, "whole workgroups under the cap");

// The torrent that owns unit u: the last one whose first unit is <= u (every torrent has one).
__device__ __forceinline__ uint64_t unit_owner(const PeTorrent* __restrict__ tors, uint64_t n_tors, uint64_t u) {
    uint64_t lo = 0, hi = n_tors;  // first_unit[lo] <= u < first_unit[hi]
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (tors[mid].first_unit <= u) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The three dwords that hold the eight bytes at `at` (any alignment) ...
__device__ __forceinline__ void wire_load(uint64_t at, uint64_t lo, uint64_t hi, uint32_t (&d)[3]) {
    const uint64_t a = at & ~uint64_t(3);
    d[0] = span_dword(a, lo, hi);
    d[1] = span_dword(a + 4, lo, hi);
    d[2] = at & 3 ? span_dword(a + 8, lo, hi) : 0;  // aligned: the word ends with the second
}
// ... and the big-endian uint64 they spell.
__device__ __forceinline__ uint64_t wire_word(uint64_t at, const uint32_t (&d)[3]) {
    const uint32_t sh = (uint32_t)at & 3;
    const uint32_t b0 = __builtin_amdgcn_alignbyte(d[1], d[0], sh), b1 = __builtin_amdgcn_alignbyte(d[2], d[1], sh);
    return (uint64_t)__builtin_bswap32(b0) << 32 | __builtin_bswap32(b1);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
    for (uint32_t m = 32; m; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

// The position of x in the ascending a[0, n), or n.
template <class T, class Key>
__device__ __forceinline__ uint32_t find(const T* __restrict__ a, uint32_t n, uint32_t x, Key key) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (key(a[mid]) < x) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && key(a[lo]) == x ? lo : n;
}

enum Mode : uint32_t { kKeep, kWire, kOnes };

__global__ void __launch_bounds__(kBlock)
peer_round_kernel(const PeTorrent* __restrict__ tors, uint64_t n_tors, uint64_t n_units,
                  const uint64_t* __restrict__ live_all, const pe::Join* __restrict__ joins_all,
                  const uint32_t* __restrict__ fulls_all, const uint8_t* __restrict__ wire, uint64_t* bits,
                  uint32_t* __restrict__ remaining_out, uint32_t* __restrict__ tflags_out, uint32_t* __restrict__ held_out,
                  uint32_t* __restrict__ wanted_out, uint32_t* __restrict__ status_out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint64_t u = (uint64_t)blockIdx.x * kWaves + wv; u < n_units; u += (uint64_t)gridDim.x * kWaves) {  // wave-uniform
        const uint64_t t = unit_owner(tors, n_tors, u);
        const PeTorrent T = tors[t];
        const uint64_t N = T.n_pieces, W = (N + 63) >> 6;
        const uint64_t* have = bits + T.bits_off;
        const uint64_t r = u - T.first_unit;  // 0: have; else slot r - 1
        if (r == 0) {
            uint32_t cnt = 0;
            for (uint64_t base = 0; base < W; base += 64 * kS) {
                uint64_t h[kS];
#pragma unroll
                for (uint32_t j = 0; j < kS; ++j) {
                    const uint64_t w = base + 64 * j + lane;
                    h[j] = w < W ? have[w] & pe::word_mask(N, w, W) : 0;
                }
#pragma unroll
                for (uint32_t j = 0; j < kS; ++j) cnt += (uint32_t)__popcll(h[j]);
            }
            cnt = wave_sum(cnt);
            if (lane == 0) {
                const uint64_t remaining = N - cnt;
                remaining_out[t] = (uint32_t)remaining;
                tflags_out[t] = pe::torrent_flags(remaining, T.threshold, T.flags);
            }
            continue;
        }
        const uint32_t p = (uint32_t)(r - 1);
        uint64_t* row = bits + T.bits_off + (1 + 2 * (uint64_t)p) * W;
        uint32_t status = 0;
        Mode mode = kKeep;
        uint64_t span_lo = 0, span_hi = 0;  // the join's span, as addresses
        const pe::Join* joins = joins_all + T.join_at;
        const uint32_t jk = find(joins, T.n_joins, p, [](const pe::Join& j) { return j.peer; });
        if (jk < T.n_joins) {
            const pe::Join J = joins[jk];
            span_lo = (uint64_t)wire + J.wire_off;
            span_hi = span_lo + J.wire_len;
            uint64_t length = 0;
            if (J.wire_len >= 8) {
                uint32_t d[3];
                wire_load(span_lo, span_lo, span_hi, d);
                length = wire_word(span_lo, d);
            }
            const bool ok = pe::wire_ok(J.wire_len, length, N);
            status = ok ? pe::kJoined : pe::kBadBitfield;
            if (ok) mode = kWire;
        }
        const uint32_t* fulls = fulls_all + T.full_at;
        if (find(fulls, T.n_fulls, p, [](uint32_t f) { return f; }) < T.n_fulls) {
            status |= pe::kSetFull;
            mode = kOnes;
        }
        uint32_t held = 0, wanted = 0, cnt = 0;
        for (uint64_t base = 0; base < W; base += 64 * kS) {  // wave-uniform
            uint64_t h[kS], old[kS];
            uint32_t d[kS][3];
#pragma unroll
            for (uint32_t j = 0; j < kS; ++j) {
                const uint64_t w = base + 64 * j + lane;
                const bool in = w < W;
                h[j] = in ? have[w] : 0;
                old[j] = in ? row[w] : 0;
                if (mode == kWire && in) wire_load(span_lo + 8 + 8 * w, span_lo, span_hi, d[j]);
                else d[j][0] = d[j][1] = d[j][2] = 0;
            }
#pragma unroll
            for (uint32_t j = 0; j < kS; ++j) {
                const uint64_t w = base + 64 * j + lane;
                if (w >= W) continue;
                const uint64_t m = pe::word_mask(N, w, W);
                uint64_t x = old[j];
                if (mode == kWire) x = wire_word(span_lo + 8 + 8 * w, d[j]) & m;
                else if (mode == kOnes) x = m;
                if (mode != kKeep && x != old[j]) row[w] = x;
                x &= m;
                held += (uint32_t)__popcll(x);
                wanted += (uint32_t)__popcll(x & ~h[j]);
                cnt += (uint32_t)__popcll(h[j] & m);
            }
        }
        held = wave_sum(held), wanted = wave_sum(wanted), cnt = wave_sum(cnt);
        if (lane == 0) {
            const uint64_t at = T.peer_off + p;
            const bool alive = (live_all[T.live_at + (p >> 6)] >> (p & 63)) & 1;
            held_out[at] = held;
            wanted_out[at] = wanted;
            status_out[at] = status | pe::peer_flags(alive, held, N, N - cnt);
        }
    }
}

}  // namespace

hipError_t launch_peer_round(const PeTorrent* tors, uint64_t n_tors, uint64_t n_units, const uint64_t* live,
                             const pe::Join* joins, const uint32_t* fulls, const uint8_t* wire, uint64_t* bits,
                             uint32_t* remaining, uint32_t* tflags, uint32_t* held, uint32_t* wanted, uint32_t* status,
                             hipStream_t s) {
    if (!n_tors) return hipSuccess;
    const hipError_t pre = launch_precheck();
    if (pre != hipSuccess) return pre;
    const uint64_t units = n_units < kPeUnitCap ? n_units : kPeUnitCap;
    t_launch_plan = 0;
    t_launch_units = n_units;
    hipLaunchKernelGGL(peer_round_kernel, dim3((uint32_t)((units + kWaves - 1) / kWaves)), dim3(kBlock), 0, s, tors, n_tors,
                       n_units, live, joins, fulls, wire, bits, remaining, tflags, held, wanted, status);
    return hipGetLastError();
}

}  // namespace krk
