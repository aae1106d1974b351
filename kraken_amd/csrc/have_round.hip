// have_round.hip -- one have round for a batch of torrents: the torrent's own row restored from
// the piece status sidecar (or the cache), merged with a verify result, and emitted as sidecar
// bytes, as the handshake's wire bitfield and as the missing list, as have_round_math.hpp defines
// the round and bit for bit what it computes.
//
// One workgroup of four waves a torrent; beyond kHvUnitCap torrents the workgroups stride.  The
// row is walked in passes of kHvPassWords = 256 words, one word a lane, wave v on the contiguous
// words [64v, 64v + 64) of the pass, so that list order needs only the four wave totals.
//   restore   a word is 64 sidecar bytes: the 16 (17 when misaligned) aligned dwords that cover
//             them, all loaded before the first use -- one unconditional run when the span covers
//             them all, byte loads for the dwords the span covers in part -- joined by v_alignbyte.
//             A dword's four bytes are compared at once (the carry-free zero-byte test on
//             x ^ 0x01010101) and the four result bits gathered by one multiply: 6 VALU a dword,
//             against a ballot a byte for the byte-a-lane form.  Bytes above 1 are counted the
//             same way.
//   lists     popcount(changed) and popcount(have) a lane, packed 16 + 16 bits (a pass holds at
//             most 16,384 of either), one in-wave inclusive scan by shuffles, the four wave totals
//             through LDS (double buffered: one barrier a pass), the running bases wave-uniform.
//             A lane stores its indices by find-first-set at base + prefix, cut at the cap; the
//             missing list's prefix is 64 w - the complete prefix, every earlier word being full.
//   emits     status: four bits become a dword by one multiply and a mask, 16 dwords a word; wire:
//             two byte-swapped dwords a word.  Either stream lands at any byte: a lane's aligned
//             dword k is v_alignbyte of its dwords k - 1 and k, dword 0 taking the neighbour lane's
//             last dword by a shuffle.  A dword of which a lane knows only a part -- the span's
//             first and last, and the one two waves share -- is written byte by byte, each byte by
//             the lane that owns it: spans of different torrents may abut inside a dword.
// Plain vector stores, one writer a byte; no atomics; all offset arithmetic is 64-bit.
#include "device_util.hpp"
#include "have_round_math.hpp"
#include "kernels.hpp"

namespace krk {

namespace {

constexpr uint32_t kWaves = 4;
constexpr uint32_t kBlock = 64 * kWaves;
static_assert(kBlock == kHvPassWords, "one word a lane");

// 0x80 in every byte of y that is not zero (no carry crosses a byte).
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t y) {
    return (((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y) & 0x80808080u;
}
// Bit k = (byte k of x == 1): the four flags sit at bits 0, 8, 16, 24 and the multiply gathers
// flag i at bit 21 + i (8 i + 7 j is distinct for all sixteen partial products).
__device__ __forceinline__ uint32_t ones4(uint32_t x) {
    const uint32_t eq = (nonzero_bytes(x ^ 0x01010101u) ^ 0x80808080u) >> 7;
    return (eq * 0x00204081u >> 21) & 0xF;
}
// The inverse: byte k = bit k of nib (bit i lands at i + 7 j, byte k's low bit is i = j = k).
__device__ __forceinline__ uint32_t bytes4(uint32_t nib) { return nib * 0x00204081u & 0x01010101u; }

// The word of the 64 sidecar bytes at `at` inside the span [lo, hi); bytes past hi read 0.
__device__ __forceinline__ uint64_t restore_word(uint64_t at, uint64_t lo, uint64_t hi, uint32_t& unexpected) {
    const uint64_t a = at & ~uint64_t(3);
    const uint32_t sh = (uint32_t)at & 3;
    uint32_t d[17];
    if (a >= lo && a + (sh ? 68 : 64) <= hi) {
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) d[k] = *as_global<uint32_t>(a + 4 * k);
        d[16] = sh ? *as_global<uint32_t>(a + 64) : 0;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 17; ++k) d[k] = span_dword(a + 4 * k, lo, hi);
    }
    uint64_t word = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        const uint32_t x = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
        word |= (uint64_t)ones4(x) << (4 * k);
        unexpected += (uint32_t)__popc(nonzero_bytes(x & 0xFEFEFEFEu));
    }
    return word;
}

// The bytes of the aligned dword at a that `known` names (bit k = byte k) and that lie below hi:
// one dword store when that is all four, else a store a byte.
__device__ __forceinline__ void span_store(uint64_t a, uint32_t v, uint32_t known, uint64_t hi) {
    if (a + 4 > hi) known &= a >= hi ? 0u : (1u << (uint32_t)(hi - a)) - 1;
    if (known == 0xF) {
        *reinterpret_cast<uint32_t*>(a) = v;
        return;
    }
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k)
        if (known >> k & 1) *reinterpret_cast<uint8_t*>(a + k) = (uint8_t)(v >> (8 * k));
}
// A lane's K dwords e, in memory order, to the byte address `at` of a span that ends at hi.  prev
// is the dword before e[0] when the lane knows it (has_prev); the dword after e[K - 1] belongs to
// the next lane when has_next.
template <uint32_t K>
__device__ __forceinline__ void emit_stream(uint64_t at, const uint32_t (&e)[K], uint32_t prev, bool has_prev, bool has_next,
                                            uint64_t hi) {
    const uint64_t a = at & ~uint64_t(3);
    const uint32_t sh = (uint32_t)at & 3;
    if (!sh) {
#pragma unroll
        for (uint32_t k = 0; k < K; ++k) span_store(a + 4 * k, e[k], 0xF, hi);
        return;
    }
    const uint32_t s = 4 - sh;  // byte j of a dword is stream byte j - sh
    span_store(a, __builtin_amdgcn_alignbyte(e[0], prev, s), has_prev ? 0xFu : 0xFu << sh & 0xFu, hi);
#pragma unroll
    for (uint32_t k = 1; k < K; ++k) span_store(a + 4 * k, __builtin_amdgcn_alignbyte(e[k], e[k - 1], s), 0xF, hi);
    if (!has_next) span_store(a + 4 * K, __builtin_amdgcn_alignbyte(0u, e[K - 1], s), (1u << sh) - 1, hi);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
    for (uint32_t m = 32; m; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

// The set bits of x, word w, to list[pos ..], ascending, cut at cap.
__device__ __forceinline__ void store_indices(uint32_t* list, uint64_t pos, uint64_t cap, uint64_t x, uint64_t w) {
    for (; x && pos < cap; x &= x - 1, ++pos) list[pos] = (uint32_t)(64 * w + (uint64_t)__builtin_ctzll(x));
}

__global__ void __launch_bounds__(kBlock) have_round_kernel(const HvTorrent* __restrict__ tors, uint64_t n_tors, HvArrays A) {
    __shared__ uint32_t tot[2][kWaves];  // a pass's wave totals, packed
    __shared__ uint32_t fin[kWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (uint64_t t = blockIdx.x; t < n_tors; t += gridDim.x) {  // workgroup-uniform
        const HvTorrent T = tors[t];
        const uint64_t N = T.n_pieces, W = (N + 63) >> 6;
        const uint32_t flags = T.flags;
        const bool bad = (flags & hv::kRestore) && T.status_len != N;
        const bool restore = (flags & hv::kRestore) && !bad, merge = flags & (hv::kMergeOr | hv::kMergeAnd);
        uint64_t* have = A.bits + T.bits_off;
        const uint64_t* ok = A.ok + T.ok_off;
        const uint64_t st_lo = (uint64_t)A.sidecar + T.status_off, st_hi = st_lo + N;
        const uint64_t so_lo = (uint64_t)A.status_out + T.status_out_off, so_hi = so_lo + N;
        const uint64_t wo_lo = (uint64_t)A.wire_out + T.wire_out_off, wo_hi = wo_lo + 8 + 8 * W;
        if ((flags & hv::kEmitWire) && tid == 0) {  // the length field; word 0's lane writes the dword they share
            const uint32_t h[2] = {0, __builtin_bswap32((uint32_t)N)};
            emit_stream<2>(wo_lo, h, 0, false, W != 0, wo_hi);
        }
        uint32_t unexpected = 0, n_changed = 0, n_complete = 0, par = 0;
        for (uint64_t p0 = 0; p0 < W; p0 += kBlock, par ^= 1) {
            const uint64_t w = p0 + tid;
            const bool in = w < W;
            const uint64_t m = in ? pe::word_mask(N, w, W) : 0;
            const uint64_t old = in ? have[w] : 0;
            const uint64_t okw = in && merge ? ok[w] : 0;
            const uint64_t st = in && restore ? restore_word(st_lo + 64 * w, st_lo, st_hi, unexpected) : 0;
            uint64_t now, changed;
            hv::word_round(flags, bad, old, st, okw, m, &now, &changed);
            if (in && now != old) have[w] = now;
            const uint64_t nm = now & m;
            const uint32_t c = (uint32_t)__popcll(changed) | (uint32_t)__popcll(nm) << 16;
            uint32_t incl = c;
#pragma unroll
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const uint32_t y = __shfl_up(incl, d, 64);
                if (lane >= d) incl += y;
            }
            if (lane == 63) tot[par][wv] = incl;
            __syncthreads();
            uint32_t before = 0, all = 0;
#pragma unroll
            for (uint32_t v = 0; v < kWaves; ++v) {
                const uint32_t x = tot[par][v];
                all += x;
                if (v < wv) before += x;
            }
            const uint32_t prefix = before + incl - c;
            if (merge && in) store_indices(A.changed + T.changed_off, (uint64_t)n_changed + (prefix & 0xFFFF), T.changed_cap, changed, w);
            if ((flags & hv::kEmitMissing) && in)
                store_indices(A.missing + T.missing_off, 64 * w - ((uint64_t)n_complete + (prefix >> 16)), T.missing_cap, ~now & m, w);
            n_changed += all & 0xFFFF, n_complete += all >> 16;
            if (flags & hv::kEmitStatus) {
                uint32_t e[16];
#pragma unroll
                for (uint32_t k = 0; k < 16; ++k) e[k] = bytes4((uint32_t)(nm >> (4 * k)) & 0xF);
                const uint32_t prev = __shfl_up(e[15], 1, 64);
                if (in) emit_stream<16>(so_lo + 64 * w, e, prev, lane > 0, lane < 63 && w + 1 < W, so_hi);
            }
            if (flags & hv::kEmitWire) {
                const uint32_t e[2] = {__builtin_bswap32((uint32_t)(nm >> 32)), __builtin_bswap32((uint32_t)nm)};
                uint32_t prev = __shfl_up(e[1], 1, 64);
                if (w == 0) prev = __builtin_bswap32((uint32_t)N);
                if (in) emit_stream<2>(wo_lo + 8 + 8 * w, e, prev, lane > 0 || w == 0, lane < 63 && w + 1 < W, wo_hi);
            }
        }
        unexpected = wave_sum(unexpected);
        if (lane == 0) fin[wv] = unexpected;
        __syncthreads();
        if (tid == 0) {
            A.flags_out[t] = bad ? hv::kBadStatus : 0;
            A.n_unexpected[t] = fin[0] + fin[1] + fin[2] + fin[3];
            A.n_changed[t] = n_changed;
            A.n_complete[t] = n_complete;
            A.bytes[t] = hv::bytes_downloaded(n_complete, T.piece_length, T.length);
        }
        __syncthreads();  // fin and tot are free for the next torrent
    }
}

}  // namespace

hipError_t launch_have_round(const HvTorrent* tors, uint64_t n_tors, const HvArrays& a, hipStream_t s) {
    if (!n_tors) return hipSuccess;
    const hipError_t pre = launch_precheck();
    if (pre != hipSuccess) return pre;
    const uint64_t units = n_tors < kHvUnitCap ? n_tors : kHvUnitCap;
    t_launch_plan = 0;
    t_launch_units = n_tors;
    hipLaunchKernelGGL(have_round_kernel, dim3((uint32_t)units), dim3(kBlock), 0, s, tors, n_tors, a);
    return hipGetLastError();
}

}  // namespace krk
