// planner_math.hpp -- the placement planners' arithmetic over a Rates value (rates.cpp): which blobs of a batch
// the host hashes whole (offload_plan), which chains it takes over mid-way (tail_plan), from how many live digesters
// on the GPU's engine out-hashes the host (digester_crossover).  Header-only and free of the runtime, so that
// tests/native/planner_math_main.cpp builds it stand-alone under AddressSanitizer and UndefinedBehaviorSanitizer.
#pragma once
#include <algorithm>
#include <functional>
#include <queue>
#include <vector>

#include "../../include/kraken_hip_internal.h"

namespace krk {

// SHA-256 host offload (offload.cpp): the longest blobs of a batch hashed on host threads while the GPU hashes the
// rest (krk_set_sha_host_offload).  Where the batch lives decides what the host saves:
//  * kOffDevice: blobs in HBM; the host reads its blobs out over D2H, the GPU still computes every piece CRC
//    (krk_sha256_dev, krk_metainfo_digest_dev);
//  * kOffHostSha: blobs in host memory, digests only; the host's blobs are hashed in place and never uploaded
//    (krk_sha256_host);
//  * kOffHostWhole: blobs in host memory, digests and piece sums; the host's blobs are hashed AND piece-summed in
//    place and never uploaded (krk_metainfo_digest_host) -- the batch's bytes over the host link shrink by theirs.
//  * kOffHostFiles: cache files (krk_metainfo_digest_files): a host blob is read once and hashed and piece-summed
//    chunk by chunk on one host thread.
enum OffMode { kOffDevice = 0, kOffHostSha = 1, kOffHostWhole = 2, kOffHostFiles = 3 };
static_assert(KRK_OFFLOAD_DEVICE == kOffDevice && KRK_OFFLOAD_HOST_SHA == kOffHostSha &&
                  KRK_OFFLOAD_HOST_WHOLE == kOffHostWhole && KRK_OFFLOAD_HOST_FILES == kOffHostFiles,
              "offload modes");

// What the planners know about this box (rates.cpp): per-stream SHA-256 rate of each AUTO tier at full residency
// (eight / two / one lane(s)), pinned D2H / H2D, one host thread's SHA-256 and CRC-32; measured on the device at
// first use.
struct Rates {
    double stream[3];
    double d2h, h2d, host_sha, host_crc, host_copy;
    int cus;
    int source;  // KRK_RATES_*
};

constexpr double kHostDerate = 0.85;  // one thread's measured rate at the clock a fully loaded socket holds

// Kernel geometry (a property of the code, not of the box): the AUTO launch plan's three tiers -- eight lanes a
// stream up to 16 x CUs streams, two lanes up to 64 x CUs, one lane beyond -- and the streams each tier keeps
// resident per CU (one pair a workgroup at eight lanes, two pairs of 32 / 64 streams at two / one lane(s)).
constexpr uint64_t kTierMaxPerCu[2] = {16, 64};
constexpr uint64_t kResidentPerCu[3] = {16, 64, 128};

inline int tier_of(uint64_t m, int cus) {
    return m <= kTierMaxPerCu[0] * (uint64_t)cus ? 0 : m <= kTierMaxPerCu[1] * (uint64_t)cus ? 1 : 2;
}

// GPU time of m streams (longest `longest` bytes, `bytes` in all) under the AUTO launch plan: the longest chain at
// the tier's per-stream rate, or the streams' bytes at the tier's aggregate (per-stream rate x streams resident on
// the chip) when they outnumber what runs at once.
inline double gpu_seconds(uint64_t longest, double bytes, uint64_t m, const Rates& R) {
    if (!m) return 0;
    const int t = tier_of(m, R.cus);
    const double r = R.stream[t];
    const double cap = (double)kResidentPerCu[t] * R.cus * r;
    return std::max(longest / r, bytes / std::min(m * r, cap));
}

// Host-resident batches: the caller's pageable bytes are copied into pinned windows on host threads while the
// previous window uploads; measured end to end at ~0.85 of the pinned H2D rate (C2 end-to-end 45.7-54.4 GB/s against
// 54 GB/s pinned).
inline double host_link(const Rates& R) { return 0.85 * R.h2d; }

// The AUTO Digester crossover (digester.cpp host_stream_limit): m live digesters on the host run SHA-NI on their
// writers' threads, min(m, threads) x one thread's rate; on the GPU their pending slots are coalesced into
// multi-stream launches that read the pinned slots in place, m x the tier's per-stream rate (x kEngineEff: the
// engine's launches start and end with the writers, measured 0.93 of the batch kernel's rate at 256 digesters,
// profiles/r04/bench_engine.json) up to the tier's residency, capped by what the engine's zero-copy slot reads carry
// over the link (kEngineLinkFrac of the pinned H2D rate: at most 32.7 GB/s of 56.3 measured, at 2,048 digesters,
// profiles/r05/bench_engine_inflight_cap.json).  The crossover is the smallest m whose GPU aggregate beats the
// host's; none (the host out-hashes the engine) is INT64_MAX: every AUTO digester stays on the host.
constexpr double kEngineEff = 0.93;
constexpr double kEngineLinkFrac = 0.58;
inline double engine_gpu_bps(uint64_t m, const Rates& R) {
    if (!m) return 0;
    const int t = tier_of(m, R.cus);
    const double r = R.stream[t] * kEngineEff;
    return std::min({(double)m * r, (double)kResidentPerCu[t] * R.cus * r, kEngineLinkFrac * R.h2d});
}
inline int64_t digester_crossover(const Rates& R, int threads) {
    const double host = std::max(1, threads) * R.host_sha;
    for (int t = 0; t < 3; ++t) {  // the first m (tier by tier) with m x r > host
        const uint64_t lo = t == 0 ? 1 : kTierMaxPerCu[t - 1] * (uint64_t)R.cus + 1;
        const uint64_t hi = t < 2 ? kTierMaxPerCu[t] * (uint64_t)R.cus : UINT64_MAX / 2;
        const double r = R.stream[t] * kEngineEff;
        // a quotient of 2^63 or more is past every tier's hi (and past what the cast may take)
        if (!(host / r < 9223372036854775808.0)) continue;
        const uint64_t m = std::max<uint64_t>(lo, (uint64_t)(host / r) + 1);
        if (m <= hi && engine_gpu_bps(m, R) > host) return (int64_t)m;
    }
    return INT64_MAX;
}

// The blobs the host hashes whole on `threads` threads: the prefix of the stable longest-first order that minimises
// max(GPU seconds, host seconds), written to *gpu_s / *host_s; empty when that gains less than the mode's margin.
inline std::vector<uint32_t> offload_plan(const uint64_t* lens, uint64_t n, int threads, const Rates& R, double* gpu_s,
                                          double* host_s, int mode = kOffDevice) {
    std::vector<uint32_t> order(n);
    for (uint64_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return lens[a] > lens[b]; });
    std::vector<double> suffix(n + 1, 0.0);
    for (uint64_t k = n; k-- > 0;) suffix[k] = suffix[k + 1] + (double)lens[order[k]];
    // GPU side with blobs k.. on the GPU: their longest chain / the chip's SHA rate, and for
    // host-resident batches their bytes over the host link (the host's blobs never cross).
    auto gpu_side = [&](uint64_t k) {
        double g = k < n ? gpu_seconds(lens[order[k]], suffix[k], n - k, R) : 0.0;
        if (mode != kOffDevice) g = std::max(g, suffix[k] / host_link(R));
        return g;
    };
    const double f0 = n ? gpu_side(0) : 0.0;
    double best = f0, best_g = f0, best_h = 0;
    uint64_t best_k = 0;
    if (threads > 0 && n) {
        const double rs = R.host_sha, rc = mode == kOffHostWhole ? R.host_crc : 0.0;
        // LPT over host threads of the tasks, in seconds: a SHA-256 pass per blob, and in
        // kOffHostWhole a piece-CRC pass per blob as its own task.
        std::priority_queue<double, std::vector<double>, std::greater<double>> load;
        for (int t = 0; t < threads; ++t) load.push(0.0);
        double maxload = 0, hbytes = 0;
        auto put = [&](double sec) {
            const double l = load.top() + sec;
            load.pop();
            load.push(l);
            maxload = std::max(maxload, l);
        };
        for (uint64_t k = 1; k <= n; ++k) {
            const double L = (double)lens[order[k - 1]];
            if (L == 0) break;  // empty blobs are not worth a thread
            if (mode == kOffHostFiles) {
                put(L / rs + L / R.host_crc + L / R.host_copy);  // one read, SHA-256 and CRC per chunk
            } else {
                put(L / rs);
                if (mode == kOffHostWhole) put(L / rc);
            }
            hbytes += L;
            const double h = mode == kOffDevice ? std::max(maxload, hbytes / R.d2h) : maxload;
            const double g = gpu_side(k);
            if (std::max(g, h) < best) {
                best = std::max(g, h);
                best_k = k;
                best_g = g;
                best_h = h;
            }
            if (h > f0) break;  // the host alone is already slower than no offload
        }
        if (best > (mode == kOffDevice ? 0.9 : 0.97) * f0) {
            best_k = 0;
            best_g = f0;
            best_h = 0;
        }
    }
    if (gpu_s) *gpu_s = best_g;
    if (host_s) *host_s = best_h;
    order.resize(best_k);
    return order;
}

// Tail handoff of device-resident chains (kOffDevice): every chain starts on the GPU and host threads take over the
// tails of the longest ones.  A SHA-256 chain is one sequential Merkle-Damgard stream, so a batch of equally long
// chains (C2: 1,000 x 100 MiB) ends when one chain ends at the GPU's ~59 MB/s a stream, however many are moved whole
// to the host -- but a host thread (SHA-NI, ~2 GB/s) that takes chain i over at time t finishes it in
// (L_i - r t) / h, and the GPU has done r t of it meanwhile.  Host threads working through takeovers one after
// another shrink the batch's end E: for C2 on 16 threads the model gives ~1.48 s against 1.78 s on the GPU alone.
// Plan for a target E: chains the GPU ends by E (L_i <= r E) stay; every other chain must be taken over by its
// deadline (E - L_i / h) / (1 - r / h); earliest deadline first over the threads (each free at the end of its
// previous tail), the GPU's prefix Y_i = r t_i rounded down to a 64-byte block.  E is the smallest feasible target
// (bisection).  r = the per-stream rate of the batch's plan tier, h = one thread's SHA-NI rate, capped by its share
// of the device-to-host copy rate.
// Chain idx[k] runs its first start[k] bytes on the GPU (0: none) and the rest on a host thread from the GPU's
// midstate; listed in the order of start (the host threads' queue).  end_s = the planned batch end, gpu_s = the GPU
// alone; empty when host takeovers would not end the batch sooner.
struct TailPlan {
    std::vector<uint32_t> idx;
    std::vector<uint64_t> start;
    double gpu_s = 0, end_s = 0;
};
inline TailPlan tail_plan(const uint64_t* lens, uint64_t n, int threads, const Rates& R) {
    TailPlan best;
    if (!n || threads <= 0) return best;
    const double r = R.stream[tier_of(n, R.cus)];
    // a tail thread runs SHA-NI alone over its two pinned buffers: 16 of them hashed 2.42 GB/s each against 2.47 for
    // one C1 thread (profiles/r05/c2_tail_handoff_trace.txt), so the rate is derated 2 %, not the 15 % that holds for
    // the host-whole and file modes (SHA + CRC + copies: the warm files leg lost 58.9 -> 55.0 GB/s when those were
    // priced at 5 %)
    const double h = std::min(R.host_sha * (0.98 / kHostDerate), R.d2h / threads);
    if (!(r > 0) || !(h > r)) return best;
    uint64_t longest = 0;
    double total = 0;
    for (uint64_t i = 0; i < n; ++i) {
        longest = std::max(longest, lens[i]);
        total += (double)lens[i];
    }
    best.gpu_s = gpu_seconds(longest, total, n, R);
    // only chain-bound batches gain (the GPU's time is its longest chain, not its aggregate
    // rate), and the plan stays cheap: at most 65,536 chains
    if (n > (1u << 16) || longest / r < 0.9 * best.gpu_s) return best;
    std::vector<uint32_t> order(n);
    for (uint64_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return lens[a] > lens[b]; });
    auto plan = [&](double E, TailPlan* out) {
        std::priority_queue<double, std::vector<double>, std::greater<double>> free_at;
        for (int t = 0; t < threads; ++t) free_at.push(0.0);
        for (uint32_t i : order) {  // longest first = earliest deadline first
            const double L = (double)lens[i];
            if (L <= r * E) break;
            const double deadline = (E - L / h) / (1.0 - r / h);
            const double t = free_at.top();
            if (deadline < 0 || t > deadline) return false;
            free_at.pop();
            const uint64_t y = std::min<uint64_t>((uint64_t)(r * t) / 64 * 64, lens[i] / 64 * 64);
            free_at.push(t + (L - (double)y) / h);
            if (out) {
                out->idx.push_back(i);
                out->start.push_back(y);
            }
        }
        return true;
    };
    double lo = 0, hi = best.gpu_s;
    if (plan(0.0, nullptr) || !plan(hi, nullptr)) return best;  // nothing to gain
    for (int it = 0; it < 40; ++it) {
        const double mid = 0.5 * (lo + hi);
        (plan(mid, nullptr) ? hi : lo) = mid;
    }
    plan(hi, &best);
    best.end_s = hi;
    // takeovers in the order their prefixes end on the GPU (the host threads' queue)
    std::vector<size_t> o(best.idx.size());
    for (size_t k = 0; k < o.size(); ++k) o[k] = k;
    std::stable_sort(o.begin(), o.end(), [&](size_t a, size_t b) { return best.start[a] < best.start[b]; });
    TailPlan sorted;
    sorted.gpu_s = best.gpu_s;
    sorted.end_s = best.end_s;
    for (size_t k : o) {
        sorted.idx.push_back(best.idx[k]);
        sorted.start.push_back(best.start[k]);
    }
    return sorted;
}

}  // namespace krk
