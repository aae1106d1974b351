// The placement planners' arithmetic (kraken_amd/csrc/planner_math.hpp) as a stand-alone program,
// each planner against a plain restatement over a small space taken exhaustively:
//  1. offload_plan: the argmin over EVERY prefix k of the stable longest-first order of
//     max(GPU seconds, host seconds), the host's seconds from a naive LPT over an array of loads;
//  2. tail_plan: its schedule replayed on `threads` threads, starts 64-byte multiples inside their chains;
//  3. digester_crossover: a linear scan over m for the first m whose modelled GPU aggregate beats the host.
// Lengths from {0, 1, 63, 64, 2^20, 2^30, 2^40 + 1}: every list of n <= 3, drawn lists of n <= 10 and around
// the tier edges of one CU (16, 17, 64, 65 chains); threads 0-4 and n + 1; all four modes; 1 and 256 CUs;
// three rate sets.  Then every field at 1e-9 or 1e18 B/s: the same checks, and no conversion out of range.
#include <math.h>
#include <stdio.h>

#include "../../kraken_amd/csrc/planner_math.hpp"

using namespace krk;

static int g_cases = 0, g_bad = 0, g_offloaded = 0, g_tails = 0, g_cross = 0;
#define CHECK(cond, ...)                        \
    do {                                        \
        if (!(cond)) {                          \
            if (g_bad++ < 20) {                 \
                printf("MISMATCH %s: ", #cond); \
                printf(__VA_ARGS__);            \
                printf("\n");                   \
            }                                   \
        }                                       \
    } while (0)

static uint64_t g_x = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_x ^= g_x << 13, g_x ^= g_x >> 7, g_x ^= g_x << 17;
    return (uint32_t)(g_x >> 16);
}

static bool close_to(double a, double b) { return fabs(a - b) <= 1e-12 * fmax(fabs(a), fabs(b)); }

// ---------------------------------------------------------------- restatements
static int ref_tier(uint64_t m, int cus) { return m <= 16ull * cus ? 0 : m <= 64ull * cus ? 1 : 2; }
static const double kRefResident[3] = {16, 64, 128};

static double ref_gpu_seconds(uint64_t longest, double bytes, uint64_t m, const Rates& R) {
    if (!m) return 0;
    const int t = ref_tier(m, R.cus);
    const double chain = longest / R.stream[t];
    const double aggregate = fmin(m * R.stream[t], kRefResident[t] * R.cus * R.stream[t]);
    return fmax(chain, bytes / aggregate);
}

// Stable longest-first order by insertion.
static std::vector<uint32_t> ref_order(const std::vector<uint64_t>& lens) {
    std::vector<uint32_t> o;
    for (uint32_t i = 0; i < lens.size(); ++i) {
        size_t at = o.size();
        while (at > 0 && lens[o[at - 1]] < lens[i]) --at;
        o.insert(o.begin() + at, i);
    }
    return o;
}

// Seconds of the host's tasks, each given in turn to the least loaded of `threads` threads.
static double ref_lpt(const std::vector<double>& tasks, int threads) {
    std::vector<double> load(threads, 0.0);
    for (double s : tasks) {
        size_t least = 0;
        for (size_t t = 1; t < load.size(); ++t)
            if (load[t] < load[least]) least = t;
        load[least] += s;
    }
    double longest = 0;
    for (double l : load) longest = fmax(longest, l);
    return longest;
}

struct RefPlan {
    uint64_t k = 0;
    double gpu_s = 0, host_s = 0;
};
static RefPlan ref_offload_plan(const std::vector<uint64_t>& lens, int threads, const Rates& R, int mode) {
    const std::vector<uint32_t> o = ref_order(lens);
    const uint64_t n = lens.size();
    auto gpu_side = [&](uint64_t k) {
        double bytes = 0;
        for (uint64_t j = k; j < n; ++j) bytes += (double)lens[o[j]];
        double g = k < n ? ref_gpu_seconds(lens[o[k]], bytes, n - k, R) : 0.0;
        if (mode != KRK_OFFLOAD_DEVICE) g = fmax(g, bytes / (0.85 * R.h2d));
        return g;
    };
    RefPlan p;
    p.gpu_s = n ? gpu_side(0) : 0.0;
    if (threads <= 0 || !n) return p;
    const double f0 = p.gpu_s;
    double best = f0;
    for (uint64_t k = 1; k <= n && lens[o[k - 1]] > 0; ++k) {  // empty blobs never go to the host
        std::vector<double> tasks;
        double hbytes = 0;
        for (uint64_t j = 0; j < k; ++j) {
            const double L = (double)lens[o[j]];
            hbytes += L;
            if (mode == KRK_OFFLOAD_HOST_FILES) {
                tasks.push_back(L / R.host_sha + L / R.host_crc + L / R.host_copy);
            } else {
                tasks.push_back(L / R.host_sha);
                if (mode == KRK_OFFLOAD_HOST_WHOLE) tasks.push_back(L / R.host_crc);
            }
        }
        double h = ref_lpt(tasks, threads);
        if (mode == KRK_OFFLOAD_DEVICE) h = fmax(h, hbytes / R.d2h);
        const double g = gpu_side(k);
        if (fmax(g, h) < best) {
            best = fmax(g, h);
            p.k = k;
            p.gpu_s = g;
            p.host_s = h;
        }
    }
    if (best > (mode == KRK_OFFLOAD_DEVICE ? 0.9 : 0.97) * f0) {
        p.k = 0;
        p.gpu_s = f0;
        p.host_s = 0;
    }
    return p;
}

static double ref_engine_bps(uint64_t m, const Rates& R) {
    if (!m) return 0;
    const int t = ref_tier(m, R.cus);
    const double r = R.stream[t] * 0.93;
    return fmin(fmin((double)m * r, kRefResident[t] * R.cus * r), 0.58 * R.h2d);
}

// ---------------------------------------------------------------- checks
static void check_offload(const std::vector<uint64_t>& lens, int threads, const Rates& R, int mode) {
    double g = -1, h = -1;
    const std::vector<uint32_t> idx = offload_plan(lens.data(), lens.size(), threads, R, &g, &h, mode);
    ++g_cases;
    g_offloaded += !idx.empty();
    const std::vector<uint32_t> o = ref_order(lens);
    CHECK(idx.size() <= o.size(), "n=%zu", lens.size());
    for (size_t j = 0; j < idx.size() && j < o.size(); ++j)  // a prefix of the stable longest-first order
        CHECK(idx[j] == o[j], "n=%zu threads=%d mode=%d j=%zu", lens.size(), threads, mode, j);
    for (uint32_t i : idx) CHECK(lens[i] > 0, "an empty blob on the host");
    const RefPlan p = ref_offload_plan(lens, threads, R, mode);
    CHECK(idx.size() == p.k, "n=%zu threads=%d mode=%d cus=%d: k %zu against %llu", lens.size(), threads, mode, R.cus,
          idx.size(), (unsigned long long)p.k);
    CHECK(close_to(g, p.gpu_s) && close_to(h, p.host_s), "n=%zu threads=%d mode=%d: %.17g %.17g against %.17g %.17g",
          lens.size(), threads, mode, g, h, p.gpu_s, p.host_s);
}

static void check_tail(const std::vector<uint64_t>& lens, int threads, const Rates& R) {
    const uint64_t n = lens.size();
    const TailPlan tp = tail_plan(lens.data(), n, threads, R);
    ++g_cases;
    CHECK(tp.idx.size() == tp.start.size(), "n=%zu", (size_t)n);
    if (tp.idx.empty()) return;
    ++g_tails;
    uint64_t longest = 0;
    double total = 0;
    for (uint64_t L : lens) longest = longest < L ? L : longest, total += (double)L;
    CHECK(threads > 0 && close_to(tp.gpu_s, ref_gpu_seconds(longest, total, n, R)), "gpu_s %.17g", tp.gpu_s);
    CHECK(tp.end_s <= tp.gpu_s, "end %.17g after the GPU alone %.17g", tp.end_s, tp.gpu_s);
    if (threads <= 0) return;
    const double r = R.stream[ref_tier(n, R.cus)];
    const double h = fmin(R.host_sha * (0.98 / 0.85), R.d2h / threads);
    // Replay: the takeovers in their listed order, each on the thread that is free first, none before the GPU
    // has hashed its prefix.  The plan sizes each tail from r t and then rounds the prefix down to a block, so
    // a tail is up to 63 bytes longer than planned: the replay may end 64 / h s (and rounding) after end_s.
    std::vector<double> free_at(threads, 0.0);
    std::vector<char> taken(n, 0);
    double end = 0;
    for (size_t k = 0; k < tp.idx.size(); ++k) {
        const uint32_t i = tp.idx[k];
        CHECK(i < n && !taken[i], "chain %u listed twice or out of range", i);
        if (i >= n) return;
        taken[i] = 1;
        CHECK(tp.start[k] % 64 == 0 && tp.start[k] <= lens[i], "start %llu of %llu", (unsigned long long)tp.start[k],
              (unsigned long long)lens[i]);
        CHECK(k == 0 || tp.start[k - 1] <= tp.start[k], "not in the order of start");
        size_t first = 0;
        for (size_t t = 1; t < free_at.size(); ++t)
            if (free_at[t] < free_at[first]) first = t;
        const double begin = fmax(free_at[first], (double)tp.start[k] / r);
        free_at[first] = begin + (double)(lens[i] - tp.start[k]) / h;
        end = fmax(end, free_at[first]);
    }
    for (uint64_t i = 0; i < n; ++i)
        if (!taken[i]) end = fmax(end, (double)lens[i] / r);  // the GPU ends the others itself
    CHECK(end <= tp.end_s * (1 + 1e-9) + 64.0 / h, "n=%zu threads=%d: replay ends %.17g, planned %.17g", (size_t)n,
          threads, end, tp.end_s);
}

static void check_crossover(const Rates& R, int threads) {
    const int64_t m = digester_crossover(R, threads);
    const double host = (threads > 1 ? threads : 1) * R.host_sha;
    ++g_cases;
    int64_t scan = INT64_MAX;  // beyond the last tier's residency the aggregate no longer grows
    for (uint64_t k = 1; k <= 128ull * R.cus + 1; ++k)
        if (ref_engine_bps(k, R) > host) {
            scan = (int64_t)k;
            break;
        }
    CHECK(m == scan, "threads=%d cus=%d: %lld against the scan's %lld", threads, R.cus, (long long)m, (long long)scan);
    if (m != INT64_MAX) {
        ++g_cross;
        CHECK(m >= 1 && engine_gpu_bps((uint64_t)m, R) > host, "threads=%d: m=%lld does not beat the host", threads,
              (long long)m);
    }
}

static const uint64_t kLens[7] = {0, 1, 63, 64, 1ull << 20, 1ull << 30, (1ull << 40) + 1};

static Rates rates(double s0, double s1, double s2, double d2h, double h2d, double sha, double crc, double copy) {
    Rates R{};
    R.stream[0] = s0, R.stream[1] = s1, R.stream[2] = s2;
    R.d2h = d2h, R.h2d = h2d, R.host_sha = sha, R.host_crc = crc, R.host_copy = copy;
    R.cus = 256;
    R.source = KRK_RATES_SET;
    return R;
}

static void check_list(const std::vector<uint64_t>& lens, const Rates* sets, int n_sets) {
    const int n = (int)lens.size();
    for (int s = 0; s < n_sets; ++s)
        for (int cus : {1, 256}) {
            Rates R = sets[s];
            R.cus = cus;
            for (int threads : {0, 1, 2, 3, 4, n + 1}) {
                for (int mode = KRK_OFFLOAD_DEVICE; mode <= KRK_OFFLOAD_HOST_FILES; ++mode)
                    check_offload(lens, threads, R, mode);
                check_tail(lens, threads, R);
            }
        }
}

int main() {
    const Rates sets[3] = {
        rates(52.6e6, 51.6e6, 35.7e6, 54e9, 54e9, 2.1e9, 17e9, 10e9),  // one MI355X beside a SHA-NI core
        rates(400e6, 300e6, 200e6, 20e9, 25e9, 0.5e9, 3e9, 4e9),       // a slow host
        rates(20e6, 15e6, 10e6, 8e9, 6e9, 5e9, 30e9, 20e9),            // a fast host behind a slow link
    };
    // every list of n <= 3 lengths
    for (int n = 0; n <= 3; ++n) {
        uint64_t count = 1;
        for (int j = 0; j < n; ++j) count *= 7;
        for (uint64_t c = 0; c < count; ++c) {
            std::vector<uint64_t> lens(n);
            uint64_t q = c;
            for (int j = 0; j < n; ++j, q /= 7) lens[j] = kLens[q % 7];
            check_list(lens, sets, 3);
        }
    }
    // drawn lists of 4..10, and around one CU's tier edges
    for (int n : {4, 5, 6, 7, 8, 9, 10, 16, 17, 64, 65})
        for (int rep = 0; rep < (n <= 10 ? 20 : 4); ++rep) {
            std::vector<uint64_t> lens(n);
            for (auto& L : lens) L = kLens[rnd() % 7];
            check_list(lens, sets, 3);
        }
    for (int s = 0; s < 3; ++s)
        for (int cus : {1, 256})
            for (int threads : {0, 1, 2, 3, 4, 16, 64, 1024}) {
                Rates R = sets[s];
                R.cus = cus;
                check_crossover(R, threads);
            }
    {  // more chains than a tail plan looks at
        std::vector<uint64_t> lens(65537, 1ull << 20);
        const TailPlan tp = tail_plan(lens.data(), lens.size(), 4, sets[0]);
        ++g_cases;
        CHECK(tp.idx.empty() && tp.start.empty() && tp.gpu_s > 0, "65,537 chains planned");
        lens.resize(65536);  // the most it looks at: equal chains, 16 threads, as C2
        check_tail(lens, 16, sets[0]);
    }
    // edge rates: every field at 1e-9 or 1e18 B/s
    for (int bits = 0; bits < 64; ++bits) {
        auto v = [&](int b) { return (bits >> b) & 1 ? 1e18 : 1e-9; };
        const Rates E = rates(v(0), v(0), v(0), v(1), v(2), v(3), v(4), v(5));
        for (int cus : {1, 256}) {
            Rates R = E;
            R.cus = cus;
            for (int threads : {0, 1, 4, 1024}) {
                if (threads == 1 || threads == 1024) check_crossover(R, threads);  // 0 counts as 1
                for (const std::vector<uint64_t>& lens : {std::vector<uint64_t>{}, std::vector<uint64_t>{0, 0},
                                                          std::vector<uint64_t>{kLens[6], kLens[5], 64, 63, 1, 0},
                                                          std::vector<uint64_t>(20, kLens[6])}) {
                    for (int mode = KRK_OFFLOAD_DEVICE; mode <= KRK_OFFLOAD_HOST_FILES; ++mode)
                        check_offload(lens, threads, R, mode);
                    check_tail(lens, threads, R);
                }
            }
        }
    }
    // the space is not vacuous: some batches were offloaded, some tails handed over, some crossovers exist
    CHECK(g_offloaded > 1000 && g_tails > 1000 && g_cross > 10, "offloaded %d tails %d crossovers %d", g_offloaded,
          g_tails, g_cross);
    printf("planner_math: %d cases (%d offloaded, %d tail plans, %d crossovers), %d mismatches\n", g_cases, g_offloaded,
           g_tails, g_cross, g_bad);
    return g_bad != 0;
}
