// rates.cpp -- the rates the planners (planner_math.hpp) work with: one host thread's hashes and memcpy measured
// once per process, each device's SHA-256 tiers and pinned copies measured once per device (or again on
// krk_planner_calibrate), nominal MI355X figures without a device, the override of krk_planner_rates_set.
#include <chrono>

#include "offload.hpp"

namespace krk {

// One host thread, bytes/s: measured once (16 MiB) and derated for the clock a fully
// loaded socket holds.  SHA-256 (x86 SHA extensions) and the piece CRC (PCLMUL folding).
static double time_rate(const std::function<void(const uint8_t*, size_t)>& f) {
    std::vector<uint8_t> buf(16u << 20, 0x5a);
    f(buf.data(), 64 << 10);  // warm
    const auto t0 = std::chrono::steady_clock::now();
    f(buf.data(), buf.size());
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return kHostDerate * buf.size() / std::max(s, 1e-6);
}
double host_sha_rate() {
    static const double r = time_rate([](const uint8_t* p, size_t n) {
        uint32_t h[8];
        memcpy(h, kIV, sizeof h);
        host_sha256_blocks(h, p, n / 64);
    });
    return r;
}
double host_copy_rate() {
    static const double r = [] {
        std::vector<uint8_t> dst(16u << 20, 0);  // touched: page faults are not the copy's cost
        return time_rate([&](const uint8_t* p, size_t n) { memcpy(dst.data(), p, n); });
    }();
    return r;
}
double host_crc_rate() {
    static const double r = time_rate([](const uint8_t* p, size_t n) {
        volatile uint32_t c = host_crc32_update(0, p, n);
        (void)c;
    });
    return r;
}

void CalBufs::release() {
    if (s) hipStreamSynchronize(s), hipStreamDestroy(s);
    for (void* p : {(void*)d_in, (void*)d_state, (void*)d_dig, (void*)d_jobs, (void*)d_copy})
        if (p) hipFree(p);
    if (h_copy) hipHostFree(h_copy);
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
}

namespace {

constexpr int kTierPlan[3] = {KRK_SHA_PLAN_8LANE, KRK_SHA_PLAN_2LANE_2PAIR, KRK_SHA_PLAN_1LANE_2PAIR};

// Without a device and without krk_planner_rates_set (planning on a host that has no
// GPU, e.g. the CPU tests): one MI355X as measured in rounds 1-2 -- per-stream rates at
// full residency of 52.6 / 51.6 / 35.7 MB/s (profiles/r02/sha8_probe_c2shape.jsonl,
// sha2_read_groups.jsonl), PCIe Gen5 x16 pinned copies of 54 GB/s.
Rates nominal_rates(int cus) {
    Rates R{};
    R.stream[0] = 52.6e6;
    R.stream[1] = 51.6e6;
    R.stream[2] = 35.7e6;
    R.d2h = R.h2d = 54e9;
    R.host_sha = host_sha_rate();
    R.host_crc = host_crc_rate();
    R.host_copy = host_copy_rate();
    R.cus = cus > 0 ? cus : 256;
    R.source = KRK_RATES_NOMINAL;
    return R;
}

// The device's own rates (~50 ms): each SHA-256 tier's plan timed on 16 / 64 / 128 x CUs
// streams of 256 KiB (every stream reads the same bytes: the kernel is issue-bound, not
// HBM-bound), pinned 64 MiB copies each way, on a stream of the calibration's own.
int calibrate(Device* D, CalBufs& cb, Rates& R) {
    R = Rates{};
    R.cus = D->cus;
    KRK_HIP(hipSetDevice(D->id));
    const uint64_t L = 256u << 10, C = 64u << 20;
    const uint32_t mmax = (uint32_t)(kResidentPerCu[2] * (uint64_t)D->cus);
    hipStream_t& s = cb.s;
    hipEvent_t &e0 = cb.e0, &e1 = cb.e1;
    uint8_t *&d_in = cb.d_in, *&d_dig = cb.d_dig, *&d_copy = cb.d_copy, *&h_copy = cb.h_copy;
    uint32_t*& d_state = cb.d_state;
    ShaJob*& d_jobs = cb.d_jobs;
    int rc = KRK_OK;
    auto ok = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && !rc) {
            set_error(KRK_EHIP, "planner calibration: %s: %s", what, hipGetErrorString(e));
            rc = KRK_EHIP;
        }
        return !rc;
    };
    auto timed_ms = [&](const std::function<hipError_t()>& f) {
        float ms = 0;
        for (int rep = 0; rep < 2 && !rc; ++rep) {  // the first run loads code and warms up
            ok(hipEventRecord(e0, s), "event");
            ok(f(), "launch");
            ok(hipEventRecord(e1, s), "event");
            ok(hipEventSynchronize(e1), "sync");
            ok(hipEventElapsedTime(&ms, e0, e1), "elapsed");
        }
        return (double)std::max(ms, 1e-3f);
    };
    auto have = [&](bool present, const std::function<hipError_t()>& make, const char* what) {
        return present || ok(make(), what);
    };
    if (cb.mmax < mmax) {  // a device with more CUs than the buffers were made for: start over
        for (void* p : {(void*)d_state, (void*)d_dig, (void*)d_jobs})
            if (p) hipFree(p);
        d_state = nullptr;
        d_dig = nullptr;
        d_jobs = nullptr;
        cb.mmax = mmax;
    }
    if (have(s, [&] { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }, "stream") &&
        have(e0, [&] { return hipEventCreate(&e0); }, "event") && have(e1, [&] { return hipEventCreate(&e1); }, "event") &&
        have(d_in, [&] { return hipMalloc(&d_in, L); }, "alloc") &&
        have(d_state, [&] { return hipMalloc(&d_state, 32ull * mmax); }, "alloc") &&
        have(d_dig, [&] { return hipMalloc(&d_dig, 32ull * mmax); }, "alloc") &&
        have(d_jobs, [&] { return hipMalloc(&d_jobs, sizeof(ShaJob) * mmax); }, "alloc") &&
        ok(hipMemsetAsync(d_in, 0x5a, L, s), "memset")) {
        std::vector<ShaJob> jobs(mmax);
        for (uint32_t i = 0; i < mmax; ++i) {
            jobs[i] = ShaJob{};
            jobs[i].ptr = reinterpret_cast<uint64_t>(d_in);
            jobs[i].len = L;
            jobs[i].out = i;
            memcpy(jobs[i].h, kIV, 32);
        }
        if (ok(hipMemcpyAsync(d_jobs, jobs.data(), sizeof(ShaJob) * mmax, hipMemcpyHostToDevice, s), "upload"))
            for (int t = 0; t < 3 && !rc; ++t) {
                const uint32_t m = (uint32_t)(kResidentPerCu[t] * (uint64_t)D->cus);
                const double ms = timed_ms([&] { return launch_sha256_plan(kTierPlan[t], d_jobs, m, d_dig, d_state, s); });
                R.stream[t] = (double)L / (ms * 1e-3);
            }
    }
    if (!rc && have(d_copy, [&] { return hipMalloc(&d_copy, C); }, "alloc") &&
        have(h_copy, [&] { return hipHostMalloc(reinterpret_cast<void**>(&h_copy), C, 0); }, "pin")) {
        // the fastest of three timed copies each way: one copy alone read 45.7 against ~56.5
        // GB/s on one box (bench.py host_link_peak), and the planners price the link with it
        auto best_ms = [&](const std::function<hipError_t()>& f) {
            double ms = timed_ms(f);
            for (int k = 0; k < 2 && !rc; ++k) ms = std::min(ms, timed_ms(f));
            return ms;
        };
        R.h2d = (double)C / (best_ms([&] { return hipMemcpyAsync(d_copy, h_copy, C, hipMemcpyHostToDevice, s); }) * 1e-3);
        R.d2h = (double)C / (best_ms([&] { return hipMemcpyAsync(h_copy, d_copy, C, hipMemcpyDeviceToHost, s); }) * 1e-3);
    }
    if (s) {
        // The buffers stay (freeing waits for the device); the stream does not: a stream
        // kept alive takes a turn in the round-robin of normal-priority streams over the
        // hardware queues, and moved the C3 host lane's D2H copies onto a queue behind the
        // windows' kernels (rank 0's shard of 8 GPUs: lane 16.5 -> 18-20 s).
        hipStreamSynchronize(s);
        hipStreamDestroy(s);
        s = nullptr;
    }
    R.host_sha = host_sha_rate();
    R.host_crc = host_crc_rate();
    R.host_copy = host_copy_rate();
    R.source = KRK_RATES_MEASURED;
    return rc;
}

// Measure D's rates and store them, one calibration of the device at a time; a failed calibration plans with the
// nominal rates.  `again` = false: a caller that waited for another's measurement keeps that one.
int measure(Device* D, RateCache& C, bool again) {
    std::lock_guard<std::mutex> g(C.cal_mu);
    if (!again) {
        std::lock_guard<std::mutex> gm(C.mu);
        if (C.measured) return KRK_OK;
    }
    Rates R{};
    const int rc = calibrate(D, C.cal, R);
    if (rc != KRK_OK) R = nominal_rates(D->cus);
    std::lock_guard<std::mutex> gm(C.mu);
    C.rates = R;
    C.measured = true;
    return rc;
}

std::mutex g_rates_mu;  // the override only: a calibration never runs under it
bool g_rates_set = false;
Rates g_rates_override{};

}  // namespace

// (Re)measure device D's rates now.
int calibrate_device(Device* D) { return measure(D, rate_cache(D), true); }

// The rates the planners use on device D: the override, else D's measured rates (the first
// caller on a device measures them; krk_init measures them eagerly, before the device
// carries any work of the library's), else -- no device -- the nominal ones.  Only the
// device being measured waits for its calibration: no process-wide lock is held across it.
Rates planner_rates(Device* D) {
    {
        std::lock_guard<std::mutex> g(g_rates_mu);
        if (g_rates_set) return g_rates_override;
    }
    if (!D) return nominal_rates(0);
    RateCache& C = rate_cache(D);
    {
        std::lock_guard<std::mutex> g(C.mu);
        if (C.measured) return C.rates;
    }
    measure(D, C, false);
    std::lock_guard<std::mutex> g(C.mu);
    return C.rates;
}

}  // namespace krk

using namespace krk;

extern "C" {

int krk_planner_calibrate(void) {
    KRK_DEVICE(D);
    return calibrate_device(D);
}

int krk_host_offload_plan(const uint64_t* lengths, uint64_t n, int threads, int cus, int mode, uint32_t* host_idx,
                          uint64_t* n_host, double* gpu_seconds_out, double* host_seconds_out) {
    KRK_CHECK(n == 0 || lengths, KRK_EINVAL, "lengths is NULL");
    KRK_CHECK(n_host, KRK_EINVAL, "n_host is NULL");
    KRK_CHECK(threads >= 0 && cus >= 0, KRK_EINVAL, "threads and cus must be >= 0");
    KRK_CHECK(mode >= KRK_OFFLOAD_DEVICE && mode <= KRK_OFFLOAD_HOST_FILES, KRK_EINVAL, "offload mode %d", mode);
    int drc = KRK_OK;
    Device* D = device(&drc);  // none: the override or the nominal rates
    Rates R = planner_rates(D);
    if (cus > 0) R.cus = cus;
    std::vector<uint32_t> idx = offload_plan(lengths, n, threads, R, gpu_seconds_out, host_seconds_out, mode);
    *n_host = idx.size();
    if (host_idx && !idx.empty()) memcpy(host_idx, idx.data(), idx.size() * 4);
    return KRK_OK;
}

int krk_sha_offload_plan(const uint64_t* lengths, uint64_t n, int threads, int cus, uint32_t* host_idx,
                         uint64_t* n_host, double* gpu_seconds_out, double* host_seconds_out) {
    return krk_host_offload_plan(lengths, n, threads, cus, KRK_OFFLOAD_DEVICE, host_idx, n_host, gpu_seconds_out,
                                 host_seconds_out);
}

int krk_sha_tail_plan(const uint64_t* lengths, uint64_t n, int threads, uint32_t* host_idx, uint64_t* start,
                      uint64_t* n_out, double* end_s, double* gpu_s) {
    KRK_CHECK(lengths && host_idx && start && n_out, KRK_EINVAL, "sha_tail_plan: null argument");
    KRK_CHECK(threads >= 0, KRK_EINVAL, "sha_tail_plan: threads < 0");
    int drc = KRK_OK;
    Device* D = device(&drc);  // none: the override or the nominal rates
    const TailPlan tp = tail_plan(lengths, n, threads, planner_rates(D));
    *n_out = tp.idx.size();
    for (size_t k = 0; k < tp.idx.size(); ++k) {
        host_idx[k] = tp.idx[k];
        start[k] = tp.start[k];
    }
    if (end_s) *end_s = tp.end_s;
    if (gpu_s) *gpu_s = tp.gpu_s;
    return KRK_OK;
}

int krk_planner_rates_get(krk_planner_rates* out) {
    KRK_CHECK(out, KRK_EINVAL, "out is NULL");
    int drc = KRK_OK;
    const Rates R = planner_rates(device(&drc));
    for (int t = 0; t < 3; ++t) out->sha_stream_bps[t] = R.stream[t];
    out->d2h_bps = R.d2h;
    out->h2d_bps = R.h2d;
    out->host_sha_bps = R.host_sha;
    out->host_crc_bps = R.host_crc;
    out->host_copy_bps = R.host_copy;
    out->cus = R.cus;
    out->source = R.source;
    return KRK_OK;
}

int krk_planner_rates_set(const krk_planner_rates* in) {
    std::lock_guard<std::mutex> g(g_rates_mu);
    if (!in) {
        g_rates_set = false;
        return KRK_OK;
    }
    KRK_CHECK(in->sha_stream_bps[0] > 0 && in->sha_stream_bps[1] > 0 && in->sha_stream_bps[2] > 0 &&
                  in->d2h_bps > 0 && in->h2d_bps > 0 && in->host_sha_bps > 0 && in->host_crc_bps > 0 && in->host_copy_bps > 0 && in->cus > 0,
              KRK_EINVAL, "planner rates must be positive");
    Rates R{};
    for (int t = 0; t < 3; ++t) R.stream[t] = in->sha_stream_bps[t];
    R.d2h = in->d2h_bps;
    R.h2d = in->h2d_bps;
    R.host_sha = in->host_sha_bps;
    R.host_crc = in->host_crc_bps;
    R.host_copy = in->host_copy_bps;
    R.cus = in->cus;
    R.source = KRK_RATES_SET;
    g_rates_override = R;
    g_rates_set = true;
    return KRK_OK;
}

}  // extern "C"
