// runtime.cpp -- the C ABI (include/kraken_hip.h): error state, device contexts and their
// teardown, synthetic fills, the memory / stream / event wrappers, timing and stats.  The
// batch calls live in batch_dev.cpp (device-resident), crc_host.cpp (host-resident CRC),
// windows.cpp (host-resident digest + metainfo; the pass itself in window_pass.cpp) and placement.cpp (HRW, ring).
#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <sys/mman.h>
#include <unistd.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "offload.hpp"
#include "runtime.hpp"
#include "staging.hpp"

namespace krk {

thread_local std::string t_err;
thread_local int t_dev = 0;

void set_error(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    t_err = buf;
    // A HIP failure the library reports is consumed here: left pending on the thread, the
    // next launch would report it again as an unchecked earlier error (launch_precheck).
    if (code == KRK_EHIP || code == KRK_ENOMEM) (void)hipGetLastError();
}

void set_device_set_from_mask(uint64_t mask);    // multidev.cpp

// Everything a device context holds: streams, tables, scratch cache, pinned
// upload slots, staging windows, the shard-key table.  Only for krk_shutdown.
static void teardown_device(Device& D) {
    hipSetDevice(D.id);
    for (hipStream_t s : {D.s_main, D.s_a, D.s_b})
        if (s) hipStreamSynchronize(s);
    delete D.staging;  // drains its windows' events
    D.staging = nullptr;
    offload_teardown(D);
    owner_tables_teardown(D);  // before the scratch cache: the tables' blocks go back to it
    {
        std::lock_guard<std::mutex> g(D.cache.mu);
        for (auto& kv : D.cache.idle) {
            hipFree(kv.second.p);
            if (kv.second.ev) hipEventDestroy(kv.second.ev);
        }
        D.cache.idle.clear();
        for (auto& kv : D.cache.live) {  // none unless a call is in flight (contract)
            hipFree(kv.second.p);
            if (kv.second.ev) hipEventDestroy(kv.second.ev);
        }
        D.cache.live.clear();
    }
    for (auto& R : D.rings)
        for (PinnedSlot& P : R->slot) {
            if (P.ev) hipEventSynchronize(P.ev), hipEventDestroy(P.ev);
            if (P.p) hipHostFree(P.p);
        }
    D.rings.clear();
    D.ring_of.clear();
    for (void* p : D.retired_pinned) hipHostFree(p);
    D.retired_pinned.clear();
    for (void* p : {(void*)D.shard_kb, (void*)D.shard_koff, (void*)D.shard_bad, (void*)D.d_tabs})
        if (p) hipFree(p);
    for (hipStream_t s : {D.s_main, D.s_a, D.s_b})
        if (s) hipStreamDestroy(s);
}

}  // namespace krk

using namespace krk;

// ======================================================================= C ABI
extern "C" {

const char* krk_version(void) { return "kraken_amd 0.1 (gfx950)"; }
const char* krk_last_error(void) { return t_err.c_str(); }

int krk_device_count(int* n) {
    KRK_CHECK(n, KRK_EINVAL, "n is NULL");
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
    int good = 0;
    for (int i = 0; i < c; ++i) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, i) == hipSuccess && strncmp(p.gcnArchName, "gfx950", 6) == 0) ++good;
    }
    *n = good;
    return KRK_OK;
}

int krk_init(uint64_t dev_mask) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        set_error(KRK_ENODEV, "no HIP device visible");
        return KRK_ENODEV;
    }
    const int saved = t_dev;
    int r = KRK_OK;
    for (int i = 0; i < n && i < 64 && !r; ++i) {
        if (dev_mask ? !((dev_mask >> i) & 1) : i != saved) continue;
        t_dev = i;
        int rc = KRK_OK;
        Device* D = device(&rc);
        if (!D) r = rc;
        // the planners' rates, measured now while the library has no work on the device
        // (a first use under load would fix a contended split for the process)
        else if (!KRK_OP_ENV("KRK_NO_CALIBRATE")) r = calibrate_device(D);
    }
    for (int i = n; i < 64 && !r; ++i)
        if ((dev_mask >> i) & 1) {
            set_error(KRK_ENODEV, "device %d out of range (%d visible)", i, n);
            r = KRK_ENODEV;
        }
    t_dev = saved;
    if (!r) {
        int rc = KRK_OK;
        device(&rc);  // restore the calling thread's current device
        if (dev_mask) set_device_set_from_mask(dev_mask);  // the multi-device entry points' devices
    }
    return r;
}

int krk_shutdown(void) {
    std::lock_guard<std::mutex> g(g_dmu);
    for (auto& D : g_devs)
        if (D) {
            engine_teardown(*D);  // dispatcher threads first: they launch on this context
            teardown_device(*D);
            D.reset();
        }
    return KRK_OK;
}

int krk_set_device(int dev) {
    t_dev = dev;
    KRK_DEVICE(D);
    (void)D;
    return KRK_OK;
}

int krk_synchronize(void) {
    KRK_DEVICE(D);
    KRK_HIP(hipStreamSynchronize(D->s_main));
    KRK_HIP(hipStreamSynchronize(D->s_a));
    KRK_HIP(hipStreamSynchronize(D->s_b));
    return KRK_OK;
}

uint64_t krk_num_pieces(uint64_t length, int64_t piece_length) {
    if (piece_length <= 0) return 0;
    return (length + (uint64_t)piece_length - 1) / (uint64_t)piece_length;
}

// ---------------------------------------------------------------- synthetic data
int krk_synth_fill_dev(uint8_t* dst_dev, uint64_t blob_idx, uint64_t offset, uint64_t n, int variant, void* stream) {
    if (!n) return KRK_OK;
    KRK_CHECK(dst_dev, KRK_EINVAL, "dst is NULL");
    KRK_DEVICE(D);
    hipStream_t s = pick(D, stream);
    const uint64_t GAMMA = 0x9E3779B97F4A7C15ULL;
    auto mix = [](uint64_t z) {
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        return z ^ (z >> 31);
    };
    const uint64_t seed = mix((0x4B52414B454EULL ^ blob_idx) + GAMMA);
    hipError_t e = timed(K_SYNTH, s, [&] { return launch_synth_fill(dst_dev, seed, offset, n, variant, s); });
    KRK_CHECK(e == hipSuccess, KRK_EHIP, "synth launch: %s", launch_error_text(e));
    return KRK_OK;
}

int krk_synth_fill_chunks_dev(const krk_chunk* chunks, uint64_t n, int variant, void* stream) {
    if (!n) return KRK_OK;
    KRK_CHECK(chunks, KRK_EINVAL, "chunks is NULL");
    KRK_CHECK(n <= 0xFFFFFFFFull / 16, KRK_EINVAL, "too many chunks");
    KRK_DEVICE(D);
    hipStream_t s = pick(D, stream);
    const uint64_t GAMMA = 0x9E3779B97F4A7C15ULL;
    auto mix = [](uint64_t z) {
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        return z ^ (z >> 31);
    };
    std::vector<SynthChunk> sc;
    sc.reserve(n);
    for (uint64_t i = 0; i < n; ++i) {
        if (!chunks[i].length) continue;
        KRK_CHECK(chunks[i].data, KRK_EINVAL, "chunk %llu: data is NULL", (unsigned long long)i);
        sc.push_back({const_cast<uint8_t*>(chunks[i].data), mix((0x4B52414B454EULL ^ chunks[i].blob) + GAMMA),
                      chunks[i].offset, chunks[i].length});
    }
    if (sc.empty()) return KRK_OK;
    void* d_sc = nullptr;
    int r = upload(D, sc.data(), sc.size() * sizeof(SynthChunk), &d_sc, s);
    if (r) return r;
    hipError_t e = timed(K_SYNTH, s, [&] {
        return launch_synth_fill_chunks(static_cast<const SynthChunk*>(d_sc), (uint32_t)sc.size(), variant, s);
    });
    scratch_free(D, d_sc, s);
    KRK_CHECK(e == hipSuccess, KRK_EHIP, "synth launch: %s", launch_error_text(e));
    return KRK_OK;
}

// ---------------------------------------------------------------- memory helpers
int krk_dev_alloc(uint64_t bytes, void** out) {
    KRK_CHECK(out, KRK_EINVAL, "out is NULL");
    KRK_DEVICE(D);
    (void)D;
    hipError_t e = hipMalloc(out, bytes ? bytes : 1);
    KRK_CHECK(e == hipSuccess, KRK_ENOMEM, "hipMalloc(%llu): %s", (unsigned long long)bytes, hipGetErrorString(e));
    return KRK_OK;
}
int krk_dev_free(void* p) {
    KRK_HIP(hipFree(p));
    return KRK_OK;
}
// Page-locked host memory for receive buffers and staged results.  Large buffers are
// anonymous mappings in transparent huge pages registered with HIP (pages placed by the
// default policy as the registration faults them in): the GPU's DMA reads them at the same
// rate as hipHostMalloc memory (57.2-57.6 GB/s) and host threads read them as fast as
// pageable memory (the library's host CRC: 216 vs 218 GB/s pageable, against 166 for
// hipHostMalloc blocks on the same box; interleaving the pages over the NUMA nodes cost as
// much, 165; tools/micro/host_mem_probe.cpp, profiles/r04/host_mem_probe*.jsonl).  Small
// buffers stay hipHostMalloc (one registration per call costs more than it saves).
namespace {
std::mutex g_host_mu;
std::unordered_map<void*, size_t> g_host_maps;  // registered mappings: address -> length
std::map<uintptr_t, size_t> g_host_ranges;      // every live krk_host_alloc block: start -> length

}  // namespace

extern "C++" {
namespace krk {
bool lib_pinned_range(const void* p, uint64_t n) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    std::lock_guard<std::mutex> g(g_host_mu);
    auto it = g_host_ranges.upper_bound(a);
    if (it == g_host_ranges.begin()) return false;
    --it;
    return a >= it->first && a + n <= it->first + it->second;
}
bool lib_pinned_block(const void* p, uint64_t n, uintptr_t* base) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    std::lock_guard<std::mutex> g(g_host_mu);
    auto it = g_host_ranges.upper_bound(a);
    if (it == g_host_ranges.begin()) return false;
    --it;
    if (a < it->first || a + n > it->first + it->second) return false;
    *base = it->first;
    return true;
}
}  // namespace krk
}
int krk_host_alloc(uint64_t bytes, void** out) {
    KRK_CHECK(out, KRK_EINVAL, "out is NULL");
    KRK_DEVICE(D);
    (void)D;
    constexpr uint64_t kLarge = 2ull << 20;
    if (bytes >= kLarge) {
        const size_t len = (bytes + kLarge - 1) & ~(kLarge - 1);
        void* p = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (p != MAP_FAILED) {
            madvise(p, len, MADV_HUGEPAGE);
            if (hipHostRegister(p, len, hipHostRegisterDefault) == hipSuccess) {
                std::lock_guard<std::mutex> g(g_host_mu);
                g_host_maps[p] = len;
                g_host_ranges[reinterpret_cast<uintptr_t>(p)] = len;
                *out = p;
                return KRK_OK;
            }
            (void)hipGetLastError();
            munmap(p, len);
        }
    }
    hipError_t e = hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault);
    KRK_CHECK(e == hipSuccess, KRK_ENOMEM, "hipHostMalloc(%llu): %s", (unsigned long long)bytes,
              hipGetErrorString(e));
    std::lock_guard<std::mutex> g(g_host_mu);
    g_host_ranges[reinterpret_cast<uintptr_t>(*out)] = bytes ? bytes : 1;
    return KRK_OK;
}
int krk_host_alloc_dma(uint64_t bytes, void** out) {
    KRK_CHECK(out, KRK_EINVAL, "out is NULL");
    KRK_DEVICE(D);
    (void)D;
    hipError_t e = hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault);
    KRK_CHECK(e == hipSuccess, KRK_ENOMEM, "hipHostMalloc(%llu): %s", (unsigned long long)bytes,
              hipGetErrorString(e));
    std::lock_guard<std::mutex> g(g_host_mu);
    g_host_ranges[reinterpret_cast<uintptr_t>(*out)] = bytes ? bytes : 1;
    return KRK_OK;
}
int krk_host_free(void* p) {
    size_t len = 0;
    {
        std::lock_guard<std::mutex> g(g_host_mu);
        g_host_ranges.erase(reinterpret_cast<uintptr_t>(p));
        auto it = g_host_maps.find(p);
        if (it != g_host_maps.end()) {
            len = it->second;
            g_host_maps.erase(it);
        }
    }
    if (len) {
        const hipError_t e = hipHostUnregister(p);
        munmap(p, len);
        KRK_HIP(e);
        return KRK_OK;
    }
    KRK_HIP(hipHostFree(p));
    return KRK_OK;
}
int krk_memcpy_h2d(void* dst, const void* src, uint64_t n) {
    KRK_DEVICE(D);
    (void)D;
    KRK_HIP(hipMemcpy(dst, src, n, hipMemcpyHostToDevice));
    return KRK_OK;
}
int krk_memcpy_d2h(void* dst, const void* src, uint64_t n) {
    KRK_DEVICE(D);
    (void)D;
    KRK_HIP(hipMemcpy(dst, src, n, hipMemcpyDeviceToHost));
    return KRK_OK;
}
int krk_memcpy_d2h_async(void* dst, const void* src, uint64_t n, void* stream) {
    KRK_DEVICE(D);
    KRK_HIP(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, pick(D, stream)));
    return KRK_OK;
}
int krk_stream_create(void** out) {
    KRK_CHECK(out, KRK_EINVAL, "out is NULL");
    KRK_DEVICE(D);
    (void)D;
    hipStream_t s;
    KRK_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *out = s;
    return KRK_OK;
}
int krk_device_pci_bus_id(char* out, uint32_t cap) {
    KRK_CHECK(out && cap >= 16, KRK_EINVAL, "device_pci_bus_id: a buffer of at least 16 bytes");
    KRK_DEVICE(D);
    KRK_HIP(hipDeviceGetPCIBusId(out, (int)cap, D->id));
    return KRK_OK;
}
int krk_device_cus(int* out) {
    KRK_CHECK(out, KRK_EINVAL, "out is NULL");
    KRK_DEVICE(D);
    *out = D->cus;
    return KRK_OK;
}
int krk_crc_launch_variant(int* out) {
    KRK_CHECK(out, KRK_EINVAL, "out is NULL");
    KRK_DEVICE(D);
    *out = D->crc_variant;
    return KRK_OK;
}
int krk_stream_create_prio(int priority, void** out) {
    KRK_CHECK(out, KRK_EINVAL, "out is NULL");
    KRK_DEVICE(D);
    (void)D;
    int least = 0, greatest = 0;  // HIP: numerically lower = higher priority
    KRK_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    const int p = priority < 0 ? greatest : priority > 0 ? least : (least + greatest) / 2;
    hipStream_t s;
    KRK_HIP(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, p));
    *out = s;
    return KRK_OK;
}
int krk_stream_destroy(void* s) {
    KRK_CHECK(s, KRK_EINVAL, "stream is NULL");
    const hipStream_t hs = static_cast<hipStream_t>(s);
    // The library state tied to the stream lives on the stream's own device, which need not
    // be this thread's.
    hipDevice_t owner = t_dev;
    KRK_HIP(hipStreamGetDevice(hs, &owner));
    const int saved = t_dev;
    int drc = KRK_OK;
    if (Device* D = device_id((int)owner, &drc)) forget_stream(D, hs);
    device_id(saved, &drc);  // the calling thread's current device is unchanged
    KRK_HIP(hipStreamDestroy(hs));
    return KRK_OK;
}
int krk_stream_sync(void* s) {
    KRK_DEVICE(D);
    KRK_HIP(hipStreamSynchronize(pick(D, s)));
    return KRK_OK;
}

int krk_event_create(void** out) {
    KRK_CHECK(out, KRK_EINVAL, "out is NULL");
    KRK_DEVICE(D);
    (void)D;
    hipEvent_t e;
    // blocking sync: a host thread waiting for a window (tens of ms) sleeps instead of
    // spinning a core of the process's CPU budget, which its hash threads need
    KRK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventBlockingSync));
    *out = e;
    return KRK_OK;
}
int krk_event_record(void* ev, void* stream) {
    KRK_CHECK(ev, KRK_EINVAL, "event is NULL");
    KRK_DEVICE(D);
    KRK_HIP(hipEventRecord(static_cast<hipEvent_t>(ev), pick(D, stream)));
    return KRK_OK;
}
int krk_event_query(void* ev, int* done) {
    KRK_CHECK(ev && done, KRK_EINVAL, "event_query: null argument");
    const hipError_t e = hipEventQuery(static_cast<hipEvent_t>(ev));
    KRK_CHECK(e == hipSuccess || e == hipErrorNotReady, KRK_EHIP, "event query: %s", hipGetErrorString(e));
    if (e == hipErrorNotReady) (void)hipGetLastError();
    *done = e == hipSuccess;
    return KRK_OK;
}
int krk_event_create_polling(void** out) {
    KRK_CHECK(out, KRK_EINVAL, "out is NULL");
    KRK_DEVICE(D);
    (void)D;
    hipEvent_t e;
    KRK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    *out = e;
    return KRK_OK;
}
int krk_stream_wait_event(void* stream, void* ev) {
    KRK_CHECK(ev, KRK_EINVAL, "event is NULL");
    KRK_DEVICE(D);
    KRK_HIP(hipStreamWaitEvent(pick(D, stream), static_cast<hipEvent_t>(ev), 0));
    return KRK_OK;
}
int krk_event_sync(void* ev) {
    KRK_CHECK(ev, KRK_EINVAL, "event is NULL");
    KRK_HIP(hipEventSynchronize(static_cast<hipEvent_t>(ev)));
    return KRK_OK;
}
int krk_event_destroy(void* ev) {
    if (ev) hipEventDestroy(static_cast<hipEvent_t>(ev));
    return KRK_OK;
}

int krk_set_timing(int on) {
    g_timing.store(on != 0);
    return KRK_OK;
}
int krk_kernel_stats(const char* kernel, uint64_t* launches, double* total_ms) {
    KRK_CHECK(kernel, KRK_EINVAL, "kernel is NULL");
    drain_timing();
    std::lock_guard<std::mutex> g(g_tmu);
    for (int k = 0; k < K_N; ++k)
        if (strcmp(kernel, kKernNames[k]) == 0) {
            if (launches) *launches = g_cnt[k];
            if (total_ms) *total_ms = g_ms[k];
            return KRK_OK;
        }
    set_error(KRK_EINVAL, "unknown kernel '%s'", kernel);
    return KRK_EINVAL;
}
int krk_sha_lanes_per_stream(uint64_t n_streams, int* lanes) {
    KRK_CHECK(lanes, KRK_EINVAL, "lanes is NULL");
    KRK_CHECK(n_streams <= 0xffffffffull, KRK_ERANGE, "too many streams");
    KRK_DEVICE(D);
    (void)D;
    *lanes = sha_lanes_for((uint32_t)n_streams);
    return KRK_OK;
}
int krk_device_clock_mhz(void* stream, double* mhz) {
    KRK_CHECK(mhz, KRK_EINVAL, "mhz is NULL");
    KRK_DEVICE(D);
    hipStream_t s = pick(D, stream);
    uint64_t* d_out = nullptr;
    KRK_HIP(scratch_alloc(D, &d_out, 32, s));
    uint64_t h[3] = {0, 0, 0};
    hipError_t e = launch_clock_probe(1u << 20, d_out, s);
    if (e == hipSuccess) e = hipMemcpyAsync(h, d_out, 24, hipMemcpyDeviceToHost, s);
    scratch_free(D, d_out, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    KRK_CHECK(e == hipSuccess, KRK_EHIP, "clock probe: %s", launch_error_text(e));
    KRK_CHECK(h[1] > 0, KRK_EHIP, "clock probe: no realtime ticks");
    *mhz = (double)h[0] / (double)h[1] * 100.0;
    return KRK_OK;
}

int krk_set_sha_plan(int plan) {
    KRK_CHECK(sha_plan_valid(plan), KRK_EINVAL, "unknown SHA-256 launch plan %d", plan);
    set_sha_plan(plan);
    return KRK_OK;
}
int krk_reset_kernel_stats(void) {
    drain_timing();
    std::lock_guard<std::mutex> g(g_tmu);
    for (int k = 0; k < K_N; ++k) { g_ms[k] = 0; g_cnt[k] = 0; }
    int cur = 0;
    hipGetDevice(&cur);
    for (int d = 0; d < kMaxDevs; ++d)
        if (g_origin[d]) {
            hipSetDevice(d);
            hipEventDestroy(g_origin[d]);
            g_origin[d] = nullptr;
        }
    hipSetDevice(cur);
    g_timeline.clear();
    return KRK_OK;
}
int krk_kernel_timeline(const char* kernel, krk_launch_rec* out, uint64_t cap, uint64_t* n) {
    KRK_CHECK(kernel && n, KRK_EINVAL, "kernel or n is NULL");
    int want = -1;
    for (int k = 0; k < K_N; ++k)
        if (strcmp(kernel, kKernNames[k]) == 0) want = k;
    KRK_CHECK(want >= 0, KRK_EINVAL, "unknown kernel '%s'", kernel);
    drain_timing();
    std::lock_guard<std::mutex> g(g_tmu);
    uint64_t m = 0;
    for (const auto& r : g_timeline) {
        if (r.k != want) continue;
        if (out && m < cap) out[m] = {r.dev, r.plan, r.units, r.t0, r.t1};
        ++m;
    }
    *n = m;
    return KRK_OK;
}
int krk_sha_plan_for(uint64_t n_streams, int* plan) {
    KRK_CHECK(plan, KRK_EINVAL, "plan is NULL");
    KRK_CHECK(n_streams <= 0xffffffffull, KRK_ERANGE, "too many streams");
    KRK_DEVICE(D);
    (void)D;
    *plan = sha_plan_for((uint32_t)n_streams);
    return KRK_OK;
}

}  // extern "C"
