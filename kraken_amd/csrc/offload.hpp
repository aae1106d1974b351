// offload.hpp -- what the library's other translation units use of the host offload: the planners' rates
// (rates.cpp; the planners are planner_math.hpp) and the executors on host threads (offload.cpp).  Not ABI.
#pragma once
#include "runtime.hpp"

namespace krk {

// Host threads the offload of a `mode` batch may use (krk_set_sha_host_offload; 0 = off).
int offload_threads(int mode = kOffDevice);
bool offload_auto();  // the offload's threads are KRK_OFFLOAD_AUTO (not set by the caller)

// rates.cpp
Rates planner_rates(Device* D);  // D == nullptr: the override or the nominal rates
int calibrate_device(Device* D);  // (re)measure D's rates now (krk_init, krk_planner_calibrate)
// One host thread's rates, bytes/s, each measured once per process on 16 MiB (no device
// needed): SHA-256 (x86 SHA extensions), CRC-32 (PCLMUL folding), memcpy.
double host_sha_rate();
double host_crc_rate();
double host_copy_rate();

// The calibration's device and pinned buffers, stream and events, kept until krk_shutdown:
// hipFree / hipHostFree wait for the whole device, i.e. for whatever other work is running
// on it when a later call re-measures.
struct CalBufs {
    hipStream_t s = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    uint8_t *d_in = nullptr, *d_dig = nullptr, *d_copy = nullptr, *h_copy = nullptr;
    uint32_t* d_state = nullptr;
    ShaJob* d_jobs = nullptr;
    uint32_t mmax = 0;
    void release();
};
// A device's planner calibration (once per device and process, or again on krk_planner_calibrate), in its pool.
struct RateCache {
    std::mutex cal_mu;  // one calibration of this device at a time
    CalBufs cal;
    std::mutex mu;  // measured, rates
    bool measured = false;
    Rates rates{};
};
RateCache& rate_cache(Device* D);

// offload.cpp.  Where offload_hash's chains start: chain j from byte start[j], from the GPU's
// midstate at note + 8 * slot[j] once the GPU has written it there (all eight words
// off kTailSentinel, or gpu_done complete), from the IV when start[j] == 0.
constexpr uint32_t kTailSentinel = 0xFFFFFFFFu;
struct TailSrc {
    const volatile uint32_t* note;
    const uint32_t* slot;
    const uint64_t* start;
    hipEvent_t gpu_done;
};
void offload_teardown(Device& D);  // krk_shutdown: the offload threads' streams and pinned buffers
void offload_hash_host(const std::vector<const uint8_t*>& ptrs, const std::vector<uint64_t>& lens, int threads,
                       uint8_t* out);
// kOffHostWhole: blob j's digest to out + 32 j and its piece sums (piece length plen[j])
// to sums[j][0 .. ceil(len / plen)), on up to `threads` threads; the SHA-256 pass and the
// CRC pass of a blob are separate tasks, longest first.
void offload_whole_host(const std::vector<const uint8_t*>& ptrs, const std::vector<uint64_t>& lens,
                        const std::vector<uint64_t>& plen, const std::vector<uint32_t*>& sums, int threads,
                        uint8_t* out);
int offload_whole_files(const std::vector<const char*>& paths, const std::vector<uint64_t>& lens,
                        const std::vector<uint64_t>& plen, const std::vector<uint32_t*>& sums, int threads,
                        uint8_t* out);
int offload_hash(Device* D, const std::vector<const uint8_t*>& ptrs, const std::vector<uint64_t>& lens, int threads,
                 hipEvent_t ready, uint8_t* out, const TailSrc* tail = nullptr);
int offload_store(Device* D, const std::vector<uint32_t>& idx, const uint8_t* dig, uint8_t* digests_dev,
                  hipStream_t s);

}  // namespace krk
