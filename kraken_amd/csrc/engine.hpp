// engine.hpp -- internal to libkraken_hip, not part of the ABI: what the streaming entry
// points (digester.cpp: krk_digester_*; piece_stream.cpp: krk_piece_stream_*,
// krk_crc32_update*) see of the per-device submission engine (engine.cpp) -- its staging
// slots, a request, the owner of requests in flight, and the calls that make, queue and
// await one.
#pragma once
#include <chrono>
#include <condition_variable>
#include <deque>

#include "runtime.hpp"

namespace krk {

using Clock = std::chrono::steady_clock;

// a knob's value (KRK_OP_ENV / KRK_AB_ENV, knobs.hpp) as a positive size, else dflt
inline size_t env_size(const char* v, size_t dflt) {
    if (!v || !*v) return dflt;
    const unsigned long long x = strtoull(v, nullptr, 10);
    return x ? (size_t)x : dflt;
}

// the CPUs this process may use: affinity AND the cgroup's CPU quota (the GPU boxes
// grant 16 CPUs' worth of quota over an affinity of 256 CPUs; counting the affinity
// alone kept AUTO digesters on the host up to 10,240 live instead of 640)
inline unsigned host_threads() { return (unsigned)std::max(1, host_cpu_budget()); }

// ------------------------------------------------------------------ slots
// Every engine owns a pool of fixed-size pinned staging slots, each with a device mirror,
// under a HARD pinned-bytes cap (KRK_SLOT_POOL_MB, krk_engine_set_pool_cap): a caller copies
// its bytes into a slot on its own thread; at the cap it waits for a release (backpressure).
// Slots are held only by requests in flight, which the engine always completes -- an owner
// keeps its partial data in its own host buffer between calls -- so the wait ends.
struct Slot {
    uint8_t* host = nullptr;      // pinned, mapped into the device's address space
    const uint8_t* mapped = nullptr;  // `host` as the device addresses it (zero-copy reads)
    uint8_t* dev = nullptr;       // device mirror (CRC requests are copied here)
    hipEvent_t h2d = nullptr;  // the last H2D of this slot
};

// 512 KiB slots: a digester that misses a launch falls one launch behind for good, so the
// launch should be short; 256 concurrent digesters from native threads, same box,
// interleaved (tests/native/digesters.cpp): 2 MiB slots with 4 in flight 8.8-12.6 GB/s,
// 512 KiB with 8 in flight 11.1-14.2 GB/s.
constexpr size_t kSlotBytes = 512u << 10;
static_assert(kSlotBytes % 64 == 0, "a slot holds whole SHA-256 blocks");
// Requests per digester / piece stream in flight.  With 512 KiB slots a launch of 256
// streams is ~9 ms, so 8 in flight keep ~70 ms of each owner's bytes ahead of the device:
// an owner whose writer thread was descheduled for a while still makes the next launch.
constexpr size_t kOwnerInflight = 8;

class SlotPool {
  public:
    size_t S = 0;  // bytes per slot (multiple of 64)

    void init(size_t slot_bytes, size_t cap_bytes) {
        S = slot_bytes;
        set_cap(cap_bytes);
    }

    // The hard cap on pinned bytes (at least one chunk).  Lowering it never frees
    // slots already allocated; it stops further growth.
    void set_cap(size_t cap_bytes) {
        {
            std::lock_guard<std::mutex> g(mu_);
            cap_ = std::max(cap_bytes, S * kPerChunk);
        }
        cv_.notify_all();
    }

    // A free slot: grows the pool one chunk at a time while under the cap, else waits
    // for a release (backpressure).  Call with the owning device current.
    Slot* acquire(int* rc) {
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            if (!free_.empty()) {
                Slot* s = free_.back();
                free_.pop_back();
                *rc = KRK_OK;
                return s;
            }
            if (allocated_ + S * kPerChunk <= cap_) {
                *rc = grow();
                if (*rc) return nullptr;
                continue;
            }
            ++waits_;
            cv_.wait(lk);
        }
    }

    // A slot for an owner to fill in place between calls, only while more than `reserve`
    // slots stay free or growable: the reserve is left to submissions (which block), so
    // slots held by idle owners can never starve the requests that release slots.
    Slot* try_acquire(size_t reserve) {
        std::lock_guard<std::mutex> g(mu_);
        const size_t growable = cap_ > allocated_ ? (cap_ - allocated_) / S : 0;
        if (free_.size() + growable <= reserve) return nullptr;
        if (free_.empty() && grow() != KRK_OK) return nullptr;
        Slot* s = free_.back();
        free_.pop_back();
        return s;
    }
    size_t reserve() {
        std::lock_guard<std::mutex> g(mu_);
        return std::max<size_t>(kPerChunk, cap_ / S / 4);
    }

    void release(Slot* s) {
        if (!s) return;
        {
            std::lock_guard<std::mutex> g(mu_);
            free_.push_back(s);
        }
        cv_.notify_one();
    }

    size_t pinned_bytes() {
        std::lock_guard<std::mutex> g(mu_);
        return allocated_;
    }
    size_t cap() {
        std::lock_guard<std::mutex> g(mu_);
        return cap_;
    }
    uint64_t waits() {
        std::lock_guard<std::mutex> g(mu_);
        return waits_;
    }

    void destroy() {
        std::lock_guard<std::mutex> g(mu_);
        for (auto& c : chunks_)
            for (int i = 0; i < kPerChunk; ++i)
                if (c[i].h2d) {
                    hipEventSynchronize(c[i].h2d);
                    hipEventDestroy(c[i].h2d);
                }
        for (void* p : host_) hipHostFree(p);
        for (void* p : dev_) hipFree(p);
        chunks_.clear();
        host_.clear();
        dev_.clear();
        free_.clear();
        allocated_ = 0;
    }

  private:
    static constexpr int kPerChunk = 16;
    std::mutex mu_;
    std::condition_variable cv_;
    std::vector<Slot*> free_;
    std::vector<std::unique_ptr<Slot[]>> chunks_;
    std::vector<void*> host_, dev_;
    size_t allocated_ = 0;
    size_t cap_ = 0;
    uint64_t waits_ = 0;

    // With mu_ held.  Everything is created before anything is published, and a
    // failure undoes what this call made: the pool never holds a half-built chunk.
    int grow() {
        const size_t bytes = S * kPerChunk;
        hipEvent_t ev[kPerChunk] = {};
        for (int i = 0; i < kPerChunk; ++i) {
            const hipError_t e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
            if (e != hipSuccess) {
                for (int j = 0; j < i; ++j) hipEventDestroy(ev[j]);
                set_error(KRK_EHIP, "engine: slot events: %s", hipGetErrorString(e));
                return KRK_EHIP;
            }
        }
        void *h = nullptr, *d = nullptr, *hm = nullptr;
        // coherent: the SHA-256 kernel reads a slot straight over PCIe (no H2D copy), and a
        // reused slot must never be served from a stale GPU cache line
        if (hipHostMalloc(&h, bytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) h = nullptr;
        else memset(h, 0, bytes);
        if (h && hipHostGetDevicePointer(&hm, h, 0) != hipSuccess) hm = nullptr;
        if (h && hm && hipMalloc(&d, bytes) != hipSuccess) d = nullptr;
        if (!h || !hm || !d) {
            if (h) hipHostFree(h);
            for (auto& e : ev) hipEventDestroy(e);
            set_error(KRK_ENOMEM, "engine: %s staging slots (%zu bytes)", h ? "device" : "pinned host", bytes);
            return KRK_ENOMEM;
        }
        std::unique_ptr<Slot[]> c(new Slot[kPerChunk]);
        for (int i = 0; i < kPerChunk; ++i) {
            c[i].host = static_cast<uint8_t*>(h) + i * S;
            c[i].mapped = static_cast<const uint8_t*>(hm) + i * S;
            c[i].dev = static_cast<uint8_t*>(d) + i * S;
            c[i].h2d = ev[i];
            free_.push_back(&c[i]);
        }
        host_.push_back(h);
        dev_.push_back(d);
        chunks_.push_back(std::move(c));
        allocated_ += bytes;
        return KRK_OK;
    }
};

// ------------------------------------------------------------------ requests
struct Waiter {
    std::mutex mu;
    std::condition_variable cv;
};

struct Req {
    Slot* slot = nullptr;  // released when the request completes
    uint64_t len = 0;
    uint64_t seq = 0;             // order of the slot's H2D on the copy stream
    const void* owner = nullptr;  // ordering key (SHA: one request per owner per launch)
    Waiter* w = nullptr;
    Clock::time_point t_submit;
    // SHA: the owner's state-table row, bytes absorbed before this request; final =
    // pad and write the digest (the state row is left as it was: no reset).
    uint32_t row = 0;
    uint64_t prefix = 0;
    bool final = false;
    uint8_t digest[32] = {};
    // CRC: stream offset of the slot's first byte and the piece length (0: the request
    // is one portion); crcs[k] = crc32 of portion k as an independent message.
    uint64_t off = 0;
    uint64_t P = 0;
    std::vector<uint32_t> crcs;
    void (*on_done)(Req*) = nullptr;  // runs on the completer thread, in FIFO order
    void* ctx = nullptr;
    int rc = KRK_OK;
    std::string err;
    bool done = false;
};

// ------------------------------------------------------------------ the engine's calls
// The engine's two queues.  Where a request's bytes are read from is a property of its queue:
//  * kSha: the SHA-256 kernel loads the pinned slot itself over PCIe (slot->mapped, zero-copy);
//    nothing is staged at submission.  The only source kept: on MI355X, same box, 256 / 640 /
//    1,024 digesters ran 14.1 / 29.6 / 21.6 GB/s, against 12.0 / 20.6 / 20.4 with one gather
//    launch per batch into the device mirrors (a batch is formed just before the running one
//    ends, so its gather cannot overlap the previous kernel) -- DESIGN.md 4.6;
//  * kCrc: the slot is copied to its device mirror (slot->dev) on the engine's copy stream at
//    submission, and the launch waits for the last-staged copy.
enum class Kind { kSha, kCrc };

struct Engine;
// The engine of device `id`, started on first use.
Engine* engine_of(int id, int* rc);
SlotPool& engine_pool(Engine* E);
std::atomic<int64_t>& engine_live_digesters(Engine* E);  // GPU digesters placed on E
// KRK_ENGINE_TRACE: one stderr line for a submission step that held its caller > 5 ms.
void trace_slow(Engine* E, const char* what, Clock::time_point t0);
// A request of queue `k` over `len` bytes: in `sl`, a slot its owner filled in place (handed
// over to the request, also when this fails), else copied from `src` into a fresh slot on
// this thread.
int make_req(Engine* E, Kind k, Slot* sl, const uint8_t* src, uint64_t len, Req** out);
void submit(Engine* E, Kind k, Req* r);
// Wait for r, return its status (the engine's error text moves to this thread).
int wait_req(Req* r);
// An owner's row of the engine's SHA state and digest tables.
uint32_t row_acquire(Engine* E, int* rc);
void row_release(Engine* E, uint32_t row);
// Host buffers (pool.S bytes, pageable) that digesters and piece streams fill between
// submissions, recycled so that a new owner's first bytes do not page-fault a fresh
// allocation (256 new uploads: half a GiB of first-touch faults).
std::unique_ptr<uint8_t[]> pend_acquire(Engine* E);
void pend_release(Engine* E, std::unique_ptr<uint8_t[]> b);
// Requests a digester may keep in flight: kOwnerInflight, but no more than its share of the
// slot pool beyond the submissions' reserve, so that many live digesters (the crossover
// sweep: 1,024+) do not fill the hard pinned cap with the few that got there first while
// the others' writers wait at it (then fewer streams make each launch).
size_t owner_inflight(Engine* E);

// ------------------------------------------------------------------ owners
// Something that keeps requests in flight on an engine: a Digester, a piece stream, one
// crc32.Update call.  The first failed request poisons it: every later call returns that
// status with that text.
struct Owner {
    Engine* E = nullptr;  // null: host placement
    Waiter w;
    std::deque<Req*> inflight;  // submission order
    int err = KRK_OK;
    std::string err_msg;

    int status() const {
        if (err) t_err = err_msg;
        return err;
    }
    void fail(int rc) {  // with rc's text in t_err
        if (rc && !err) {
            err = rc;
            err_msg = t_err;
        }
    }
    void push(Kind k, Req* r) {
        r->w = &w;
        inflight.push_back(r);
        submit(E, k, r);
    }
    // Wait until at most `keep` requests are in flight; hook(r, rc) sees each one retired.
    template <class Hook>
    int drain(size_t keep, Hook&& hook) {
        while (inflight.size() > keep) {
            Req* r = inflight.front();
            const int rc = wait_req(r);
            inflight.pop_front();
            hook(r, rc);
            delete r;
            fail(rc);
        }
        return status();
    }
    int drain(size_t keep) {
        return drain(keep, [](Req*, int) {});
    }
};

}  // namespace krk
