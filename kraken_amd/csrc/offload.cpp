// offload.cpp -- host offload of the longest SHA-256 chains of a batch
// (krk_set_sha_host_offload; used by krk_sha256_dev / krk_metainfo_digest_dev on blobs in
// HBM and by krk_sha256_host / krk_metainfo_digest_host on blobs in host memory).
//
// SHA-256 is one sequential chain per blob (core/digester.go:28-72).  A GPU stream runs
// at ~59 MB/s (eight lanes), one x86 core with the SHA extensions at
// ~2 GB/s.  A batch whose longest blobs dominate (C1: one 1 GiB blob; the log-uniform
// regen batches of C5) therefore finishes sooner when host threads take the longest
// chains -- reading them out of HBM through pinned double buffers -- while the GPU
// hashes the rest and the piece CRCs of every blob.  The planner picks how many of the
// longest blobs go to the host by minimising max(GPU time, host time); a batch of equal
// blobs (C2) gains nothing (the GPU's chain is the same blob length) and stays on the GPU.
// Blobs in host memory are worked on in place, never uploaded; krk_metainfo_digest_host's
// host blobs get their piece sums on the host too, which takes their bytes off the host
// link -- C2 end-to-end, link-bound, then hands the host the blobs the link would carry
// past the GPU's own chain time.
#include <fcntl.h>
#include <unistd.h>

#include <chrono>
#include <thread>

#include "offload.hpp"

namespace krk {

namespace {

// Host threads of the offload: KRK_OFFLOAD_AUTO (the default) = the CPUs this call may use
// for blobs read out of HBM (their D2H copies need no host CPU), a quarter of them for
// host-resident batches, whose windows need the rest as copy threads (C2 end-to-end: 4 of
// 16 threads 55.5 GB/s, 8 54.4-55.2, 16 49.9).  0 = off, n = n threads.
std::atomic<int> g_off_threads{KRK_OFFLOAD_AUTO};

// A D2H copy (a multiple of 64; 16 MiB measured slower beside the C3 windows).
constexpr uint64_t kD2hChunk = 8ull << 20;

}  // namespace

// One offload thread's copy resources: buffer b is filled on stream s[b].  Completion is
// awaited with hipStreamSynchronize, not an event: an event record is a packet on the
// stream's hardware queue, and with more streams than hardware queues (4) it can sit
// behind the batch's own long SHA-256 kernel (tools/micro/d2h_probe.hip: copy kernels
// on 4 of 16 streams waited 1 s for a 1 s kernel on a fifth), while the DMA copies
// themselves do not wait for it.
struct Worker {
    static constexpr int depth = 2;
    hipStream_t s[depth] = {};
    uint8_t* buf[depth] = {};
    void release() {
        for (int b = 0; b < depth; ++b) {
            if (s[b]) hipStreamSynchronize(s[b]), hipStreamDestroy(s[b]);
            if (buf[b]) hipHostFree(buf[b]);
        }
        *this = Worker{};
    }
    int make() {
        for (int b = 0; b < depth; ++b) {
            const hipError_t es = hipStreamCreateWithFlags(&s[b], hipStreamNonBlocking);
            if (es == hipSuccess && hipHostMalloc((void**)&buf[b], kD2hChunk, hipHostMallocDefault) == hipSuccess)
                continue;
            release();
            KRK_CHECK(es == hipSuccess, KRK_EHIP, "sha256 host offload: stream: %s", hipGetErrorString(es));
            KRK_CHECK(false, KRK_ENOMEM, "sha256 host offload: pinned buffers");
        }
        return KRK_OK;
    }
    bool issue(uint64_t c, const uint8_t* src, uint64_t m) {
        return m == 0 || hipMemcpyAsync(buf[c % depth], src, m, hipMemcpyDeviceToHost, s[c % depth]) == hipSuccess;
    }
    const uint8_t* wait(uint64_t c) { return hipStreamSynchronize(s[c % depth]) ? nullptr : buf[c % depth]; }
    void drain() { hipStreamSynchronize(s[0]), hipStreamSynchronize(s[1]); }
};

// A resumer (krk_sha256_resume_dev_on_host): one copy stream, `depth` pinned buffers and
// their events -- copies run up to depth - 1 chunks ahead of the hash, so a copy held
// back a few ms behind another stream's packet in a shared hardware queue does not stall it.
struct Resumer {
    static constexpr int depth = 4;
    hipStream_t s = nullptr;
    uint8_t* buf[depth] = {};
    hipEvent_t ev[depth] = {};
    void release() {
        if (s) hipStreamSynchronize(s), hipStreamDestroy(s);
        for (int b = 0; b < depth; ++b) {
            if (buf[b]) hipHostFree(buf[b]);
            if (ev[b]) hipEventDestroy(ev[b]);
        }
        *this = Resumer{};
    }
    int make() {
        bool ok = hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess;
        for (int b = 0; ok && b < depth; ++b)
            ok = hipHostMalloc(reinterpret_cast<void**>(&buf[b]), kD2hChunk, hipHostMallocDefault) == hipSuccess &&
                 hipEventCreateWithFlags(&ev[b], hipEventDisableTiming) == hipSuccess;
        if (!ok) release();
        KRK_CHECK(ok, KRK_ENOMEM, "sha256 resume: pinned buffers / stream");
        return KRK_OK;
    }
    bool issue(uint64_t c, const uint8_t* src, uint64_t m) {
        return (m == 0 || hipMemcpyAsync(buf[c % depth], src, m, hipMemcpyDeviceToHost, s) == hipSuccess) &&
               hipEventRecord(ev[c % depth], s) == hipSuccess;
    }
    const uint8_t* wait(uint64_t c) { return hipEventSynchronize(ev[c % depth]) ? nullptr : buf[c % depth]; }
    void drain() { hipStreamSynchronize(s); }
};

struct Times {  // a thread's seconds waiting for copies (and the GPU's midstate), hashing, issuing, awaiting `ready`
    double wait = 0, hash = 0, issue = 0, ready = 0;
};
using Clock = std::chrono::steady_clock;
static double since(Clock::time_point a) { return std::chrono::duration<double>(Clock::now() - a).count(); }

// One chain, L bytes from device address src, continued from h (`absorbed` bytes in) on the calling thread over
// pipe P: the copies run Pipe::depth - 1 chunks ahead of SHA-NI over each; after_prime() runs between the first
// copies' issue and the first wait (the tail handoff awaits the GPU's midstate there, while the first chunk comes
// down).  The last chunk finalises into digest when `final`.  On failure no copy is left in flight into the buffers.
template <class Pipe, class Hook>
static bool walk_chain(Pipe& P, Times& T, uint32_t h[8], uint64_t absorbed, const uint8_t* src, uint64_t L, bool final,
                       uint8_t* digest, Hook&& after_prime) {
    const uint64_t nch = std::max<uint64_t>(1, (L + kD2hChunk - 1) / kD2hChunk);
    auto issue = [&](uint64_t c) {
        const auto ti = Clock::now();
        const bool ok = P.issue(c, src + c * kD2hChunk, std::min(kD2hChunk, L - c * kD2hChunk));
        T.issue += since(ti);
        return ok;
    };
    bool ok = true;
    uint64_t issued = 0;
    for (; ok && issued < std::min<uint64_t>(nch, Pipe::depth - 1); ++issued) ok = issue(issued);
    ok = ok && after_prime();
    for (uint64_t c = 0; ok && c < nch; ++c) {
        if (issued < nch) ok = issue(issued++);  // into the buffer hashed at c - 1
        const auto tw = Clock::now();
        const uint8_t* p = ok ? P.wait(c) : nullptr;
        if (!(ok = p != nullptr)) break;
        const auto th = Clock::now();
        T.wait += std::chrono::duration<double>(th - tw).count();
        const uint64_t m = std::min(kD2hChunk, L - c * kD2hChunk);
        if (c + 1 < nch || !final) {
            host_sha256_blocks(h, p, m / 64);
            absorbed += m;
        } else {
            host_sha256_final(h, absorbed, p, m, digest);
        }
        T.hash += since(th);
    }
    if (!ok) P.drain();
    return ok;
}

// T = min(max(threads, 1), items) threads run work(): T - 1 started here and the caller.
template <class F>
static void run_threads(size_t items, int threads, F&& work) {
    const int T = (int)std::min<size_t>((size_t)std::max(threads, 1), items);
    std::vector<std::thread> pool;
    for (int t = 1; t < T; ++t) pool.emplace_back(work);
    work();
    for (auto& th : pool) th.join();
}

// Per device: the free worker sets and resumers, and the planner calibration.  Each offload phase takes a set of
// worker resources of its own (two streams + two pinned buffers a thread), so concurrent callers on one device
// (several krk_sha256_dev callers, *_multi workers sharing a GPU) hash at the same time.
struct OffloadPool {
    std::mutex mu;
    std::vector<std::vector<Worker>> free_sets;
    std::vector<Resumer> free_resumers;
    RateCache rate;
};

// A pooled resource (or a fresh, empty one) for one call: it goes back to the pool whatever happens in between.
template <class X>
struct Lease {
    std::mutex& mu;
    std::vector<X>& free;
    X x{};
    Lease(std::mutex& m, std::vector<X>& f) : mu(m), free(f) {
        std::lock_guard<std::mutex> g(mu);
        if (free.empty()) return;
        x = std::move(free.back());
        free.pop_back();
    }
    ~Lease() {
        std::lock_guard<std::mutex> g(mu);
        free.push_back(std::move(x));
    }
};

static OffloadPool* pool_of(Device* D) {
    std::lock_guard<std::mutex> g(D->offload_mu);
    if (!D->offload) D->offload = new OffloadPool();
    return D->offload;
}
RateCache& rate_cache(Device* D) { return pool_of(D)->rate; }

bool offload_auto() { return g_off_threads.load(std::memory_order_relaxed) == KRK_OFFLOAD_AUTO; }

int offload_threads(int mode) {
    const int t = g_off_threads.load(std::memory_order_relaxed);
    if (t != KRK_OFFLOAD_AUTO) return t;
    const int budget = host_threads_for_call();
    return mode == kOffDevice ? budget : std::max(1, budget / 4);
}

// Hash blobs (device pointers, lengths) on up to `threads` host threads; digest j to
// out + 32 j.  The D2H copies start once `ready` (recorded on the caller's stream: the
// bytes may still be being written there) has completed.  Blocks until all are hashed.
int offload_hash(Device* D, const std::vector<const uint8_t*>& ptrs, const std::vector<uint64_t>& lens, int threads,
                 hipEvent_t ready, uint8_t* out, const TailSrc* tail) {
    if (ptrs.empty()) return KRK_OK;
    OffloadPool& P = *pool_of(D);
    // at least one thread: the knob may have been lowered since the plan was made
    const int T = (int)std::min<size_t>((size_t)std::max(threads, 1), ptrs.size());
    Lease<std::vector<Worker>> lease(P.mu, P.free_sets);
    std::vector<Worker>& set = lease.x;
    while ((int)set.size() < T) {
        Worker w;
        if (int r = w.make()) return r;
        set.push_back(w);
    }
    std::atomic<size_t> next{0};
    std::atomic<int> err{0};
    static const bool trace = KRK_OP_ENV("KRK_TRACE") && atoi(KRK_OP_ENV("KRK_TRACE")) > 0;
    std::vector<Times> times(T);
    const auto t_start = Clock::now();
    std::vector<std::thread> pool;
    for (int t = 0; t < T; ++t)
        pool.emplace_back([&, t] {
            // The host waits for `ready` (the caller's stream up to the call; the batch's own
            // kernels come after it): a stream wait packet could queue behind those kernels.
            if (hipSetDevice(D->id) != hipSuccess || hipEventSynchronize(ready) != hipSuccess) {
                err.store(1);
                return;
            }
            for (size_t j; !err.load() && (j = next.fetch_add(1)) < ptrs.size();) {
                const uint64_t st = tail ? tail->start[j] : 0;  // the GPU's prefix of the chain
                uint32_t h[8];
                memcpy(h, kIV, sizeof h);
                auto midstate = [&] {
                    if (!st) return true;
                    const volatile uint32_t* w = tail->note + 8 * (uint64_t)tail->slot[j];
                    const auto tw = Clock::now();
                    bool ok = true;
                    for (;;) {
                        bool all = true;
                        for (int k = 0; k < 8 && all; ++k) all = w[k] != kTailSentinel;
                        if (all) break;
                        const hipError_t q = hipEventQuery(tail->gpu_done);
                        if (q == hipSuccess) break;  // the kernel has ended: the words are final
                        if (q != hipErrorNotReady) {
                            ok = false;
                            break;
                        }
                        std::this_thread::sleep_for(std::chrono::microseconds(20));
                    }
                    for (int k = 0; k < 8; ++k) h[k] = w[k];
                    times[t].wait += since(tw);
                    return ok;
                };
                if (!walk_chain(set[t], times[t], h, st, ptrs[j] + st, lens[j] - st, true, out + 32 * j, midstate))
                    err.store(1);
            }
        });
    for (auto& th : pool) th.join();
    if (trace) {
        uint64_t bytes = 0;
        for (uint64_t L : lens) bytes += L;
        double w = 0, h = 0;
        for (const Times& x : times) w += x.wait, h += x.hash;
        fprintf(stderr, "krk_trace sha_offload: threads=%d blobs=%zu bytes=%llu wall=%.3fs wait=%.3fs hash=%.3fs (thread sums)\n",
                T, ptrs.size(), (unsigned long long)bytes, since(t_start), w, h);
    }
    KRK_CHECK(!err.load(), KRK_EHIP, "sha256 host offload: device-to-host copy failed");
    return KRK_OK;
}

// The calling thread's seconds in krk_sha256_resume_dev_on_host / krk_sha256_resume_host
// (krk_sha256_resume_stats, krk_sha256_resume_stats2).
static thread_local Times t_resume;

// One chain continued on the calling thread from device bytes (krk_sha256_resume_dev_on_host)
// over a resumer of the device's pool.
static int resume_on_host(Device* D, uint32_t h[8], uint64_t absorbed, const uint8_t* src, uint64_t L, bool final,
                          uint8_t* digest, hipEvent_t ready) {
    OffloadPool& P = *pool_of(D);
    Lease<Resumer> lease(P.mu, P.free_resumers);
    Resumer& R = lease.x;
    if (!R.s)
        if (int r = R.make()) return r;
    if (ready) {
        const auto tr = Clock::now();
        KRK_HIP(hipEventSynchronize(ready));
        t_resume.ready += since(tr);
    }
    const bool ok = walk_chain(R, t_resume, h, absorbed, src, L, final, digest, [] { return true; });
    KRK_CHECK(ok, KRK_EHIP, "sha256 resume: device-to-host copy failed");
    return KRK_OK;
}

void offload_teardown(Device& D) {  // krk_shutdown: no offload phase is running (contract)
    OffloadPool* P = D.offload;
    if (!P) return;
    for (auto& set : P->free_sets)
        for (Worker& w : set) w.release();
    for (Resumer& r : P->free_resumers) r.release();
    P->rate.cal.release();
    delete P;
    D.offload = nullptr;
}

// Hash host-resident blobs on up to `threads` threads (next-longest first); digest j to
// out + 32 j.
void offload_hash_host(const std::vector<const uint8_t*>& ptrs, const std::vector<uint64_t>& lens, int threads,
                       uint8_t* out) {
    std::atomic<size_t> next{0};
    run_threads(ptrs.size(), threads, [&] {
        for (size_t j; (j = next.fetch_add(1)) < ptrs.size();) {
            HostCpuToken tok;  // a blob at a time under the process's CPU tokens
            uint32_t h[8];
            memcpy(h, kIV, sizeof h);
            host_sha256_final(h, 0, ptrs[j], lens[j], out + 32 * j);
        }
    });
}

void offload_whole_host(const std::vector<const uint8_t*>& ptrs, const std::vector<uint64_t>& lens,
                        const std::vector<uint64_t>& plen, const std::vector<uint32_t*>& sums, int threads,
                        uint8_t* out) {
    // Task t: blob t / 2, its SHA-256 pass (even t) or its piece-CRC pass (odd t), in
    // order of cost (the CRC pass runs ~6x the SHA-256 rate on one core).
    const double rs = host_sha_rate(), rc = host_crc_rate();
    std::vector<std::pair<double, size_t>> tasks;
    tasks.reserve(2 * ptrs.size());
    for (size_t j = 0; j < ptrs.size(); ++j) {
        tasks.push_back({lens[j] / rs, 2 * j});
        if (lens[j]) tasks.push_back({lens[j] / rc, 2 * j + 1});  // an empty blob has no pieces
    }
    std::stable_sort(tasks.begin(), tasks.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
    std::atomic<size_t> next{0};
    run_threads(tasks.size(), threads, [&] {
        for (size_t q; (q = next.fetch_add(1)) < tasks.size();) {
            HostCpuToken tok;  // a task at a time under the process's CPU tokens
            const size_t j = tasks[q].second / 2;
            const uint8_t* p = ptrs[j];
            const uint64_t L = lens[j];
            if (tasks[q].second % 2 == 0) {
                uint32_t h[8];
                memcpy(h, kIV, sizeof h);
                host_sha256_final(h, 0, p, L, out + 32 * j);
            } else {
                // core/metainfo.go:157-179: piece i = bytes [iP, min((i+1)P, L)), crc32 each
                const uint64_t P = plen[j];
                for (uint64_t o = 0, i = 0; o < L; o += P, ++i) sums[j][i] = host_crc32_update(0, p + o, std::min(P, L - o));
            }
        }
    });
}

// kOffHostFiles: file j read once in 1 MiB chunks, each chunk hashed (SHA-256) and its
// piece portions CRC'd while it is in the cache; digest to out + 32 j, sums to sums[j].
// Errors keep the reference's texts ("open <path>: ...", "read blob: <path>: ...").
int offload_whole_files(const std::vector<const char*>& paths, const std::vector<uint64_t>& lens,
                        const std::vector<uint64_t>& plen, const std::vector<uint32_t*>& sums, int threads,
                        uint8_t* out) {
    constexpr size_t kChunk = size_t(1) << 20;  // a multiple of 64: only the last chunk is partial
    std::atomic<size_t> next{0};
    std::atomic<bool> failed{false};
    std::mutex emu;
    int rc = KRK_OK;
    std::string msg;
    auto fail = [&](int code, const std::string& m) {
        std::lock_guard<std::mutex> g(emu);
        if (!rc) {
            rc = code;
            msg = m;
        }
        failed = true;
    };
    run_threads(paths.size(), threads, [&] {
        std::vector<uint8_t> buf(kChunk);
        for (size_t j; !failed && (j = next.fetch_add(1)) < paths.size();) {
            HostCpuToken tok;  // a file at a time under the process's CPU tokens
            const int fd = open(paths[j], O_RDONLY | O_CLOEXEC);
            if (fd < 0) {
                fail(KRK_EIO, std::string("open ") + paths[j] + ": " + strerror(errno));
                return;
            }
            const uint64_t L = lens[j], P = plen[j];
            uint32_t h[8];
            memcpy(h, kIV, sizeof h);
            uint32_t crc = 0;
            uint64_t pos = 0, in_piece = 0, piece = 0;
            bool ok = true;
            do {
                const size_t m = (size_t)std::min<uint64_t>(kChunk, L - pos);
                for (size_t got = 0; got < m;) {
                    const ssize_t g = pread(fd, buf.data() + got, m - got, (off_t)(pos + got));
                    if (g < 0 && errno == EINTR) continue;
                    if (g <= 0) {
                        fail(KRK_EIO, std::string("read blob: ") + paths[j] + ": " +
                                          (g < 0 ? strerror(errno) : "unexpected EOF"));
                        ok = false;
                        break;
                    }
                    got += (size_t)g;
                }
                if (!ok) break;
                for (size_t q = 0; q < m;) {  // core/metainfo.go:157-179 over this chunk
                    const size_t take = (size_t)std::min<uint64_t>(m - q, P - in_piece);
                    crc = host_crc32_update(crc, buf.data() + q, take);
                    q += take;
                    in_piece += take;
                    if (in_piece == P) {
                        sums[j][piece++] = crc;
                        crc = 0;
                        in_piece = 0;
                    }
                }
                if (pos + m < L) host_sha256_blocks(h, buf.data(), m / 64);
                else host_sha256_final(h, pos, buf.data(), m, out + 32 * j);
                pos += m;
            } while (pos < L);
            if (ok && in_piece) sums[j][piece] = crc;
            close(fd);
            if (!ok) return;
        }
    });
    if (rc) set_error(rc, "%s", msg.c_str());
    return rc;
}

// Write host-computed digests into digests_dev (record j: 4-byte blob index, 32-byte
// digest) on stream s: one upload + one scatter launch.
int offload_store(Device* D, const std::vector<uint32_t>& idx, const uint8_t* dig, uint8_t* digests_dev,
                  hipStream_t s) {
    if (idx.empty()) return KRK_OK;
    std::vector<uint8_t> rec(idx.size() * 36);
    for (size_t j = 0; j < idx.size(); ++j) {
        memcpy(&rec[36 * j], &idx[j], 4);
        memcpy(&rec[36 * j + 4], dig + 32 * j, 32);
    }
    void* d = nullptr;
    int r = upload(D, rec.data(), rec.size(), &d, s);
    if (r) return r;
    hipError_t e = launch_digest_scatter(static_cast<const uint8_t*>(d), (uint32_t)idx.size(), digests_dev, s);
    scratch_free(D, d, s);
    KRK_CHECK(e == hipSuccess, KRK_EHIP, "digest scatter launch: %s", launch_error_text(e));
    return KRK_OK;
}

}  // namespace krk

using namespace krk;

extern "C" {

int krk_set_sha_host_offload(int threads) {
    KRK_CHECK(threads == KRK_OFFLOAD_AUTO || (threads >= 0 && threads <= 1024), KRK_EINVAL,
              "host offload threads %d outside -1 (auto), 0..1024", threads);
    g_off_threads.store(threads);
    return KRK_OK;
}

int krk_sha_host_offload(int* threads) {
    KRK_CHECK(threads, KRK_EINVAL, "threads is NULL");
    *threads = g_off_threads.load();
    return KRK_OK;
}

int krk_sha_offload_geometry(uint64_t* d2h_chunk_bytes, uint32_t* worker_depth, uint32_t* resumer_depth) {
    KRK_CHECK(d2h_chunk_bytes && worker_depth && resumer_depth, KRK_EINVAL, "sha_offload_geometry: null argument");
    *d2h_chunk_bytes = kD2hChunk;
    *worker_depth = Worker::depth;
    *resumer_depth = Resumer::depth;
    return KRK_OK;
}

static int resume_args(const uint32_t* state8, uint64_t absorbed, const uint8_t* data, uint64_t n, int final,
                       const uint8_t* digest32) {
    KRK_CHECK(state8, KRK_EINVAL, "sha256_resume: state is NULL");
    KRK_CHECK(n == 0 || data, KRK_EINVAL, "sha256_resume: data is NULL");
    KRK_CHECK(absorbed % 64 == 0, KRK_EINVAL, "sha256_resume: absorbed bytes not a multiple of 64");
    KRK_CHECK(final || n % 64 == 0, KRK_EINVAL, "sha256_resume: a non-final run must be whole 64-byte blocks");
    KRK_CHECK(!final || digest32, KRK_EINVAL, "sha256_resume: digest is NULL");
    return KRK_OK;
}

int krk_sha256_resume_dev_on_host(uint32_t* state8, uint64_t absorbed, const uint8_t* data_dev, uint64_t n,
                                  int final, uint8_t* digest32, void* stream) {
    if (int r = resume_args(state8, absorbed, data_dev, n, final, digest32)) return r;
    KRK_DEVICE(D);
    if (!stream)  // the caller has waited for the bytes: an event on an idle stream would still
                  // queue behind other streams' packets in its shared hardware queue (ms each)
        return resume_on_host(D, state8, absorbed, data_dev, n, final != 0, digest32, nullptr);
    hipEvent_t ready;
    KRK_HIP(hipEventCreateWithFlags(&ready, hipEventDisableTiming));
    int r = KRK_OK;
    if (hipEventRecord(ready, static_cast<hipStream_t>(stream)) != hipSuccess) {
        set_error(KRK_EHIP, "sha256_resume: event record failed");
        r = KRK_EHIP;
    }
    if (!r) r = resume_on_host(D, state8, absorbed, data_dev, n, final != 0, digest32, ready);
    hipEventDestroy(ready);
    return r;
}

int krk_sha256_resume_host(uint32_t* state8, uint64_t absorbed, const uint8_t* data_host, uint64_t n, int final,
                           uint8_t* digest32) {
    if (int r = resume_args(state8, absorbed, data_host, n, final, digest32)) return r;
    const auto t = Clock::now();
    if (!final)
        host_sha256_blocks(state8, data_host, n / 64);
    else
        host_sha256_final(state8, absorbed, data_host, n, digest32);
    t_resume.hash += since(t);
    return KRK_OK;
}

int krk_sha256_resume_stats(double* copy_wait_s, double* hash_s) {
    if (copy_wait_s) *copy_wait_s = t_resume.wait;
    if (hash_s) *hash_s = t_resume.hash;
    return KRK_OK;
}
int krk_sha256_resume_stats2(double* issue_s, double* ready_s) {
    if (issue_s) *issue_s = t_resume.issue;
    if (ready_s) *ready_s = t_resume.ready;
    return KRK_OK;
}

}  // extern "C"
