// engine.cpp -- the per-device submission engine behind the streaming entry points
// (digester.cpp: krk_digester_*; piece_stream.cpp: krk_piece_stream_*, krk_crc32_update).
//
// The reference calls these from many goroutines at once (SURVEY.md 8(b)
// "Threading": origin/blobserver/uploader.go:75 and lib/store/ca_store.go:119 run a
// Digester per upload / cache fill, lib/torrent/storage/agentstorage/torrent.go:182
// a PieceHash per received piece).  One launch per call would serialise them and
// leave the chip empty, so every device context owns a pool of pinned staging slots
// (engine.hpp) and two queues (SHA-256, CRC-32), each with a dispatcher thread that
// coalesces the pending requests into ONE launch and a completer thread that retires
// launches in order, so up to kInflight launches per queue are on the device at once and
// the host's job building, result copies and wake-ups overlap the kernels.
//
// SHA-256 (Digester): every GPU digester owns a row of the engine's HBM state table
// (8 words) and digest table (32 B).  A request's job starts from that row
// (kShaFromState, or the IV for the first request) and writes it back, so a
// digester's requests chain through the device in stream order: the dispatcher takes
// at most one request per digester per launch and may launch the next batch behind the
// running one without waiting for its results.  It forms that next batch once every
// digester of the running batch has its next request queued, or shortly before the
// running batch is due to end (estimated from the measured per-byte time of earlier
// batches), so a digester whose next request arrives a little late still makes the
// next launch.  Only final requests copy anything back (their digests).
//
// CRC-32 (PieceHash / piece streams): requests carry no state: each piece portion is
// hashed as an independent message, so any number of an owner's requests may share a
// launch; the owner folds the portions' CRCs (piece_stream.cpp).
#include <thread>
#include <unordered_set>

#include "engine.hpp"
#include "engine_math.hpp"

namespace krk {
namespace {

constexpr int kMaxInflight = 8;           // result buffers per queue (launches on the device at once <= this)
constexpr int kInflight = 3;              // launches per queue on the device at once
static_assert(kInflight <= kMaxInflight, "every launch on the device writes a result buffer of its own");
constexpr uint32_t kStateRows = 65536;    // GPU digesters per device (state + digest rows)
constexpr uint64_t kMaxCrcBatchBytes = 4ull << 30;
// SHA coalescing on an idle device: the longest the first request waits for company, or
// kQuiet with no new owner.  10 ms: 256 writers starting together reach their first full
// slot over 5-25 ms on a CPU-quota box; with 3 ms a third of the rounds launched before all
// were in and ran 3-4 launches more (profiles/r03/engine_quiet_ab.jsonl: median 13.94 ->
// 14.16 GB/s, every round 33 launches).  A GPU Digester carries >= 512 KiB a request, ~9 ms
// of a stream.
constexpr auto kCoalesce = std::chrono::milliseconds(30);
constexpr auto kQuiet = std::chrono::milliseconds(10);

struct Inflight {
    std::vector<Req*> batch;
    hipEvent_t done = nullptr;
    int rc = KRK_OK;
    std::string err;
    int out_i = -1;  // the queue's pinned result buffer this launch writes
    uint64_t max_len = 0;
    Clock::time_point t_launch;
    char reason = '-';                    // trace: why the batch was formed
    size_t depth = 0, left_queued = 0;    // trace: launches on the device, requests left
    int64_t missing = 0;
    double est = 0;                       // trace: the per-byte time estimate when formed
    // SHA: digest rows [row0, row0 + nrows) copied back (final requests)
    uint32_t row0 = 0, nrows = 0;
    // CRC: request i's portion CRCs at base[i] .. base[i + 1] of the results
    std::vector<uint64_t> base;
    uint64_t total = 0;
};

struct Queue {
    const Kind kind;  // kSha: one request per owner per launch, coalesced; kCrc: FIFO
    explicit Queue(Kind k) : kind(k) {}
    bool sha() const { return kind == Kind::kSha; }
    std::mutex mu;
    std::condition_variable cv;       // dispatcher: requests, a retired launch, stop
    std::condition_variable cv_done;  // completer: a launch to retire
    std::deque<Req*> q;
    std::deque<Inflight*> inflight;   // launch order
    bool stop = false, disp_exited = false;
    bool dispatching = false;  // a batch is between take_batch and publish (one at a time: stream order = owner order)
    std::thread th, th_done;
    hipStream_t s = nullptr;
    uint8_t* out[kMaxInflight] = {};  // pinned result buffers, grown on demand
    size_t out_cap[kMaxInflight] = {};
    bool out_busy[kMaxInflight] = {};
    std::vector<uint8_t*> retired;    // grown-out result buffers
    // SHA coalescing: per owner, requests queued and non-final requests in launches on
    // the device; `missing` counts owners with requests on the device but none queued
    // (and no final request formed: a digester that asked for its digest is not
    // expected back).  A new batch is formed early only when missing == 0.
    struct Own {
        int queued = 0, flying = 0;
        bool closed = false;
    };
    std::unordered_map<const void*, Own> own;
    int64_t missing = 0;
    Clock::time_point due;                        // expected end of the last launch
    Clock::time_point last_arrival;               // an owner with nothing on the device queued a request
    Clock::time_point last_done;                  // when the previous launch retired
    double ns_per_byte = 1e9 / 59e6;              // per-stream SHA time, EMA of measured launches
};

}  // namespace

struct Engine {
    Device* D = nullptr;
    int dev = 0;
    SlotPool pool;
    hipStream_t s_copy = nullptr;
    std::mutex copy_mu;
    uint64_t copy_seq = 0;
    Queue sha{Kind::kSha}, crc{Kind::kCrc};
    uint32_t* d_state = nullptr;  // kStateRows x 8 words
    uint8_t* d_digest = nullptr;  // kStateRows x 32 B
    std::mutex row_mu;
    std::vector<uint32_t> free_rows;
    std::mutex pend_mu;
    std::vector<std::unique_ptr<uint8_t[]>> pend_free;
    uint32_t next_row = 0;
    uint64_t fail_crc_at = 0;     // fault injection for tests: the n-th CRC launch fails (0 = never)
    bool trace = false;           // KRK_ENGINE_TRACE: one stderr line per SHA launch
    Clock::time_point t0 = Clock::now();
    uint64_t crc_launches = 0;
    std::atomic<uint64_t> sha_batches{0}, sha_jobs{0}, crc_batches{0}, crc_reqs{0};
    std::atomic<int64_t> live_digesters{0};  // GPU digesters placed on this engine
};

namespace {

void finish(Req* r, int rc, const std::string& err) {
    r->rc = rc;
    if (rc != KRK_OK) r->err = err;
    if (r->on_done) r->on_done(r);
    std::lock_guard<std::mutex> g(r->w->mu);
    r->done = true;
    r->w->cv.notify_all();
}

int grow_out(Queue& Q, int i, size_t n) {
    if (Q.out_cap[i] >= n) return KRK_OK;
    // freeing pinned memory waits for the whole device: the old buffer is kept until teardown
    if (Q.out[i]) Q.retired.push_back(Q.out[i]);
    Q.out[i] = nullptr;
    Q.out_cap[i] = 0;
    size_t cap = 1 << 20;
    while (cap < n) cap <<= 1;
    KRK_HIP(hipHostMalloc(reinterpret_cast<void**>(&Q.out[i]), cap, hipHostMallocDefault));
    Q.out_cap[i] = cap;
    return KRK_OK;
}

// One multi-stream SHA-256 launch: job i runs from its owner's state row (or the IV)
// and writes the row back (non-final) or the owner's digest row (final).
int launch_sha(Engine* E, Inflight* f) {
    Device* D = E->D;
    Queue& Q = E->sha;
    const size_t n = f->batch.size();
    std::vector<ShaJob> jobs(n);
    uint32_t lo = UINT32_MAX, hi = 0;
    for (size_t i = 0; i < n; ++i) {
        Req* r = f->batch[i];
        // zero-copy: the producer waves load the pinned slot over PCIe (Kind, engine.hpp)
        jobs[i] = sha_job(r->slot ? r->slot->mapped : reinterpret_cast<const uint8_t*>(E->d_state), r->prefix, r->len,
                          r->final, r->row);
        f->max_len = std::max<uint64_t>(f->max_len, r->len);
        if (r->final) lo = std::min(lo, r->row), hi = std::max(hi, r->row);
    }
    int rc = run_jobs(D, jobs, E->d_digest, E->d_state, Q.s);
    if (!rc && lo <= hi) {
        f->row0 = lo;
        f->nrows = hi - lo + 1;
        rc = grow_out(Q, f->out_i, 32ull * f->nrows);
        if (!rc && hipMemcpyAsync(Q.out[f->out_i], E->d_digest + 32ull * lo, 32ull * f->nrows, hipMemcpyDeviceToHost,
                                  Q.s) != hipSuccess) {
            set_error(KRK_EHIP, "engine: SHA digest copy");
            rc = KRK_EHIP;
        }
    }
    return rc;
}

void complete_sha(Engine* E, Inflight* f) {
    if (f->rc) return;
    for (Req* r : f->batch)
        if (r->final) memcpy(r->digest, E->sha.out[f->out_i] + 32ull * (r->row - f->row0), 32);
    E->sha_batches.fetch_add(1, std::memory_order_relaxed);
    E->sha_jobs.fetch_add(f->batch.size(), std::memory_order_relaxed);
}

// Portions of stream bytes [a, a+len) cut at multiples of P: engine_math.hpp.
using em::Portions;
using em::portions;

int launch_crc(Engine* E, Inflight* f) {
    Device* D = E->D;
    Queue& Q = E->crc;
    ItemBuilder B;
    CrcBatch cb;
    auto& batch = f->batch;
    f->base.assign(batch.size() + 1, 0);
    uint64_t total = 0;
    const Req* last = nullptr;  // the last-staged request of the batch
    for (size_t i = 0; i < batch.size(); ++i) {
        Req* r = batch[i];
        f->base[i] = total;
        const Portions p = portions(r->off, r->len, r->P);
        total += p.count;
        f->max_len = std::max<uint64_t>(f->max_len, r->len);
        if (!p.count) continue;
        if (!last || r->seq > last->seq) last = r;
        const uint64_t dev = reinterpret_cast<uint64_t>(r->slot->dev);
        const uint64_t a = r->off, b = r->off + r->len;
        uint64_t idx = f->base[i];
        auto part = [&](uint64_t s, uint64_t e) {  // a portion hashed as its own message
            B.piece(cb.items, dev + (s - a), s, e, s, e, (uint32_t)idx++, 0xFFFFFFFFu);
        };
        if (p.head) part(a, p.first_end);
        if (p.f1 > p.f0) {
            B.run(cb, dev + (p.f0 * r->P - a), p.f0, p.f1, r->P, idx - p.f0);
            idx += p.f1 - p.f0;
        }
        if (p.tail) part(std::max(a, p.f1 * r->P), b);
    }
    f->base[batch.size()] = total;
    f->total = total;
    if (total >= (1ull << 32)) {
        set_error(KRK_EINVAL, "engine: more than 2^32 CRC portions in one batch");
        return KRK_EINVAL;
    }
    if (!total) return KRK_OK;
    // The copy stream's H2D of every request of the batch is done once the last-staged one
    // is (one stream, copies in seq order): one wait instead of one per request.
    KRK_HIP(hipStreamWaitEvent(Q.s, last->slot->h2d, 0));
    int rc = KRK_OK;
    uint32_t* d_sums = nullptr;
    KRK_HIP(scratch_alloc(D, &d_sums, total * 4, Q.s));
    if (hipMemsetAsync(d_sums, 0, total * 4, Q.s) != hipSuccess) {
        set_error(KRK_EHIP, "engine: CRC sums clear");
        rc = KRK_EHIP;
    }
    if (!rc) rc = run_items(D, cb, d_sums, Q.s);
    if (!rc) rc = grow_out(Q, f->out_i, total * 4);
    if (!rc && hipMemcpyAsync(Q.out[f->out_i], d_sums, total * 4, hipMemcpyDeviceToHost, Q.s) != hipSuccess) {
        set_error(KRK_EHIP, "engine: CRC result copy");
        rc = KRK_EHIP;
    }
    scratch_free(D, d_sums, Q.s);
    return rc;
}

void complete_crc(Engine* E, Inflight* f) {
    if (f->rc) return;
    const uint32_t* res = reinterpret_cast<const uint32_t*>(E->crc.out[f->out_i]);
    for (size_t i = 0; i < f->batch.size(); ++i) f->batch[i]->crcs.assign(res + f->base[i], res + f->base[i + 1]);
    E->crc_batches.fetch_add(1, std::memory_order_relaxed);
    E->crc_reqs.fetch_add(f->batch.size(), std::memory_order_relaxed);
}

// Owner bookkeeping for the SHA coalescing (with Q.mu held): apply `f` to o's counts
// and keep Q.missing = #owners with requests on the device, none queued, not closed.
template <class F>
void own_update(Queue& Q, const void* o, F&& f) {
    Queue::Own& w = Q.own[o];
    const bool before = w.flying > 0 && w.queued == 0 && !w.closed;
    f(w);
    const bool after = w.flying > 0 && w.queued == 0 && !w.closed;
    Q.missing += (after ? 1 : 0) - (before ? 1 : 0);
    if (w.queued == 0 && w.flying == 0) Q.own.erase(o);
}

// Every owner with requests on the device has its next request queued; on an idle
// device, every live GPU digester of the engine has one queued.
bool expected_present(const Queue& Q, int64_t live) {
    if (Q.q.empty()) return false;
    if (Q.inflight.empty()) return live > 0 && (int64_t)Q.own.size() >= live;
    return Q.missing == 0;
}

// With Q->mu held and no dispatch in progress: the next batch (SHA: the oldest request of
// each owner, FIFO -- its state row chains through the launches, which run one after the
// other on the queue's stream; CRC: up to kMaxCrcBatchBytes), marked as being dispatched.
Inflight* take_batch(Queue* Q, char reason) {
    auto* f = new Inflight();
    if (Q->sha()) {
        std::unordered_set<const void*> seen;
        for (auto it = Q->q.begin(); it != Q->q.end() && f->batch.size() < kStateRows;) {
            if (seen.insert((*it)->owner).second) {
                Req* r = *it;
                f->batch.push_back(r);
                own_update(*Q, r->owner, [&](Queue::Own& w) {
                    --w.queued;
                    if (r->final) w.closed = true;
                });
                it = Q->q.erase(it);
            } else {
                ++it;
            }
        }
    } else {
        uint64_t bytes = 0;
        while (!Q->q.empty() && (f->batch.empty() || bytes + Q->q.front()->len <= kMaxCrcBatchBytes)) {
            bytes += Q->q.front()->len;
            f->batch.push_back(Q->q.front());
            Q->q.pop_front();
        }
    }
    f->reason = reason;
    f->depth = Q->inflight.size();
    f->left_queued = Q->q.size();
    f->missing = Q->missing;
    f->est = Q->ns_per_byte;
    for (int i = 0; i < kMaxInflight; ++i)
        if (!Q->out_busy[i]) {
            Q->out_busy[i] = true;
            f->out_i = i;
            break;
        }
    Q->dispatching = true;
    return f;
}

// Without the lock: launch f on the queue's stream and record its completion event.
void launch_batch(Engine* E, Queue* Q, Inflight* f) {
    // A caller's thread may run this (submit): the launch goes to the engine's device, and
    // the caller's current device -- HIP's and the library's (t_dev, which the launch timing
    // records) -- is restored afterwards.
    int hip_saved = -1;
    if (hipGetDevice(&hip_saved) != hipSuccess) hip_saved = -1;
    const int t_saved = t_dev;
    struct Restore {
        int hip, t;
        ~Restore() {
            t_dev = t;
            if (hip >= 0) hipSetDevice(hip);
        }
    } restore{hip_saved, t_saved};
    hipSetDevice(E->dev);
    t_dev = E->dev;
    f->t_launch = Clock::now();
    if (Q->sha() && E->trace)
        fprintf(stderr, "krk_engine sha t=%.3fms abs=%.3fms n=%zu why=%c depth=%zu left_queued=%zu missing=%lld est=%.2fns/B\n",
                std::chrono::duration<double, std::milli>(f->t_launch - E->t0).count(),
                std::chrono::duration<double, std::milli>(f->t_launch.time_since_epoch()).count(), f->batch.size(),
                f->reason, f->depth, f->left_queued, (long long)f->missing, f->est);
    if (!Q->sha() && ++E->crc_launches == E->fail_crc_at) {
        set_error(KRK_EHIP, "engine: injected failure of CRC launch %llu (fault injection, diag build)",
                  (unsigned long long)E->crc_launches);
        f->rc = KRK_EHIP;
    } else {
        f->rc = Q->sha() ? launch_sha(E, f) : launch_crc(E, f);
    }
    if (!f->rc) {
        if (hipEventCreateWithFlags(&f->done, hipEventDisableTiming) != hipSuccess ||
            hipEventRecord(f->done, Q->s) != hipSuccess) {
            set_error(KRK_EHIP, "engine: launch event");
            f->rc = KRK_EHIP;
        }
    }
    if (f->rc) f->err = t_err;
}

// With Q->mu held: f joins the launches on the device; the next dispatch may start.
void publish(Queue* Q, Inflight* f) {
    if (Q->sha()) {
        for (const Req* r : f->batch)
            if (!r->final) own_update(*Q, r->owner, [](Queue::Own& w) { ++w.flying; });
        const auto start = std::max(f->t_launch, Q->inflight.empty() ? f->t_launch : Q->due);
        Q->due = start + std::chrono::nanoseconds((int64_t)(Q->ns_per_byte * (double)f->max_len));
    }
    Q->inflight.push_back(f);
    Q->dispatching = false;
}

void dispatcher(Engine* E, Queue* Q) {
    hipSetDevice(E->dev);
    t_dev = E->dev;
    for (;;) {
        Inflight* f = nullptr;
        {
            std::unique_lock<std::mutex> lk(Q->mu);
            Q->cv.wait(lk, [&] {
                return (Q->stop && Q->q.empty() && !Q->dispatching) ||
                       (!Q->q.empty() && !Q->dispatching && Q->inflight.size() < (size_t)kInflight);
            });
            if (Q->q.empty()) {  // stop requested and drained
                Q->disp_exited = true;
                Q->cv_done.notify_all();
                return;
            }
            char reason = '-';
            if (Q->sha()) {
                // Coalesce: on an idle device the first request waits kCoalesce for
                // company; behind running launches, the next batch is formed once every
                // owner with requests on the device has its next request queued, or ~1 ms
                // before the last launch is due to end.  (Forming it as soon as SOME owners
                // are back splits the owners into groups that alternate between launches:
                // each would then run at a fraction of the per-stream rate.)  The submission
                // that completes the set usually launches the batch itself (submit()).
                reason = 'T';
                for (;;) {
                    if (Q->stop || expected_present(*Q, E->live_digesters.load(std::memory_order_relaxed))) {  // every owner on the device is back
                        reason = Q->stop ? 'S' : 'P';
                        break;
                    }
                    // idle device: wait until every live GPU digester has a request queued, or
                    // kQuiet passes with no new owner, at most kCoalesce after the first request,
                    // so that uploads that start together also start on the device together
                    // (a digester that misses the first launch runs a whole launch behind)
                    const auto until = Q->inflight.empty()
                                           ? std::min(Q->q.front()->t_submit + kCoalesce, Q->last_arrival + kQuiet)
                                           : Q->due - std::chrono::milliseconds(1);
                    if (Clock::now() >= until) break;
                    Q->cv.wait_until(lk, until);
                    if (Q->q.empty() || Q->dispatching) break;
                }
                // a caller dispatched meanwhile, or took every request
                if (Q->q.empty() || Q->dispatching || Q->inflight.size() >= (size_t)kInflight) continue;
            }
            f = take_batch(Q, reason);
        }
        launch_batch(E, Q, f);
        {
            std::lock_guard<std::mutex> g(Q->mu);
            publish(Q, f);
        }
        Q->cv.notify_all();
        Q->cv_done.notify_one();
    }
}

// Retires launches in order: waits for the device, hands results to the requests,
// releases their slots and wakes their owners.
void completer(Engine* E, Queue* Q) {
    hipSetDevice(E->dev);
    t_dev = E->dev;
    const bool sha = Q->sha();
    for (;;) {
        Inflight* f = nullptr;
        {
            std::unique_lock<std::mutex> lk(Q->mu);
            Q->cv_done.wait(lk, [&] { return !Q->inflight.empty() || Q->disp_exited; });
            if (Q->inflight.empty()) return;
            f = Q->inflight.front();
        }
        if (!f->rc && f->done && hipEventSynchronize(f->done) != hipSuccess) {
            set_error(KRK_EHIP, "engine: %s batch failed", sha ? "SHA" : "CRC");
            f->rc = KRK_EHIP;
            f->err = t_err;
        }
        const auto t_done = Clock::now();
        if (sha && E->trace)
            fprintf(stderr, "krk_engine sha_done abs=%.3fms n=%zu\n",
                    std::chrono::duration<double, std::milli>(t_done.time_since_epoch()).count(), f->batch.size());
        if (sha) complete_sha(E, f);
        else complete_crc(E, f);
        {
            // bookkeeping first: once finished, a request (and its owner) may be freed
            std::lock_guard<std::mutex> g(Q->mu);
            Q->inflight.pop_front();
            if (f->out_i >= 0) Q->out_busy[f->out_i] = false;
            if (sha) {
                for (const Req* r : f->batch)
                    if (!r->final) own_update(*Q, r->owner, [](Queue::Own& w) { --w.flying; });
                if (!f->rc && f->max_len >= (256u << 10)) {  // per-stream time of this launch
                    const auto start = std::max(f->t_launch, Q->last_done);
                    const double ns =
                        (double)std::chrono::duration_cast<std::chrono::nanoseconds>(t_done - start).count();
                    Q->ns_per_byte = 0.7 * Q->ns_per_byte + 0.3 * (ns / (double)f->max_len);
                }
            }
            Q->last_done = t_done;
        }
        for (Req* r : f->batch) {
            E->pool.release(r->slot);
            finish(r, f->rc, f->err);
        }
        if (f->done) hipEventDestroy(f->done);
        Q->cv.notify_all();
        delete f;
    }
}

int engine_start(Engine* E) {
    E->pool.init(kSlotBytes, env_size(KRK_OP_ENV("KRK_SLOT_POOL_MB"), 4096) << 20);
    E->fail_crc_at = env_size(KRK_AB_ENV("KRK_ENGINE_FAIL_CRC_LAUNCH"), 0);
    E->trace = env_size(KRK_OP_ENV("KRK_ENGINE_TRACE"), 0) != 0;
    KRK_HIP(hipMalloc(&E->d_state, 32ull * kStateRows));
    KRK_HIP(hipMalloc(&E->d_digest, 32ull * kStateRows));
    KRK_HIP(hipStreamCreateWithFlags(&E->s_copy, hipStreamNonBlocking));
    for (Queue* Q : {&E->sha, &E->crc}) {
        KRK_HIP(hipStreamCreateWithFlags(&Q->s, hipStreamNonBlocking));
        Q->last_done = Clock::now();
    }
    for (Queue* Q : {&E->sha, &E->crc}) {  // threads start last: none runs when an allocation failed
        Q->th = std::thread(dispatcher, E, Q);
        Q->th_done = std::thread(completer, E, Q);
    }
    return KRK_OK;
}

void engine_free_resources(Engine* E) {
    hipSetDevice(E->dev);
    for (hipStream_t s : {E->s_copy, E->sha.s, E->crc.s})
        if (s) hipStreamSynchronize(s), hipStreamDestroy(s);
    for (Queue* Q : {&E->sha, &E->crc}) {
        for (auto& p : Q->out)
            if (p) hipHostFree(p), p = nullptr;
        for (uint8_t* p : Q->retired) hipHostFree(p);
        Q->retired.clear();
    }
    if (E->d_state) hipFree(E->d_state);
    if (E->d_digest) hipFree(E->d_digest);
    E->pool.destroy();
}

void engine_stop(Engine* E) {
    for (Queue* Q : {&E->sha, &E->crc}) {
        {
            std::lock_guard<std::mutex> g(Q->mu);
            Q->stop = true;
        }
        Q->cv.notify_all();
        Q->cv_done.notify_all();
        if (Q->th.joinable()) Q->th.join();
        if (Q->th_done.joinable()) Q->th_done.join();
    }
    engine_free_resources(E);
}

// r's slot holds r->len bytes: issue its H2D to the device mirror on the copy stream.
int stage(Engine* E, Req* r) {
    if (!r->len) return KRK_OK;
    KRK_HIP(hipSetDevice(E->dev));
    std::lock_guard<std::mutex> g(E->copy_mu);
    KRK_HIP(hipMemcpyAsync(r->slot->dev, r->slot->host, r->len, hipMemcpyHostToDevice, E->s_copy));
    KRK_HIP(hipEventRecord(r->slot->h2d, E->s_copy));
    r->seq = ++E->copy_seq;
    return KRK_OK;
}

}  // namespace

Engine* engine_of(int id, int* rc) {
    Device* D = device_id(id, rc);
    if (!D) return nullptr;
    std::lock_guard<std::mutex> g(D->engine_mu);
    if (!D->engine) {
        auto* E = new Engine();
        E->D = D;
        E->dev = id;
        *rc = engine_start(E);
        if (*rc) {
            engine_free_resources(E);
            delete E;
            return nullptr;
        }
        D->engine = E;
    }
    return D->engine;
}

SlotPool& engine_pool(Engine* E) { return E->pool; }
std::atomic<int64_t>& engine_live_digesters(Engine* E) { return E->live_digesters; }

void trace_slow(Engine* E, const char* what, Clock::time_point t0) {
    const double ms = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
    if (E->trace && ms > 5.0)
        fprintf(stderr, "krk_engine slow %s %.2fms abs=%.3fms\n", what, ms,
                std::chrono::duration<double, std::milli>(t0.time_since_epoch()).count());
}

// Queue r.  On the SHA queue, the submission that completes the coalescing set (every
// owner with requests on the device has its next one queued; on an idle device, every
// live GPU digester has one) launches the batch on its own thread: with many writer
// threads busy filling slots, the dispatcher thread could wait tens of milliseconds for a
// CPU while the device idled (tools/engine_slow.py: slow rounds' first launch formed ~90
// ms after their requests were all queued).  The dispatcher still forms the batches that
// coalescing times out on.
void submit(Engine* E, Kind k, Req* r) {
    Queue& Q = k == Kind::kSha ? E->sha : E->crc;
    r->t_submit = Clock::now();
    Inflight* f = nullptr;
    {
        std::lock_guard<std::mutex> g(Q.mu);
        Q.q.push_back(r);
        if (Q.sha()) {
            own_update(Q, r->owner, [&](Queue::Own& w) {
                if (w.queued == 0 && w.flying == 0) Q.last_arrival = r->t_submit;
                ++w.queued;
                w.closed = false;
            });
            if (!Q.dispatching && !Q.stop && Q.inflight.size() < (size_t)kInflight &&
                expected_present(Q, E->live_digesters.load(std::memory_order_relaxed)))
                f = take_batch(&Q, 'C');
        }
    }
    if (f) {
        const std::string keep = t_err;  // the launch's error text belongs to its requests
        launch_batch(E, &Q, f);
        t_err = keep;
        {
            std::lock_guard<std::mutex> g(Q.mu);
            publish(&Q, f);
        }
        Q.cv_done.notify_one();
    }
    Q.cv.notify_all();
}

int make_req(Engine* E, Kind k, Slot* sl, const uint8_t* src, uint64_t len, Req** out) {
    *out = nullptr;
    if (!sl && len) {
        int rc = KRK_OK;
        sl = E->pool.acquire(&rc);
        if (!sl) return rc;
        memcpy(sl->host, src, len);
    }
    auto* r = new Req();
    r->slot = sl;
    r->len = len;
    const int rc = k == Kind::kCrc ? stage(E, r) : KRK_OK;
    if (rc) {
        E->pool.release(sl);
        delete r;
        return rc;
    }
    *out = r;
    return KRK_OK;
}

int wait_req(Req* r) {
    std::unique_lock<std::mutex> lk(r->w->mu);
    r->w->cv.wait(lk, [&] { return r->done; });
    if (r->rc) t_err = r->err;
    return r->rc;
}

uint32_t row_acquire(Engine* E, int* rc) {
    std::lock_guard<std::mutex> g(E->row_mu);
    if (!E->free_rows.empty()) {
        const uint32_t r = E->free_rows.back();
        E->free_rows.pop_back();
        *rc = KRK_OK;
        return r;
    }
    if (E->next_row < kStateRows) {
        *rc = KRK_OK;
        return E->next_row++;
    }
    set_error(KRK_ENOMEM, "engine: more than %u GPU digesters on one device", kStateRows);
    *rc = KRK_ENOMEM;
    return 0;
}

void row_release(Engine* E, uint32_t row) {
    std::lock_guard<std::mutex> g(E->row_mu);
    E->free_rows.push_back(row);
}

std::unique_ptr<uint8_t[]> pend_acquire(Engine* E) {
    {
        std::lock_guard<std::mutex> g(E->pend_mu);
        if (!E->pend_free.empty()) {
            auto b = std::move(E->pend_free.back());
            E->pend_free.pop_back();
            return b;
        }
    }
    return std::unique_ptr<uint8_t[]>(new uint8_t[E->pool.S]);
}

void pend_release(Engine* E, std::unique_ptr<uint8_t[]> b) {
    if (!b) return;
    std::lock_guard<std::mutex> g(E->pend_mu);
    if (E->pend_free.size() < 4096) E->pend_free.push_back(std::move(b));
}

size_t owner_inflight(Engine* E) {
    const size_t slots = E->pool.cap() / E->pool.S, reserve = E->pool.reserve();
    const int64_t live = std::max<int64_t>(1, E->live_digesters.load(std::memory_order_relaxed));
    const size_t share = slots > reserve ? (slots - reserve) / (size_t)live : 0;
    return std::max<size_t>(2, std::min(kOwnerInflight, share));
}

// krk_shutdown: stop the engine of D (its dispatcher and completer threads drain their queues).
void engine_teardown(Device& D) {
    std::lock_guard<std::mutex> g(D.engine_mu);
    if (D.engine) {
        engine_stop(D.engine);
        delete D.engine;
        D.engine = nullptr;
    }
}

}  // namespace krk

using namespace krk;

extern "C" {

int krk_engine_stats(uint64_t* sha_batches, uint64_t* sha_jobs, uint64_t* crc_batches, uint64_t* crc_requests,
                     uint64_t* pinned_bytes) {
    KRK_DEVICE(D);
    uint64_t v[5] = {0, 0, 0, 0, 0};
    {
        std::lock_guard<std::mutex> g(D->engine_mu);
        if (Engine* E = D->engine) {
            v[0] = E->sha_batches.load();
            v[1] = E->sha_jobs.load();
            v[2] = E->crc_batches.load();
            v[3] = E->crc_reqs.load();
            v[4] = E->pool.pinned_bytes();
        }
    }
    uint64_t* o[5] = {sha_batches, sha_jobs, crc_batches, crc_requests, pinned_bytes};
    for (int i = 0; i < 5; ++i)
        if (o[i]) *o[i] = v[i];
    return KRK_OK;
}

int krk_engine_set_pool_cap(uint64_t bytes, uint64_t* cap_out, uint64_t* waits_out) {
    KRK_DEVICE(D0);
    int rc = KRK_OK;
    Engine* E = engine_of(D0->id, &rc);
    if (!E) return rc;
    if (bytes) E->pool.set_cap(bytes);
    if (cap_out) *cap_out = E->pool.cap();
    if (waits_out) *waits_out = E->pool.waits();
    return KRK_OK;
}

}  // extern "C"
