// window_pass.cpp -- the host-resident window pass (window_pass.hpp): every
// window of a schedule is laid into a staging slot, filled from the source or sent up straight
// from the caller's pages, and run through the SHA-256 and CRC kernels; with the two sources
// (caller memory, cache files) and the file batches' descriptor budget.
//
// The schedule says which bytes of which blob a window carries (window_math.hpp): for the
// digest calls every live blob advances by the same chunk per window, SHA-256 chained through
// per-blob midstates in HBM and the chunk's piece CRCs XOR-accumulated into its pieces (CRC-32
// is linear, so any cut is legal); the CRC-only calls pack the blobs end to end.  The host's
// work per window is O(chunks).
#include "window_pass.hpp"

#include <dirent.h>
#include <sys/resource.h>

#include <condition_variable>
#include <deque>
#include <thread>

namespace krk {

// ------------------------------------------------------------------ caller memory
bool MemSource::all_pinned(const std::vector<char>& skip) const {
    for (uint64_t i = 0; i < n; ++i)
        if (!(i < skip.size() && skip[i]) && blobs[i].length && !host_pinned(blobs[i].data, blobs[i].length)) return false;
    return true;
}

void MemSource::setup(const std::vector<char>& skip, bool pinned_, int gather_mode, hipStream_t cp) {
    pinned = pinned_;
    std::vector<std::pair<uintptr_t, uintptr_t>> ranges;
    for (uint64_t i = 0; i < n; ++i)
        if (!(i < skip.size() && skip[i]) && blobs[i].length) {
            const uintptr_t a = reinterpret_cast<uintptr_t>(blobs[i].data);
            ranges.push_back({a, a + blobs[i].length});
        }
    // every windowed blob read at its host address, not the first alone
    mapped = pinned && gather_mode != 0 && !ranges.empty();
    MappedAtHost at_host;
    for (size_t k = 0; mapped && k < ranges.size(); ++k)
        mapped = at_host(reinterpret_cast<const void*>(ranges[k].first), ranges[k].second - ranges[k].first);
    if (!pinned && gather_mode == 1 && !ranges.empty()) {
        reg = std::make_unique<HostRegistry>(std::move(ranges));
        gather_stream = cp;
    }
}

int MemSource::fill(const std::vector<FillTask>& tasks) {
    std::vector<CopyTask> c;
    c.reserve(tasks.size());
    for (const FillTask& t : tasks)
        if (t.len) c.push_back({t.dst, at(t.b, t.off), t.len});
    par_copy(c);
    return KRK_OK;
}

// ------------------------------------------------------------------ cache files
FileSource::FileSource(const krk_file_blob* f, uint64_t n, bool want_direct, bool async)
    : files_(f), direct_(want_direct), async_(async), fd_(n, -1), is_direct_(n, 0),
      ra_(async ? new std::atomic<uint64_t>[n]() : nullptr) {}

FileSource::~FileSource() {
    for (int x : fd_)
        if (x >= 0) close(x);
}

int FileSource::open_file(uint32_t i) {
    if (fd_[i] >= 0) return KRK_OK;
    int x = -1;
    if (direct_) {
        x = open(files_[i].path, O_RDONLY | O_DIRECT | O_CLOEXEC);
        is_direct_[i] = x >= 0;
    }
    if (x < 0) x = open(files_[i].path, O_RDONLY | O_CLOEXEC);
    KRK_CHECK(x >= 0, KRK_EIO, "open %s: %s", files_[i].path, strerror(errno));
    fd_[i] = x;
    return KRK_OK;
}

int FileSource::fill(const std::vector<FillTask>& tasks) {
    std::vector<ReadTask> plain, odirect;
    for (const FillTask& t : tasks) {
        // every file is opened, an empty one too: Generate / verify open the file and fail on
        // a missing one
        int r = open_file(t.b);
        if (r) return r;
        if (!t.len) continue;
        (is_direct_[t.b] ? odirect : plain)
            .push_back({fd_[t.b], t.off, t.dst, (size_t)t.len, (size_t)t.b, ra_ ? &ra_[t.b] : nullptr, files_[t.b].length});
    }
    for (int pass = 0; pass < 2; ++pass) {
        const auto& rt = pass ? odirect : plain;
        if (rt.empty()) continue;
        int e = 0;
        long bad = pass == 1 && async_ && use_aio() ? aio_.read(rt, &e) : -2;
        if (bad == -2) bad = par_read(rt, pass == 1, &e);
        if (bad >= 0) {
            const char* path = files_[rt[bad].blob].path;
            if (e) set_error(KRK_EIO, "read blob: %s: %s", path, strerror(e));
            else set_error(KRK_EIO, "read blob: %s: unexpected EOF", path);
            return KRK_EIO;
        }
    }
    for (const FillTask& t : tasks)  // a blob's last chunk: its file is done
        if (t.off + t.len == files_[t.b].length && fd_[t.b] >= 0) {
            close(fd_[t.b]);
            fd_[t.b] = -1;
        }
    return KRK_OK;
}

// File descriptors the file batches may hold open, shared by the whole process (ADVICE r04:
// every *_multi worker and every concurrent caller took the whole remaining budget for
// itself): the soft RLIMIT_NOFILE less the descriptors open at first use and a reserve for
// the rest of the process, handed out in leases.
namespace {
class FdPool {
  public:
    uint64_t acquire(uint64_t want) {
        std::unique_lock<std::mutex> g(mu_);
        if (!init_) {
            free_ = initial_budget();
            init_ = true;
        }
        cv_.wait(g, [&] { return free_ > 0; });
        const uint64_t take = std::max<uint64_t>(1, std::min(want, free_));
        free_ -= take;
        return take;
    }
    void release(uint64_t n) {
        {
            std::lock_guard<std::mutex> g(mu_);
            free_ += n;
        }
        cv_.notify_all();
    }

  private:
    static uint64_t initial_budget() {
        if (const char* e = KRK_OP_ENV("KRK_FD_BUDGET"))  // tests: a small budget without touching the rlimit
            if (strtoull(e, nullptr, 10) > 0) return strtoull(e, nullptr, 10);
        struct rlimit rl {};
        if (getrlimit(RLIMIT_NOFILE, &rl) != 0 || rl.rlim_cur == RLIM_INFINITY) return uint64_t(1) << 20;
        uint64_t open_now = 0;
        if (DIR* d = opendir("/proc/self/fd")) {
            while (readdir(d)) ++open_now;
            closedir(d);
        }
        const uint64_t reserve = 64 + open_now;
        return rl.rlim_cur > reserve + 16 ? rl.rlim_cur - reserve : 16;
    }
    std::mutex mu_;
    std::condition_variable cv_;
    bool init_ = false;
    uint64_t free_ = 0;
};
FdPool& fd_pool() {
    static FdPool* p = new FdPool();  // leaked: used until exit
    return *p;
}
}  // namespace
FdLease::FdLease(uint64_t want) : n(fd_pool().acquire(want)) {}
FdLease::~FdLease() { fd_pool().release(n); }

// ------------------------------------------------------------------ the pass
template <class Source>
int run_windows(const WindowPass& p, Source& src) {
    Device* D = p.D;
    StagingLease lease;
    int r = lease_staging(D, p.lease, lease);
    if (r) return r;
    Pipeline& pl = *lease.p;
    HostRegistry* reg = nullptr;
    if constexpr (Source::kMemory) reg = src.reg.get();
    // A window as built from the schedule: fill tasks, SHA jobs, CRC items.  Window wi always
    // lands in staging slot wi % pl.n (Pipeline::next), so its addresses are known ahead.
    struct Built {
        std::vector<FillTask> tasks;
        std::vector<ShaJob> jobs;
        CrcBatch items;
        size_t fill = 0;
        double build_s = 0;
    };
    ItemBuilder B;
    std::vector<WinChunk> win;
    int built = 0;
    auto build = [&](Built& bt) {  // false: the schedule has ended
        const double tb = wall_s();
        if (!p.next(win)) return false;
        const Window& w = pl.w[built++ % pl.n];
        bt = Built();
        bt.tasks.reserve(win.size());
        if (p.ks) bt.jobs.reserve(win.size());
        for (const WinChunk& c : win) {
            const uint64_t L = p.lens[c.blob];
            bt.tasks.push_back({c.blob, c.off, c.len, w.host + bt.fill});
            if (c.len && p.kc)
                B.add(bt.items, reinterpret_cast<uint64_t>(w.dev + bt.fill), c.off, c.off + c.len, L,
                      (uint64_t)p.plens[c.blob], p.soff[c.blob]);
            if (p.ks) bt.jobs.push_back(chunk_job(w.dev + bt.fill, c.off, c.len, L, c.blob));
            bt.fill += (c.len + p.place - 1) / p.place * p.place;
        }
        bt.build_s = wall_s() - tb;
        return true;
    };
    // With build_ahead, the next windows are built on a helper thread while this one fills and
    // enqueues the current one: with 14,336 live blobs the build is ~1.7 ms a window, 16 % of
    // a page-cache files pass that was fill-bound.
    std::mutex bmu;
    std::condition_variable bcv;
    std::deque<Built> ready;
    bool built_all = false, stop_build = false;
    std::thread builder;
    if (p.build_ahead)
        builder = std::thread([&] {
            for (bool more = true; more;) {
                {
                    std::unique_lock<std::mutex> lk(bmu);
                    bcv.wait(lk, [&] { return stop_build || ready.size() < p.build_ahead; });
                    if (stop_build) return;
                }
                Built bt;
                more = build(bt);
                std::lock_guard<std::mutex> g(bmu);
                if (more) ready.push_back(std::move(bt));
                else built_all = true;
                bcv.notify_all();
            }
        });
    struct BuilderJoin {  // on every way out of the loop
        std::thread& t;
        std::mutex& mu;
        std::condition_variable& cv;
        bool& stop;
        ~BuilderJoin() {
            {
                std::lock_guard<std::mutex> g(mu);
                stop = true;
            }
            cv.notify_all();
            if (t.joinable()) t.join();
        }
    } builder_join{builder, bmu, bcv, stop_build};
    double t_acq = 0, t_build = 0, t_fill = 0, t_enq = 0, t_wait_build = 0;
    auto take = [&](Built& bt) {  // false: every window built and run
        if (!p.build_ahead) return build(bt);
        const double tw = wall_s();
        std::unique_lock<std::mutex> lk(bmu);
        bcv.wait(lk, [&] { return !ready.empty() || built_all; });
        if (ready.empty()) return false;
        bt = std::move(ready.front());
        ready.pop_front();
        bcv.notify_all();
        t_wait_build += wall_s() - tw;
        return true;
    };
    PassStats none, *st = p.st ? p.st : &none;
    int k = 0, wi = 0;
    const double t0 = wall_s();
    Built bt;
    while (!r && take(bt)) {
        t_build += bt.build_s;
        const double ta = wall_s();
        r = pl.acquire(k);
        if (r) break;
        if (reg && wi >= pl.n) reg->copied(wi - pl.n);  // acquire waited for that window's copy
        const double tb = wall_s();
        t_acq += tb - ta;
        Window& w = pl.w[k];
        if (bt.fill > w.cap) {  // the lease covers every window the schedule can build
            set_error(KRK_EINVAL, "%s: window of %zu bytes exceeds the %zu-byte staging lease", p.what, bt.fill,
                      (size_t)w.cap);
            r = KRK_EINVAL;
            break;
        }
        // The way up.  Page-locked sources go straight from the caller's memory into the device
        // window: a DMA a chunk for a few wide chunks (many small DMAs cost more than the
        // staging copy, staging.hpp kDirectMaxCalls), else one gather launch that reads them
        // over PCIe (pinned blobs mapped at their host addresses, or pageable ones once
        // registered); everything else through the pinned host window.
        bool direct = false, gather = false;
        std::vector<CopyTask> up;
        if constexpr (Source::kMemory) {
            direct = !bt.tasks.empty() && src.pinned && bt.tasks.size() <= kDirectMaxCalls;
            gather = !direct && !bt.tasks.empty() && src.gather_ready(wi);
            if (direct || gather) {
                up.reserve(bt.tasks.size());
                for (const FillTask& t : bt.tasks)
                    if (t.len) up.push_back({w.dev + (t.dst - w.host), src.at(t.b, t.off), t.len});
            }
        }
        if (!direct && !gather) {
            r = src.fill(bt.tasks);
            if (r) break;
        }
        const double td = wall_s();
        t_fill += td - tb;
        ++st->windows;
        st->direct_windows += direct;
        st->gather_windows += gather;
        hipError_t e = hipSuccess;
        if (gather) {
            r = pl.h2d_gather(D, k, up, p.cp);
            if (r) break;
        } else {
            e = direct ? pl.h2d_direct(k, up, p.cp) : pl.h2d(k, bt.fill, p.cp);
        }
        if (e != hipSuccess || (p.ks && hipStreamWaitEvent(p.ks, w.copied, 0) != hipSuccess) ||
            (p.kc && hipStreamWaitEvent(p.kc, w.copied, 0) != hipSuccess)) {
            set_error(KRK_EHIP, "%s: staging copy failed", p.what);
            r = KRK_EHIP;
            break;
        }
        if (p.ks) r = run_jobs(D, bt.jobs, p.d_dig, p.d_state, p.ks);
        if (!r && p.kc) r = run_items(D, bt.items, p.d_sums, p.kc);
        if (r) break;
        // the device window is free again once the kernels have read it
        if (p.ks) pl.release(k, 0, p.ks);
        if (p.kc) pl.release(k, 1, p.kc);
        t_enq += wall_s() - td;
        k = pl.next(k);
        ++wi;
    }
    st->loop_s = wall_s() - t0;
    st->acquire_s = t_acq;
    st->fill_s = t_fill;
    st->enqueue_s = t_enq;
    if (reg) {
        st->registered_bytes = reg->registered_bytes();
        st->register_s = reg->register_seconds();
    }
    if (trace_on())
        fprintf(stderr,
                "krk_trace windows: %s windows=%d lease=%zu loop=%.3fs acquire=%.3fs build=%.3fs (ahead %zu; waited "
                "%.3fs) fill=%.3fs enqueue=%.3fs\n",
                p.what, st->windows, p.lease, st->loop_s, t_acq, t_build, p.build_ahead, t_wait_build, t_fill, t_enq);
    return r;
}
template int run_windows<MemSource>(const WindowPass&, MemSource&);
template int run_windows<FileSource>(const WindowPass&, FileSource&);

}  // namespace krk
