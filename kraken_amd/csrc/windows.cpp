// windows.cpp -- the C ABI's host-resident digest calls: the upload /
// cache-fill verify of origin/blobserver/uploader.go:74-94 and lib/store/ca_store.go:99-135
// (Digester over the bytes) fused with the metainfo of lib/metainfogen/generator.go:41-58
// (piece CRCs of the same bytes), so each byte is read once -- from the caller's buffers
// (krk_metainfo_digest_host) or from the cache files themselves (krk_metainfo_digest_files) --
// and crosses PCIe once, where the reference reads every upload twice.  Also here: the window
// schedule's C ABI, the krk_windows_last_* statistics and the gather's test entry point.  The
// pass itself is window_pass.cpp.
//
// The window schedule (the C3 machinery of kraken_amd/windowed.py, here in C++: WindowSched,
// window_math.hpp): at most `cap` blobs are live, admitted longest first so the longest chain
// starts in window 0: by default 7/8 of the largest stream count the SHA-256 launch plan still
// runs on two lanes a stream (14,336 on 256 CUs), which keeps every window on a multi-lane
// plan and leaves an eighth of the CUs free of SHA workgroups for the window's CRC launch,
// queued beside it on another stream (profiles/r02/c3_live_cap.jsonl).
#include <sys/mman.h>

#include <thread>

#include "offload.hpp"
#include "window_pass.hpp"

namespace krk {

// Live streams per window on device D: 7/8 of the largest stream count whose SHA-256 launch
// still runs two (or eight) lanes a stream, a multiple of the two-pair workgroup's 64.
uint64_t window_stream_cap(Device* D) {
    (void)D;  // the plan reads the current device's CU count
    uint64_t lo = 1, hi = uint64_t(1) << 30;
    if (sha_lanes_for((uint32_t)hi) >= 2) return (hi * 7 / 8) / 64 * 64;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) / 2;
        (sha_lanes_for((uint32_t)mid) >= 2 ? lo : hi) = mid;
    }
    return std::max<uint64_t>(64, (lo * 7 / 8) / 64 * 64);
}

namespace {
thread_local PassStats t_last_call;

// KRK_HOST_GATHER: 0 = host-buffer calls always stage; 1 = gather pageable blobs too
// (registered for the call: host_register.hpp); unset (AUTO) = gather page-locked blobs'
// wide windows, stage pageable ones.  Measured on MI355X, C2 end to end
// (profiles/r05/bench_c2.json): pageable 100 MiB blobs registered and gathered 27.3 GB/s
// (3.8 s a pass with the registrations already made, 8.2 s registering 100 GB of fresh 4 KiB
// pages at ~20 GB/s -- registration does not scale with threads), staged 52.3 GB/s; pinned
// blobs (the files leg's krk_host_alloc sources) gathered 58.0 GB/s at 0.034 CPU-s/GB,
// staged 54.9 at 0.134.  The GPU reads 4 KiB-page registrations far slower than the
// library's huge-page pinned blocks, so AUTO registers nothing.
std::atomic<int> g_host_gather{-2};  // -2: not read yet; krk_set_host_gather
int host_gather_mode() {
    int m = g_host_gather.load(std::memory_order_relaxed);
    if (m != -2) return m;
    const char* e = KRK_OP_ENV("KRK_HOST_GATHER");
    int expect = -2;
    g_host_gather.compare_exchange_strong(expect, e ? (atoi(e) > 0 ? 1 : 0) : -1);
    return g_host_gather.load();
}

// Every host-buffer entry point, once its streams have drained and before any copy-out: the
// registry's helpers stopped and every caller range it registered released.  A HIP copy whose
// destination starts in a registered page and runs past it is refused ("copy-out failed:
// invalid argument"): the registry rounds each blob out to whole pages,
// so with the last windows' segments still registered an output array -- or any heap buffer
// -- sharing a page with a small blob was such a destination.  The count left registered is
// kept for krk_windows_last_copyout (0 by construction).
void release_caller_pages(MemSource& f, PassStats* st) {
    if (!f.reg) return;
    f.reg->finish(f.gather_stream);
    st->live_at_copyout = f.reg->live_segments();
}

// A call's results to the caller's host memory, refused (not attempted) while the call still
// holds a registration touching the destination's pages.
int copy_out(void* dst, const void* src_dev, size_t n, const HostRegistry* reg, const char* what) {
    if (!n) return KRK_OK;
    KRK_CHECK(!reg || !reg->overlaps_live(dst, n), KRK_EINVAL,
              "%s copy-out: destination shares a page the call still holds registered", what);
    const hipError_t e = hipMemcpy(dst, src_dev, n, hipMemcpyDeviceToHost);
    KRK_CHECK(e == hipSuccess, KRK_EHIP, "%s copy-out failed: %s", what, hipGetErrorString(e));
    return KRK_OK;
}

// KRK_LIVE_CAP: overrides the window's live-stream cap (tests, sweeps).
uint64_t live_cap_for(Device* D) {
    const char* e = KRK_OP_ENV("KRK_LIVE_CAP");
    const uint64_t v = e ? strtoull(e, nullptr, 10) : 0;
    return v ? v : window_stream_cap(D);
}

// A file batch read O_DIRECT (cold: bound by the disk) needs no more live files than it takes
// the windows' SHA-256 streams to outrun the host link -- h2d over the eight-lane per-stream
// rate, ~970 on MI355X, rounded up to 64: every live file beyond that only shrinks each
// file's chunk of a window, and so the disk's requests.  Cold 32 GiB leg on one box
// (profiles/r06/bench_files_live.json): 3,734 live 12.4 GB/s, 2,048 14.7, 1,024 15.2, 512
// 15.2, 256 13.5 (the streams bind there), the reference's two reads 14.3.  KRK_LIVE_CAP wins.
uint64_t direct_live_cap(Device* D) {
    if (KRK_OP_ENV("KRK_LIVE_CAP")) return live_cap_for(D);
    const Rates R = planner_rates(D);
    const double per_stream = R.stream[0] > 0 ? R.stream[0] : 58e6;
    const double link = R.h2d > 0 ? R.h2d : 56e9;
    const uint64_t need = (uint64_t)(link / per_stream) + 1;
    return std::min(live_cap_for(D), std::max<uint64_t>(256, (need + 63) / 64 * 64));
}

}  // namespace

}  // namespace krk

using namespace krk;

// What krk_metainfo_digest_host, krk_sha256_host and krk_metainfo_digest_files share: the
// device results, the host offload's share with its thread and results, the caller's arrays.
// An entry point checks its arguments, then plan(), start(), its source, run().
namespace {
struct WindowCall {
    const char* name;  // the entry point, in its error texts
    uint64_t n;
    uint32_t* sums_host;
    uint8_t* digests_host;
    bool crc;  // piece sums too (false: digests only, no sums buffer)
    std::vector<uint64_t> lens, soff;
    std::vector<int64_t> plens;
    uint64_t lo = 0, hi = 0;  // the sums span
    double resident = -1;       // file batches: PassStats' resident and direct_reads
    bool direct_reads = false;
    uint8_t* d_dig = nullptr;  // the device's results
    uint32_t *d_state = nullptr, *d_sums = nullptr;
    DevMem mem;
    int off_t = 0;  // the host share's threads, blobs, results, thread and failure
    std::vector<char> on_host;
    std::vector<uint32_t> host, host_sums;
    std::vector<uint8_t> host_dig;
    std::vector<uint64_t> host_sums_off;
    std::thread host_th;
    int host_rc = KRK_OK;
    std::string host_err;
    const int saved_share = t_host_share;

    template <class Blob>
    WindowCall(const char* name_, const Blob* blobs, uint64_t n_, uint32_t* sums, uint8_t* digests, bool crc_ = true)
        : name(name_), n(n_), sums_host(sums), digests_host(digests), crc(crc_), lens(n_), soff(n_), plens(n_),
          on_host(n_, 0) {
        for (uint64_t i = 0; i < n; ++i) {
            lens[i] = blobs[i].length;
            plens[i] = blobs[i].piece_length;
            soff[i] = blobs[i].sums_offset;
        }
        if (crc) sums_span(blobs, n, &lo, &hi);
    }
    // the host thread writes this call's scratch: joined on every path before that goes
    ~WindowCall() {
        if (host_th.joinable()) host_th.join();
        t_host_share = saved_share;
    }

    // The blobs that `threads` host threads take under `mode`, their scratch, the device outputs.
    int plan(Device* D, int mode, int threads) {
        KRK_CHECK(hi == lo || sums_host, KRK_EINVAL, "sums_host is NULL");
        off_t = threads;
        if (off_t > 0) host = offload_plan(lens.data(), n, off_t, planner_rates(D), nullptr, nullptr, mode);
        for (uint32_t i : host) on_host[i] = 1;
        KRK_HIP(mem.alloc(&d_dig, n * 32));
        KRK_HIP(mem.alloc(&d_state, n * 32));
        if (crc) {
            KRK_HIP(mem.alloc(&d_sums, std::max<uint64_t>(hi, 1) * 4));
            KRK_HIP(hipMemset(d_sums, 0, std::max<uint64_t>(hi, 1) * 4));
        }
        host_dig.resize(32 * host.size());
        host_sums_off.assign(host.size() + 1, 0);
        for (size_t j = 0; crc && j < host.size(); ++j)
            host_sums_off[j + 1] = host_sums_off[j] + krk_num_pieces(lens[host[j]], plens[host[j]]);
        host_sums.resize(host_sums_off.back());
        return KRK_OK;
    }
    // work(lengths, piece lengths, sums destinations of the host blobs) -> int on the host
    // thread, started before the windows; its failure is kept for run().
    template <class F>
    void start(F work) {
        if (host.empty()) return;
        host_th = std::thread([this, work] {
            std::vector<uint64_t> l(host.size()), pl(host.size());
            std::vector<uint32_t*> so(host.size());
            for (size_t j = 0; j < host.size(); ++j) {
                l[j] = lens[host[j]];
                pl[j] = (uint64_t)plens[host[j]];
                so[j] = host_sums.data() + host_sums_off[j];
            }
            host_rc = work(l, pl, so);
            if (host_rc) host_err = t_err;
        });
        // The copy threads and the offload's threads share the process's CPU budget: above it
        // a CPU quota throttles the whole process.
        t_host_share = std::max(4, host_threads_for_call() - off_t);
    }
    // The windows of the blobs the host did not take (WindowSched: `cap` live, chunks a multiple
    // of `align`), copied on s_main with SHA-256 on s_a and CRC on s_b, then both sides' results
    // into the caller's arrays.
    template <class Source>
    int run(Device* D, Source& src, uint64_t align, uint64_t cap) {
        PassStats st;
        st.resident = resident;
        st.direct_reads = direct_reads;
        std::vector<uint32_t> blobs;
        for (uint64_t i = 0; i < n; ++i)
            if (!on_host[i]) blobs.push_back((uint32_t)i);
        int r = KRK_OK;
        HostRegistry* reg = nullptr;
        if (!blobs.empty()) {
            const size_t W = window_bytes();
            const uint64_t live_cap = std::min<uint64_t>(cap, blobs.size());
            WindowSched sched(lens.data(), blobs, W, live_cap, align);
            const size_t place = std::max<uint64_t>(align == 64 ? 16 : align, 16);  // chunk start alignment in the window
            // a window holds about W bytes, but never less than one minimum chunk (the schedule's
            // alignment) a live blob, each rounded up to `place` (a small KRK_WINDOW_MB
            // or a large KRK_LIVE_CAP made live x 64 > W + 16 x live)
            const uint64_t span = std::max<uint64_t>(W, live_cap * std::max<uint64_t>(align, 64)) + place * live_cap;
            if constexpr (Source::kMemory)
                if ((reg = src.reg.get())) src.announce(WindowSched(lens.data(), blobs, W, live_cap, align));
            const WindowPass pass{"metainfo windows", D, [&](std::vector<WinChunk>& w) { return sched.next(w); }, place,
                                  span, D->s_main, D->s_a, crc ? D->s_b : nullptr, lens.data(), plens.data(), soff.data(),
                                  d_dig, d_state, d_sums, /*build_ahead=*/2, &st};
            r = run_windows(pass, src);
            st.max_live = sched.max_live();
        }
        // drain what was queued even after a read error (the windows' kernels read the buffers)
        const bool synced = hipStreamSynchronize(D->s_a) == hipSuccess &&
                            (!crc || hipStreamSynchronize(D->s_b) == hipSuccess) &&
                            hipStreamSynchronize(D->s_main) == hipSuccess;
        if (!r && !synced) {
            set_error(KRK_EHIP, "%s: sync failed", name);
            r = KRK_EHIP;
        }
        if constexpr (Source::kMemory) release_caller_pages(src, &st);
        if (!r) r = copy_out(digests_host, d_dig, n * 32, reg, "digest");
        if (!r && hi > lo) r = copy_out(sums_host + lo, d_sums + lo, (hi - lo) * 4, reg, "sums");
        if (host_th.joinable()) host_th.join();
        if (!r && host_rc) {
            t_err = host_err;
            r = host_rc;
        }
        for (size_t q = 0; !r && q < host.size(); ++q) {
            memcpy(digests_host + 32 * (size_t)host[q], &host_dig[32 * q], 32);
            if (const uint64_t np = host_sums_off[q + 1] - host_sums_off[q])
                memcpy(sums_host + soff[host[q]], &host_sums[host_sums_off[q]], np * 4);
        }
        st.host_blobs = host.size();
        t_last_call = st;
        return r;
    }
    // run() from the caller's buffers: page-locked blobs DMA'd or gathered as they are, pageable
    // ones registered for the gather (KRK_HOST_GATHER) or staged.
    int run_memory(Device* D, const krk_blob* blobs) {
        // KRK_PINNED_DIRECT=0 stages pinned sources too (A/B)
        static const bool allow_direct = !KRK_AB_ENV("KRK_PINNED_DIRECT") || atoi(KRK_AB_ENV("KRK_PINNED_DIRECT")) != 0;
        MemSource src(blobs, n);
        src.setup(on_host, allow_direct && src.all_pinned(on_host), host_gather_mode(), D->s_main);
        return run(D, src, 64, live_cap_for(D));
    }
};
}  // namespace

extern "C" {

int krk_window_stream_cap(uint64_t* cap) {
    KRK_CHECK(cap, KRK_EINVAL, "cap is NULL");
    KRK_DEVICE(D);
    *cap = window_stream_cap(D);
    return KRK_OK;
}

struct krk_window_sched {
    std::vector<uint64_t> lens;
    std::unique_ptr<WindowSched> s;
    std::vector<WinChunk> win;
};

int krk_window_sched_new(const uint64_t* lengths, uint64_t n, uint64_t window_bytes, uint64_t live_cap,
                         krk_window_sched** out) {
    KRK_CHECK(out && (n == 0 || lengths), KRK_EINVAL, "window_sched_new: null argument");
    KRK_CHECK(window_bytes >= 64 && live_cap >= 1, KRK_EINVAL, "window bytes >= 64 and live cap >= 1");
    KRK_CHECK(n <= 0xFFFFFFFFull, KRK_EINVAL, "more than 2^32 blobs");
    auto* w = new krk_window_sched();
    w->lens.assign(lengths, lengths + n);
    std::vector<uint32_t> all(n);
    for (uint64_t i = 0; i < n; ++i) all[i] = (uint32_t)i;
    w->s = std::make_unique<WindowSched>(w->lens.data(), std::move(all), window_bytes, live_cap);
    *out = w;
    return KRK_OK;
}

int krk_window_sched_next(krk_window_sched* w, uint32_t* blobs, uint64_t* offsets, uint64_t* lengths, uint64_t cap,
                          uint64_t* n_out) {
    KRK_CHECK(w && n_out, KRK_EINVAL, "window_sched_next: null argument");
    if (!w->s->next(w->win)) {
        *n_out = 0;
        return KRK_OK;
    }
    *n_out = w->win.size();
    KRK_CHECK(w->win.size() <= cap, KRK_ERANGE, "window has %zu chunks, capacity %llu", w->win.size(),
              (unsigned long long)cap);
    for (size_t k = 0; k < w->win.size(); ++k) {
        if (blobs) blobs[k] = w->win[k].blob;
        if (offsets) offsets[k] = w->win[k].off;
        if (lengths) lengths[k] = w->win[k].len;
    }
    return KRK_OK;
}

int krk_window_sched_drop(krk_window_sched* w, uint32_t blob, uint64_t* offset) {
    KRK_CHECK(w && offset, KRK_EINVAL, "window_sched_drop: null argument");
    KRK_CHECK(w->s->drop(blob, offset), KRK_EINVAL, "window_sched_drop: blob %u is neither live nor waiting", blob);
    return KRK_OK;
}

int krk_window_sched_set_chunk_cap(krk_window_sched* w, uint64_t max_chunk) {
    KRK_CHECK(w && max_chunk >= 64, KRK_EINVAL, "window_sched_set_chunk_cap: null schedule or cap < 64");
    w->s->set_max_chunk(max_chunk);
    return KRK_OK;
}

void krk_window_sched_free(krk_window_sched* w) { delete w; }

int krk_metainfo_digest_host(const krk_blob* blobs, uint64_t n, uint32_t* sums_host, uint8_t* digests_host) {
    KRK_DEVICE(D);
    int r = validate_blobs(blobs, n);
    if (r) return r;
    if (!n) return KRK_OK;
    KRK_CHECK(digests_host, KRK_EINVAL, "digests_host is NULL");
    WindowCall c("metainfo_digest_host", blobs, n, sums_host, digests_host);
    // SHA-256 host offload (KRK_OFFLOAD_AUTO by default): the planner's blobs are hashed and
    // piece-summed in place on host threads and never cross the host link.
    r = c.plan(D, kOffHostWhole, offload_threads(kOffHostWhole));
    if (r) return r;
    c.start([&](auto& l, auto& pl, auto& so) {
        std::vector<const uint8_t*> p;
        for (uint32_t i : c.host) p.push_back(blobs[i].data);
        offload_whole_host(p, l, pl, so, c.off_t, c.host_dig.data());
        return KRK_OK;
    });
    return c.run_memory(D, blobs);
}

// Whole-blob SHA-256 of host buffers (the Digester over many uploads at once): the same
// windows and schedule as krk_metainfo_digest_host without the CRC launches, and the
// planner's blobs hashed in place on host threads (KRK_OFFLOAD_HOST_SHA).
int krk_sha256_host(const uint8_t* const* data_host, const uint64_t* lengths, uint64_t n, uint8_t* digests_host) {
    KRK_DEVICE(D);
    if (!n) return KRK_OK;
    KRK_CHECK(data_host && lengths && digests_host, KRK_EINVAL, "sha256_host: null argument");
    for (uint64_t i = 0; i < n; ++i)
        KRK_CHECK(lengths[i] == 0 || data_host[i], KRK_EINVAL, "blob %llu: data is NULL", (unsigned long long)i);
    std::vector<krk_blob> blobs(n);
    for (uint64_t i = 0; i < n; ++i) blobs[i] = krk_blob{data_host[i], lengths[i], 1, 0};
    WindowCall c("sha256_host", blobs.data(), n, nullptr, digests_host, /*crc=*/false);
    int r = c.plan(D, kOffHostSha, offload_threads(kOffHostSha));
    if (r) return r;
    c.start([&](auto& l, auto&, auto&) {
        std::vector<const uint8_t*> p;
        for (uint32_t i : c.host) p.push_back(data_host[i]);
        offload_hash_host(p, l, c.off_t, c.host_dig.data());
        return KRK_OK;
    });
    return c.run_memory(D, blobs.data());
}

// The page-cache resident share of a file batch, from up to 64 evenly spaced files' first
// 16 MiB (mmap + mincore: no page is read).  -1 when none could be sampled.
static double files_resident_fraction(const krk_file_blob* files, uint64_t n) {
    const uint64_t step = std::max<uint64_t>(1, n / 64);
    const size_t pg = (size_t)sysconf(_SC_PAGESIZE);
    uint64_t in = 0, all = 0;
    std::vector<unsigned char> vec;
    for (uint64_t i = 0; i < n; i += step) {
        const size_t len = (size_t)std::min<uint64_t>(files[i].length, 16ull << 20);
        if (!len) continue;
        const int fd = open(files[i].path, O_RDONLY | O_CLOEXEC);
        if (fd < 0) continue;  // the pass reports it
        void* m = mmap(nullptr, len, PROT_READ, MAP_SHARED, fd, 0);
        close(fd);
        if (m == MAP_FAILED) continue;
        vec.assign((len + pg - 1) / pg, 0);
        if (mincore(m, len, vec.data()) == 0) {
            for (unsigned char c : vec) in += c & 1;
            all += vec.size();
        }
        munmap(m, len);
    }
    return all ? (double)in / (double)all : -1.0;
}

int krk_metainfo_digest_files(const krk_file_blob* files, uint64_t n, uint32_t* sums_host, uint8_t* digests_host) {
    KRK_DEVICE(D);
    if (!n) return KRK_OK;
    KRK_CHECK(files && digests_host, KRK_EINVAL, "metainfo_digest_files: null argument");
    int r = KRK_OK;
    for (uint64_t i = 0; i < n && !r; ++i) {
        KRK_CHECK(files[i].path, KRK_EINVAL, "file %llu: path is NULL", (unsigned long long)i);
        r = validate_pieces(files[i]);
    }
    if (r) return r;
    WindowCall c("metainfo_digest_files", files, n, sums_host, digests_host);
    // Host offload (AUTO by default): the planner's files are read, hashed and piece-summed
    // by host threads in one pass each and never cross the host link.
    // A batch mostly out of the page cache (the residency sample) is bound by the disk,
    // wherever its bytes are hashed: under AUTO, host threads would read the same disk and
    // take CPU from the window readers (cold 32 GiB leg: AUTO 13.4 GB/s against 14.8
    // GPU-only, profiles/r05/bench_files.json), so such a batch stays on the windows -- and
    // is read with O_DIRECT (below).
    int off_t = offload_threads(kOffHostWhole);
    c.resident = files_resident_fraction(files, n);
    const bool cold = c.resident >= 0 && c.resident < 0.5;
    if (cold && offload_auto()) off_t = 0;
    r = c.plan(D, kOffHostFiles, off_t);
    if (r) return r;
    c.start([&](auto& l, auto& pl, auto& so) {
        std::vector<const char*> p;
        for (uint32_t i : c.host) p.push_back(files[i].path);
        return offload_whole_files(p, l, pl, so, c.off_t, c.host_dig.data());
    });
    // O_DIRECT reads (Linux AIO, a window's chunks queued at once): KRK_FILE_DIRECT=1 / 0
    // force them on / off; by default a cold batch takes them (no page-cache copy, a deep
    // disk queue from one thread: 16.3 GB/s against 11.7 for 16 threads' page-cache preads
    // of the same window chunks, profiles/r05/disk_probe_aio.jsonl) and a cached one reads
    // the page cache.
    const char* fd_env = KRK_OP_ENV("KRK_FILE_DIRECT");
    const bool direct = c.direct_reads = fd_env ? atoi(fd_env) > 0 : cold;
    FileSource src(files, n, direct, /*async=*/true);
    // at most as many live blobs as this call holds file descriptors (a lease of the
    // process's budget, shared with every other file batch running now)
    FdLease fds(std::min<uint64_t>(direct ? direct_live_cap(D) : live_cap_for(D), n));
    return c.run(D, src, direct ? 4096 : 64, fds.n);
}

int krk_windows_last_call(uint64_t* max_live, int* windows, uint64_t* host_blobs) {
    if (max_live) *max_live = t_last_call.max_live;
    if (windows) *windows = t_last_call.windows;
    if (host_blobs) *host_blobs = t_last_call.host_blobs;
    return KRK_OK;
}

int krk_windows_last_copyout(uint64_t* live_registered) {
    KRK_CHECK(live_registered, KRK_EINVAL, "live_registered is NULL");
    *live_registered = t_last_call.live_at_copyout;
    return KRK_OK;
}

int krk_windows_last_direct(int* direct_windows) {
    KRK_CHECK(direct_windows, KRK_EINVAL, "direct_windows is NULL");
    *direct_windows = t_last_call.direct_windows;
    return KRK_OK;
}

int krk_set_host_gather(int mode) {
    KRK_CHECK(mode >= -1 && mode <= 1, KRK_EINVAL, "host gather mode %d outside -1 (auto), 0, 1", mode);
    g_host_gather.store(mode);
    return KRK_OK;
}

// The windows' gather launch on spans the caller lays out (tests): every span is checked as
// the windows check theirs before anything is queued.
int krk_gather_spans_dev(const void* const* src, void* const* dst, const uint64_t* n, uint64_t count, void* stream) {
    if (!count) return KRK_OK;
    KRK_CHECK(src && dst && n, KRK_EINVAL, "gather_spans_dev: null argument");
    KRK_DEVICE(D);
    MappedAtHost at_host;
    std::vector<GatherSpan> spans;
    spans.reserve(count);
    for (uint64_t i = 0; i < count; ++i) {
        KRK_CHECK(!(reinterpret_cast<uintptr_t>(dst[i]) & 15), KRK_EINVAL,
                  "gather_spans_dev: dst of span %llu is not 16-byte aligned", (unsigned long long)i);
        if (!n[i]) continue;
        KRK_CHECK(n[i] < (1ull << 60) && dst[i] && device_writable(dst[i], (n[i] + 15) & ~15ull), KRK_EINVAL,
                  "gather_spans_dev: dst of span %llu must be device-writable over its length rounded up to 16",
                  (unsigned long long)i);
        KRK_CHECK(src[i] && at_host(src[i], n[i]), KRK_EINVAL,
                  "gather_spans_dev: src of span %llu is not page-locked memory mapped at its host address",
                  (unsigned long long)i);
        spans.push_back({static_cast<uint8_t*>(dst[i]), static_cast<const uint8_t*>(src[i]), n[i]});
    }
    return run_gather(D, spans, pick(D, stream));
}

int krk_windows_last_gather(int* gather_windows, uint64_t* registered_bytes, double* register_seconds) {
    if (gather_windows) *gather_windows = t_last_call.gather_windows;
    if (registered_bytes) *registered_bytes = t_last_call.registered_bytes;
    if (register_seconds) *register_seconds = t_last_call.register_s;
    return KRK_OK;
}

int krk_windows_last_phases(double* loop_s, double* acquire_s, double* fill_s, double* enqueue_s,
                            double* resident, int* direct_reads) {
    if (resident) *resident = t_last_call.resident;
    if (direct_reads) *direct_reads = t_last_call.direct_reads ? 1 : 0;
    if (loop_s) *loop_s = t_last_call.loop_s;
    if (acquire_s) *acquire_s = t_last_call.acquire_s;
    if (fill_s) *fill_s = t_last_call.fill_s;
    if (enqueue_s) *enqueue_s = t_last_call.enqueue_s;
    return KRK_OK;
}

}  // extern "C"
