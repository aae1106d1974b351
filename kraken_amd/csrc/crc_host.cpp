// crc_host.cpp -- the C ABI's host-resident CRC-only calls: krk_piece_sums_host with its
// host / GPU split and NUMA hand-out, krk_piece_sums_files with its host placement, and
// krk_verify_pieces_host.  Their GPU share goes through the window pass (window_pass.cpp).
#include <errno.h>
#include <fcntl.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <chrono>
#include <optional>

#include "offload.hpp"
#include "window_pass.hpp"

using namespace krk;

// The GPU pass of the CRC-only calls: the blobs' bytes packed end to end into windows
// (PackSched, chunks `place` apart), up on s_a by the way the source allows (window_pass.cpp)
// and through the CRC kernel on s_b; the sums the blobs cover back to the caller.  The windows
// are built in the loop (a packed window has few chunks, and krk_piece_sums_host's host
// threads already fill the CPU budget a build-ahead thread would share; not measured).
template <class Blob, class Source>
static int crc_pass(Device* D, const char* what, const Blob* blobs, uint64_t n, Source& src, size_t place,
                    uint32_t* sums_host) {
    uint64_t lo, hi;
    sums_span(blobs, n, &lo, &hi);
    if (hi == lo) return KRK_OK;
    KRK_CHECK(sums_host, KRK_EINVAL, "sums_host is NULL");
    KRK_CHECK(n <= 0xFFFFFFFFull, KRK_EINVAL, "more than 2^32 blobs");
    const size_t W = window_bytes();  // a multiple of 1 MiB
    KRK_CHECK(W % place == 0, KRK_EINVAL, "%s: window of %zu bytes is no multiple of %zu", what, W, place);
    uint32_t* d_sums = nullptr;
    DevMem mem;
    KRK_HIP(mem.alloc(&d_sums, hi * 4));
    KRK_HIP(hipMemset(d_sums, 0, hi * 4));
    std::vector<uint64_t> lens(n), soff(n);
    std::vector<int64_t> plens(n);
    for (uint64_t i = 0; i < n; ++i) {
        lens[i] = blobs[i].length;
        plens[i] = blobs[i].piece_length;
        soff[i] = blobs[i].sums_offset;
    }
    PackSched sched(lens.data(), n, W, place);
    const WindowPass pass{what, D, [&](std::vector<WinChunk>& w) { return sched.next(w); }, place, W, D->s_a, nullptr,
                          D->s_b, lens.data(), plens.data(), soff.data(), nullptr, nullptr, d_sums, /*build_ahead=*/0,
                          nullptr};
    int r = run_windows(pass, src);
    // drain what was queued even after a read error (the windows' kernels read the buffers)
    if (hipStreamSynchronize(D->s_b) != hipSuccess && !r) { set_error(KRK_EHIP, "sync failed"); r = KRK_EHIP; }
    if (!r && hipMemcpy(sums_host + lo, d_sums + lo, (hi - lo) * 4, hipMemcpyDeviceToHost) != hipSuccess) {
        set_error(KRK_EHIP, "sums copy-out failed");
        r = KRK_EHIP;
    }
    return r;
}

extern "C" {

// krk_piece_sums_host / krk_verify_pieces_host: the reference hashes each received
// piece on the host (lib/torrent/storage/agentstorage/torrent.go:182-193), and one host
// core's PCLMUL CRC (~12 GB/s) is within a few x of what the host link carries to the
// GPU, so the batch is split by bytes, whole pieces at a time, between host threads and
// the GPU pass in proportion to the measured rates (planner_rates):
//  * pinned caller bytes: the GPU side costs no host CPU (DMA straight into the device
//    window), so the GPU takes h2d / (h2d + threads x crc) of the bytes;
//  * pageable bytes: the GPU side needs a host memcpy into pinned staging, so it helps
//    only if a core copies faster than it CRCs; otherwise everything stays on the host.
// Host threads = the CPUs this process may use (affinity and cgroup quota).
struct PieceTask {
    const uint8_t* p;
    uint64_t n;
    uint64_t out;
};

// NUMA-aware hand-out of host CRC tasks (runs of ~8 MiB), opt-in: the node of each task's
// first, middle and last page (move_pages, one call for all of them) and, per claim, the
// node of the CPU the claiming thread runs on; a thread takes the next task of its own node
// and steals from the others once its node has none (KRK_CRC_NUMA=1), and with
// KRK_CRC_NUMA=2, for a batch spread over both sockets' memory, a thread that takes another
// node's task runs it on that node's CPUs (NodeVisit).  Off by default (0 = one plain
// cursor): on the GPU boxes' two-socket hosts, five interleaved A/B runs of the three modes
// (profiles/r05/host_mem_probe_numa.jsonl) moved the spread-buffer case by +33, +8, +14,
// -14, +31 % with visits and left every one-node buffer equal or a few % lower -- inside the
// host's minute-to-minute swing, not a win to ship.
class NodeTasks {
  public:
    // sysfs's CPU lists per node, parsed once: node of each CPU and the CPUs of each node
    struct Topology {
        std::vector<int> node_of_cpu = std::vector<int>(CPU_SETSIZE, 0);
        std::vector<cpu_set_t> cpus;
        Topology() {
            for (int nd = 0; nd < 64; ++nd) {
                FILE* f = fopen(("/sys/devices/system/node/node" + std::to_string(nd) + "/cpulist").c_str(), "r");
                if (!f) break;
                char buf[4096] = {0};
                const size_t got = fread(buf, 1, sizeof buf - 1, f);
                fclose(f);
                buf[got] = 0;
                cpu_set_t set;
                CPU_ZERO(&set);
                for (char* q = buf; *q && *q != '\n';) {  // "0-63,128-191"
                    char* e = nullptr;
                    const long lo = strtol(q, &e, 10);
                    if (e == q) break;
                    long hi = lo;
                    if (*e == '-') hi = strtol(e + 1, &e, 10);
                    for (long c = lo; c <= hi && c < CPU_SETSIZE; ++c) {
                        node_of_cpu[(size_t)c] = nd;
                        CPU_SET((int)c, &set);
                    }
                    q = (*e == ',') ? e + 1 : e;
                }
                cpus.push_back(set);
            }
        }
    };
    static const Topology& topo() {
        static const Topology t;
        return t;
    }
    static int cpu_node(int cpu) { return cpu >= 0 && cpu < CPU_SETSIZE ? topo().node_of_cpu[(size_t)cpu] : 0; }
    // the CPUs of node nd (nullptr when sysfs did not list it)
    static const cpu_set_t* node_cpus(int nd) {
        return nd >= 0 && (size_t)nd < topo().cpus.size() ? &topo().cpus[(size_t)nd] : nullptr;
    }
    // node visits (mode 2) only for a batch spread over nodes: two or more nodes holding at least
    // an eighth of the tasks each.  A batch on one node keeps its threads spread over both
    // sockets (moving all of them to the memory's socket measured 10 % slower).
    bool visits() const {
        if (mode_ < 2) return false;
        std::vector<size_t> on(list_.size(), 0);
        for (int nd : node_)
            if (nd >= 0) ++on[(size_t)nd];
        size_t big = 0;
        for (size_t c : on) big += c * 8 >= node_.size();
        return big >= 2;
    }
    int node_of(size_t task) const { return task < node_.size() ? node_[task] : -1; }
    // tasks' first, middle and last pages -> per-node lists; a task whose three pages are
    // not on one node (interleaved memory) is nobody's: it goes on its first page's list and
    // is never visited.  False when there is one node or the query fails.
    bool build(const std::vector<const void*>& first, const std::vector<const void*>& mid,
               const std::vector<const void*>& last) {
        const char* v = KRK_AB_ENV("KRK_CRC_NUMA");
        mode_ = v ? atoi(v) : 0;
        const size_t n = first.size();
        if (mode_ <= 0 || n < 2) return false;
        std::vector<int> status(3 * n, -1);
        std::vector<void*> pages(3 * n);
        auto page = [](const void* q) { return reinterpret_cast<void*>(reinterpret_cast<uintptr_t>(q) & ~uintptr_t(4095)); };
        for (size_t i = 0; i < n; ++i) {
            pages[3 * i] = page(first[i]);
            pages[3 * i + 1] = page(mid[i]);
            pages[3 * i + 2] = page(last[i]);
        }
        if (syscall(SYS_move_pages, 0, (unsigned long)pages.size(), pages.data(), nullptr, status.data(), 0) != 0)
            return false;
        int nodes = 0;
        for (int st : status) nodes = std::max(nodes, st + 1);
        if (nodes < 2) return false;
        list_.assign((size_t)nodes, {});
        node_.assign(n, -1);
        for (size_t i = 0; i < n; ++i) {
            const int a = status[3 * i], b = status[3 * i + 1], c = status[3 * i + 2];
            if (a >= 0 && a == b && b == c) node_[i] = a;
            list_[(size_t)std::max(0, a)].push_back(i);
        }
        next_ = std::vector<std::atomic<size_t>>(list_.size());
        return true;
    }
    // the next task for a thread on the CPU it runs on now (SIZE_MAX: none left)
    size_t claim() {
        const int home = std::min<int>((int)list_.size() - 1, cpu_node(sched_getcpu()));
        for (size_t k = 0; k < list_.size(); ++k) {
            const size_t nd = ((size_t)home + k) % list_.size();
            if (next_[nd].load(std::memory_order_relaxed) >= list_[nd].size()) continue;
            const size_t i = next_[nd].fetch_add(1);
            if (i < list_[nd].size()) return list_[nd][i];
        }
        return SIZE_MAX;
    }

  private:
    int mode_ = 0;
    std::vector<int> node_;
    std::vector<std::vector<size_t>> list_;
    std::vector<std::atomic<size_t>> next_;
};

// Mode 2 of KRK_CRC_NUMA (the default): a thread that takes a task of another node moves to
// that node's CPUs for the task (within the CPUs it may use) and back afterwards.
struct NodeVisit {
    cpu_set_t old;
    bool moved = false;
    explicit NodeVisit(int nd) {
        if (sched_getaffinity(0, sizeof old, &old) != 0) return;
        const cpu_set_t* on = NodeTasks::node_cpus(nd);
        if (!on) return;
        cpu_set_t to;
        CPU_AND(&to, &old, on);
        if (CPU_COUNT(&to) == 0) return;
        moved = sched_setaffinity(0, sizeof to, &to) == 0;
    }
    ~NodeVisit() {
        if (moved) sched_setaffinity(0, sizeof old, &old);
    }
};

// The pinned-batch split of each device, learned from earlier calls (per device).
//  * frac: the balanced GPU share -- where both sides would have ended together at the
//    rates the last split call measured (-1: none yet; first call: the rates' model, <= 10 %);
//  * r_split / r_host: whole-call throughput (bytes / wall time) of calls at that split and
//    of host-only calls.  The DMA reads share host memory with the CRC threads, so a balanced
//    split can still lose to the host alone (C4's 20 GiB pinned blob on one box: 131 GB/s at
//    the balanced 27 % against 260 host-only; f1verify on another: 282 at 10 % against 228).
//    So the first split call sets up the windows (not a sample), the second measures the
//    split, the next runs host-only, later calls take whichever measured faster, and every
//    16th call re-measures the other one.
struct CrcSplit {
    std::mutex mu;
    double frac = -1, r_split = 0, r_host = 0;
    uint64_t calls = 0;
    bool warm = false;  // a split call has run: the staging windows exist (the first pays their set-up)
    bool use_split() const { return r_host <= 0 || r_split >= r_host; }
};
static CrcSplit g_crc_split[kMaxDevs];
static CrcSplit& crc_split_of(int dev) { return g_crc_split[(dev >= 0 && dev < kMaxDevs) ? dev : 0]; }
static thread_local uint64_t t_split_gpu = 0, t_split_host = 0;

int krk_piece_sums_host(const krk_blob* blobs, uint64_t n_blobs, uint32_t* sums_host) {
    int r = validate_blobs(blobs, n_blobs);
    if (r) return r;
    uint64_t lo, hi;
    sums_span(blobs, n_blobs, &lo, &hi);
    if (hi == lo) return KRK_OK;
    KRK_CHECK(sums_host, KRK_EINVAL, "sums_host is NULL");
    // Concurrent callers (the agent's dispatcher verifying from several goroutines) share the
    // CPU budget instead of each starting a full set of threads.
    static std::atomic<int> callers{0};
    struct Caller {
        Caller() { callers.fetch_add(1); }
        ~Caller() { callers.fetch_sub(1); }
    } caller;
    const int T = std::max(1, host_threads_for_call() / std::max(1, callers.load()));
    bool all_pinned = true;
    double bytes = 0;
    for (uint64_t i = 0; i < n_blobs; ++i) {
        bytes += (double)blobs[i].length;
        if (all_pinned && blobs[i].length && !host_pinned(blobs[i].data, blobs[i].length)) all_pinned = false;
    }
    const char* forced = KRK_OP_ENV("KRK_CRC_GPU_FRACTION");
    // Pageable batches stay on the host threads and need no device; pinned (or forced) ones
    // split by the device's rates.
    Device* D = nullptr;
    if (all_pinned || forced) {
        int drc = KRK_OK;
        D = device(&drc);
        if (!D) return drc;
    }
    const Rates R = D ? planner_rates(D) : Rates{};
    // Pinned bytes: the GPU's share starts from the rates' model, capped at 10 %, and is then
    // set from what the previous calls measured (each side's bytes over its own wall time
    // while both ran): the DMA reads share the host's memory with the CRC threads, so the
    // static model overestimates the GPU side (f1verify, same box: 10 % 282 GB/s, 20 % 182,
    // host only 228).  Pageable bytes stay on the host: a copy into pinned staging per byte
    // cost more than the GPU saved (host only 241 GB/s, the model's split 202).
    const double c = R.host_crc, H = T * c;
    double gpu_frac = 0.0;
    CrcSplit& cs = crc_split_of(D ? D->id : 0);
    if (all_pinned && !forced) {
        std::lock_guard<std::mutex> g(cs.mu);
        const uint64_t k = ++cs.calls;
        bool split = cs.r_split <= 0 || (cs.r_host > 0 && cs.use_split());
        if (cs.r_split > 0 && cs.r_host <= 0) split = false;  // the second call: host only
        else if (k % 16 == 0) split = !split;                    // re-measure the other side
        gpu_frac = split ? (cs.frac >= 0 ? cs.frac : std::min(0.10, R.h2d / (R.h2d + H))) : 0.0;
    }
    if (forced) gpu_frac = std::clamp(atof(forced), 0.0, 1.0);
    // Whole pieces to the GPU until its share of the bytes is reached, the rest to the host.
    const double quota = gpu_frac * bytes;
    double gbytes = 0;
    std::vector<krk_blob> gpu;
    std::vector<uint64_t> gpu_dst;  // sums_host index of each GPU blob's first sum
    std::vector<PieceTask> host;
    uint64_t g_sums = 0;
    for (uint64_t i = 0; i < n_blobs; ++i) {
        const krk_blob& b = blobs[i];
        const uint64_t P = (uint64_t)b.piece_length, np = krk_num_pieces(b.length, b.piece_length);
        uint64_t q = 0;  // pieces [0, q) of this blob go to the GPU
        while (q < np && gbytes < quota) {
            gbytes += (double)std::min(P, b.length - q * P);
            ++q;
        }
        if (q) {
            gpu.push_back(krk_blob{b.data, std::min(b.length, q * P), b.piece_length, g_sums});
            gpu_dst.push_back(b.sums_offset);
            g_sums += q;
        }
        for (uint64_t k = q; k < np; ++k) host.push_back({b.data + k * P, std::min(P, b.length - k * P), b.sums_offset + k});
    }
    // The host share on the host pool's idle threads (and this thread once the GPU pass is
    // queued): at most T threads, one per 8 MiB of host bytes (a small share stays on the
    // calling thread).
    const auto t0 = std::chrono::steady_clock::now();
    std::atomic<int64_t> host_end_ns{0};
    std::atomic<size_t> left{host.size()};
    double hbytes_all = 0;
    for (const PieceTask& h : host) hbytes_all += (double)h.n;
    const int TH = (int)std::min<size_t>({(size_t)T, host.size(), (size_t)(hbytes_all / (8 << 20)) + 1});
    // A task is a run of consecutive pieces (~8 MiB): one thread streams through adjacent
    // bytes, which the hardware prefetchers follow (256 KiB tasks handed out one at a time ran
    // C4's host side ~30 % below contiguous spans, profiles/r04/host_mem_probe_lib.jsonl).
    static const double task_bytes = [] {  // KRK_CRC_TASK_KB overrides the run length (A/B)
        const char* v = KRK_AB_ENV("KRK_CRC_TASK_KB");
        return v ? atof(v) * 1024.0 : double(8u << 20);
    }();
    const size_t G = host.empty() ? 1
                                  : std::max<size_t>(1, (size_t)(task_bytes / std::max(1.0, hbytes_all / host.size())));
    const size_t n_tasks = (host.size() + G - 1) / G;
    left.store(n_tasks);
    NodeTasks nt;
    bool numa = false;
    if (n_tasks >= 2) {
        std::vector<const void*> first(n_tasks), mid(n_tasks), last(n_tasks);
        for (size_t t = 0; t < n_tasks; ++t) {
            const size_t j0 = t * G, j1 = std::min(host.size(), (t + 1) * G) - 1;
            first[t] = host[j0].p;
            mid[t] = host[(j0 + j1) / 2].p + host[(j0 + j1) / 2].n / 2;
            last[t] = host[j1].p + (host[j1].n ? host[j1].n - 1 : 0);
        }
        numa = nt.build(first, mid, last);
    }
    const bool visits = numa && nt.visits();
    HostBatch hb(n_tasks, gpu.empty() ? TH - 1 : TH, [&](size_t t) {
        if (numa) {  // every call claims one task: n_tasks calls take them all
            const size_t k = nt.claim();
            if (k != SIZE_MAX) t = k;
        }
        std::optional<NodeVisit> visit;
        if (visits && nt.node_of(t) >= 0 && nt.node_of(t) != NodeTasks::cpu_node(sched_getcpu()))
            visit.emplace(nt.node_of(t));
        for (size_t j = t * G; j < std::min(host.size(), (t + 1) * G); ++j)
            sums_host[host[j].out] = host_crc32_update(0, host[j].p, host[j].n);
        if (left.fetch_sub(1) == 1)  // the last task: the host side's wall time
            host_end_ns.store(
                std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count());
    });
    double gpu_s = 0;
    if (!gpu.empty()) {
        std::vector<uint32_t> gs(g_sums);
        // pinned bytes go up straight from the caller's pages (a DMA a chunk or the gather),
        // pageable ones through the pinned staging windows
        MemSource src(gpu.data(), gpu.size());
        src.setup({}, all_pinned, /*gather_mode=*/-1, D->s_a);
        r = crc_pass(D, "piece_sums_host", gpu.data(), gpu.size(), src, 16, gs.data());
        gpu_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (!r)
            for (size_t j = 0; j < gpu.size(); ++j) {
                const uint64_t cnt = krk_num_pieces(gpu[j].length, gpu[j].piece_length);
                memcpy(sums_host + gpu_dst[j], gs.data() + gpu[j].sums_offset, cnt * 4);
            }
    }
    hb.join();
    const double hbytes = bytes - gbytes, host_s = host_end_ns.load() * 1e-9;
    t_split_gpu = (uint64_t)gbytes;
    t_split_host = (uint64_t)hbytes;
    const double call_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (!r && all_pinned && !forced && bytes >= (128u << 20) && call_s > 0) {
        std::lock_guard<std::mutex> g(cs.mu);
        auto ema = [](double& x, double v) { x = x > 0 ? 0.5 * x + 0.5 * v : v; };
        if (gbytes > 0 && !cs.warm) {
            cs.warm = true;  // not a sample: this call allocated and pinned the windows
        } else if (gbytes > 0) {
            ema(cs.r_split, bytes / call_s);
            if (gbytes >= (64u << 20) && hbytes >= (64u << 20) && gpu_s > 0 && host_s > 0) {
                // the split where both sides would have ended together at the rates just measured
                const double rg = gbytes / gpu_s, rh = hbytes / host_s, want = rg / (rg + rh);
                cs.frac = cs.frac >= 0 ? 0.5 * cs.frac + 0.5 * want : want;
            }
        } else {
            ema(cs.r_host, bytes / call_s);
        }
    }
    return r;
}

int krk_crc_host_split(uint64_t* gpu_bytes, uint64_t* host_bytes, double* gpu_fraction) {
    if (gpu_bytes) *gpu_bytes = t_split_gpu;
    if (host_bytes) *host_bytes = t_split_host;
    if (gpu_fraction) {
        CrcSplit& cs = crc_split_of(t_dev);
        std::lock_guard<std::mutex> g(cs.mu);
        *gpu_fraction = cs.r_host > 0 && !cs.use_split() ? 0.0 : cs.frac;
    }
    return KRK_OK;
}

// The host placement of krk_piece_sums_files: what the reference's Generate does with a
// cache file (lib/metainfogen/generator.go:41-58 -> core.NewMetaInfo over the file reader,
// core/metainfo.go:157-179), spread over the host pool.  Each file is cut into spans of
// whole pieces (~16 MiB); a span's thread preads it in 512 KiB chunks into a buffer of its
// own and folds each chunk into the piece's CRC while the chunk is in cache.  The same
// bytes through the GPU cost the same pread (into a pinned window) plus the host link, so
// where the host's CRC capacity exceeds the link this placement is faster.
static int piece_sums_files_host(const krk_file_blob* files, uint64_t n, uint32_t* sums_host) {
    struct Span {
        uint64_t file, first, pieces;
    };
    std::vector<Span> spans;
    constexpr uint64_t kSpan = 16ull << 20;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t P = (uint64_t)files[i].piece_length, np = krk_num_pieces(files[i].length, files[i].piece_length);
        const uint64_t per = std::max<uint64_t>(1, kSpan / P);
        for (uint64_t k = 0; k < np; k += per) spans.push_back({i, k, std::min(per, np - k)});
    }
    std::mutex emu;
    std::string emsg;
    std::atomic<bool> failed{false};
    auto fail = [&](const std::string& m) {
        std::lock_guard<std::mutex> g(emu);
        if (emsg.empty()) emsg = m;
        failed.store(true);
    };
    const int T = std::max(1, host_threads_for_call());
    // 512 KiB reads: 328 GB/s against 277 at the oracle's 32 KiB, alternated with the oracle
    // on one box (profiles/r06/c5regen_files_chunk_ab.jsonl)
    constexpr size_t kChunk = 512u << 10;
    host_parallel_for(spans.size(), T - 1, [&](size_t s) {
        if (failed.load(std::memory_order_relaxed)) return;
        thread_local std::vector<uint8_t> buf;
        if (buf.size() < kChunk) buf.resize(kChunk);
        const Span& sp = spans[s];
        const krk_file_blob& f = files[sp.file];
        const int fd = open(f.path, O_RDONLY | O_CLOEXEC);
        if (fd < 0) {
            fail(std::string("open ") + f.path + ": " + strerror(errno));
            return;
        }
        const uint64_t P = (uint64_t)f.piece_length;
        for (uint64_t k = sp.first; k < sp.first + sp.pieces; ++k) {
            uint64_t a = k * P;
            const uint64_t e = std::min(f.length, a + P);
            uint32_t c = 0;
            while (a < e) {
                const ssize_t got = pread(fd, buf.data(), std::min<uint64_t>(kChunk, e - a), (off_t)a);
                if (got < 0 && errno == EINTR) continue;
                if (got <= 0) {
                    fail(std::string("read blob: ") + f.path + ": " + (got < 0 ? strerror(errno) : "unexpected EOF"));
                    close(fd);
                    return;
                }
                c = host_crc32_update(c, buf.data(), (size_t)got);
                a += (uint64_t)got;
            }
            sums_host[f.sums_offset + k] = c;
        }
        close(fd);
    });
    if (failed.load()) {
        set_error(KRK_EIO, "%s", emsg.c_str());
        return KRK_EIO;
    }
    return KRK_OK;
}

int krk_piece_sums_files(const krk_file_blob* files, uint64_t n, uint32_t* sums_host) {
    if (!n) return KRK_OK;
    KRK_CHECK(files, KRK_EINVAL, "files is NULL");
    uint64_t lo, hi, bytes = 0;
    for (uint64_t i = 0; i < n; ++i) {
        KRK_CHECK(files[i].path, KRK_EINVAL, "file %llu: path is NULL", (unsigned long long)i);
        KRK_CHECK(files[i].piece_length > 0, KRK_EINVAL, "piece length must be positive");
        bytes += files[i].length;
    }
    sums_span(files, n, &lo, &hi);
    // An empty file has no piece to read, but Generate opens it (GetCacheFileReader,
    // lib/metainfogen/generator.go:47-49): a missing or unreadable one fails.
    for (uint64_t i = 0; i < n; ++i)
        if (files[i].length == 0) {
            const int fd = open(files[i].path, O_RDONLY | O_CLOEXEC);
            KRK_CHECK(fd >= 0, KRK_EIO, "open %s: %s", files[i].path, strerror(errno));
            close(fd);
        }
    if (hi == 0) return KRK_OK;
    KRK_CHECK(sums_host, KRK_EINVAL, "sums_host is NULL");
    // CRC placement (krk_set_crc_placement, else the measured crossover; HOST without a device)
    int prc = KRK_OK;
    const int where = resolve_crc_placement(KRK_PLACE_AUTO, &prc);
    if (where < 0) return prc;
    t_split_gpu = where == KRK_PLACE_GPU ? bytes : 0;
    t_split_host = where == KRK_PLACE_GPU ? 0 : bytes;
    if (where != KRK_PLACE_GPU) return piece_sums_files_host(files, n, sums_host);
    KRK_DEVICE(D);
    const bool want_direct = KRK_OP_ENV("KRK_FILE_DIRECT") && atoi(KRK_OP_ENV("KRK_FILE_DIRECT")) > 0;
    // every read by par_read; every file starts page-aligned in the window (O_DIRECT)
    FileSource src(files, n, want_direct, /*async=*/false);
    return crc_pass(D, "piece_sums_files", files, n, src, 4096, sums_host);
}

int krk_verify_pieces_host(const uint8_t* const* data, const uint64_t* lengths, const uint32_t* expected,
                           uint64_t n, uint8_t* ok_out) {
    if (!n) return KRK_OK;
    KRK_CHECK(data && lengths && expected && ok_out, KRK_EINVAL, "verify_pieces_host: null argument");
    // Each piece is a one-piece blob; an empty piece sums to 0 (crc32 of nothing).
    std::vector<krk_blob> blobs(n);
    for (uint64_t i = 0; i < n; ++i)
        blobs[i] = krk_blob{data[i], lengths[i], (int64_t)std::max<uint64_t>(lengths[i], 1), i};
    std::vector<uint32_t> sums(n, 0);
    int r = krk_piece_sums_host(blobs.data(), n, sums.data());
    if (r) return r;
    for (uint64_t i = 0; i < n; ++i) ok_out[i] = sums[i] == expected[i];
    return KRK_OK;
}

}  // extern "C"
