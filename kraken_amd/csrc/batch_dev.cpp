// batch_dev.cpp -- the C ABI's device-resident batch calls: piece sums, SHA-256 with its host
// share and tail handoff, the fused metainfo + digest batch, the chunk (window) steps and
// piece verification over blobs already in HBM.
#include "offload.hpp"
#include "runtime.hpp"
#include "staging.hpp"

using namespace krk;

extern "C" {

int krk_piece_sums_dev(const krk_blob* blobs, uint64_t n_blobs, uint32_t* sums_dev, void* stream) {
    KRK_DEVICE(D);
    return piece_sums_dev(D, blobs, n_blobs, sums_dev, pick(D, stream));
}

// The chains of a device-resident batch host threads finish (krk_set_sha_host_offload; empty
// when it is off or would not shorten the batch), and a per-blob mark: whole blobs
// (`start` empty: offload_plan), or the tails of chains the GPU starts (tail_plan) when those
// end the batch sooner -- the model's ends compared, KRK_SHA_TAIL=0 keeps whole blobs only.
struct HostShare {
    std::vector<uint32_t> idx;
    std::vector<uint64_t> start;  // tail handoff: the GPU's prefix of chain idx[k]
};
struct TailStats {
    uint64_t chains = 0, gpu_prefix_bytes = 0;
};
static thread_local TailStats t_last_tail;  // krk_sha_last_tail
static HostShare offload_split(Device* D, const uint64_t* lens, uint64_t n, std::vector<char>& on_host) {
    on_host.assign(n, 0);
    HostShare hs;
    const int T = offload_threads();
    if (T <= 0 || n == 0) return hs;
    const Rates R = planner_rates(D);
    double g = 0, h = 0;
    hs.idx = offload_plan(lens, n, T, R, &g, &h);
    static const bool tails = !KRK_AB_ENV("KRK_SHA_TAIL") || atoi(KRK_AB_ENV("KRK_SHA_TAIL")) != 0;
    if (tails) {
        const double whole = std::max(g, h);
        TailPlan tp = tail_plan(lens, n, T, R);
        if (!tp.idx.empty() && tp.end_s < 0.95 * whole) {
            hs.idx = std::move(tp.idx);
            hs.start = std::move(tp.start);
        }
    }
    for (uint32_t i : hs.idx) on_host[i] = 1;
    t_last_tail = {hs.start.empty() ? 0 : hs.idx.size(), 0};
    for (uint64_t y : hs.start) t_last_tail.gpu_prefix_bytes += y;
    return hs;
}

// The GPU's side of a batch: whole chains, and the prefixes of the chains whose tails host
// threads finish -- those write their midstates to `note` (page-locked, coherent host memory
// the kernel stores to over PCIe) instead of a digest.
static void host_share_jobs(const HostShare& hs, const uint8_t* const* ptrs, std::vector<ShaJob>& jobs) {
    for (size_t k = 0; k < hs.start.size(); ++k)
        if (hs.start[k]) {
            ShaJob j = full_job(ptrs[hs.idx[k]], hs.start[k], hs.idx[k]);
            j.flags = 0;  // a midstate, not a digest
            jobs.push_back(j);
        }
}

// Page-locked note for the midstates of n chains, every word kTailSentinel; its device
// address in *dev.
static int tail_note(uint64_t n, uint32_t** host, uint32_t** dev) {
    *host = *dev = nullptr;
    KRK_HIP(hipHostMalloc(reinterpret_cast<void**>(host), std::max<uint64_t>(n, 1) * 32,
                          hipHostMallocMapped | hipHostMallocCoherent));
    memset(*host, 0xFF, std::max<uint64_t>(n, 1) * 32);
    static_assert(kTailSentinel == 0xFFFFFFFFu, "the note's fill");
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, *host, 0) != hipSuccess) {
        hipHostFree(*host);
        *host = nullptr;
        KRK_CHECK(false, KRK_EHIP, "sha256 tail handoff: no device address for the midstate note");
    }
    *dev = static_cast<uint32_t*>(d);
    return KRK_OK;
}

// Hash the host threads' chains (their D2H waits for `ready`; tails wait for their midstates
// in `note`, written by the launch `gpu_done` follows) and store the digests into digests_dev
// on stream s.
static int offload_run(Device* D, const HostShare& hs, const uint8_t* const* ptrs, const uint64_t* lens,
                       hipEvent_t ready, uint8_t* digests_dev, hipStream_t s, const uint32_t* note = nullptr,
                       hipEvent_t gpu_done = nullptr) {
    const std::vector<uint32_t>& host = hs.idx;
    std::vector<const uint8_t*> p(host.size());
    std::vector<uint64_t> l(host.size());
    for (size_t j = 0; j < host.size(); ++j) {
        p[j] = ptrs[host[j]];
        l[j] = lens[host[j]];
    }
    std::vector<uint8_t> dig(32 * host.size());
    TailSrc tail{note, host.data(), hs.start.data(), gpu_done};
    int r = offload_hash(D, p, l, offload_threads(), ready, dig.data(), hs.start.empty() ? nullptr : &tail);
    return r ? r : offload_store(D, host, dig.data(), digests_dev, s);
}

// A batch's SHA-256 launch plus its host share, in two steps so that other launches (the
// CRC) can be queued between them: launch() queues the GPU part on `s` (whole chains, and
// the prefixes of the tails with their midstate note); finish() runs the host threads'
// chains beside it and returns once their digests are queued into digests_dev on `s_out`
// (with tails: once the launch has ended too, so the note can go).
struct ShaHostShare {
    const HostShare& hs;
    uint32_t *note = nullptr, *note_dev = nullptr;
    Event done;
    int r = KRK_OK;
    explicit ShaHostShare(const HostShare& h) : hs(h) {}
    ShaHostShare(const ShaHostShare&) = delete;
    ShaHostShare& operator=(const ShaHostShare&) = delete;
    ~ShaHostShare() { release(nullptr); }
    void release(hipStream_t s) {
        if (note) {  // the launch wrote the note: it goes only once the launch has ended
            if (done) hipEventSynchronize(done);
            else if (s) hipStreamSynchronize(s);
            hipHostFree(note);
            note = nullptr;
        }
    }
    int launch(Device* D, const std::vector<char>& on_host, const uint8_t* const* ptrs, const uint64_t* lens,
               uint64_t n, uint8_t* digests_dev, hipStream_t s) {
        std::vector<ShaJob> jobs;
        jobs.reserve(n);
        for (uint64_t i = 0; i < n; ++i)
            if (!on_host[i]) jobs.push_back(full_job(ptrs[i], lens[i], (uint32_t)i));
        const bool tails = !hs.start.empty();
        if (tails) {
            host_share_jobs(hs, ptrs, jobs);
            if ((r = tail_note(n, &note, &note_dev))) return r;
            if (done.create() != hipSuccess) {
                set_error(KRK_EHIP, "sha256 tail handoff: event");
                return r = KRK_EHIP;
            }
        }
        if ((r = run_jobs(D, jobs, digests_dev, note_dev, s))) return r;
        if (tails && hipEventRecord(done, s) != hipSuccess) {
            set_error(KRK_EHIP, "sha256 tail handoff: event record");
            return r = KRK_EHIP;
        }
        return r;
    }
    int finish(Device* D, const uint8_t* const* ptrs, const uint64_t* lens, hipEvent_t ready, uint8_t* digests_dev,
               hipStream_t s, hipStream_t s_out) {
        if (!r && !hs.idx.empty()) r = offload_run(D, hs, ptrs, lens, ready, digests_dev, s_out, note, done);
        release(s);
        return r;
    }
};

int krk_sha_last_tail(uint64_t* chains, uint64_t* gpu_prefix_bytes) {
    if (chains) *chains = t_last_tail.chains;
    if (gpu_prefix_bytes) *gpu_prefix_bytes = t_last_tail.gpu_prefix_bytes;
    return KRK_OK;
}

int krk_sha256_dev(const uint8_t* const* data_dev, const uint64_t* lengths, uint64_t n, uint8_t* digests_dev,
                   void* stream) {
    KRK_DEVICE(D);
    if (!n) return KRK_OK;
    KRK_CHECK(data_dev && lengths && digests_dev, KRK_EINVAL, "sha256_dev: null argument");
    hipStream_t s = pick(D, stream);
    std::vector<char> on_host;
    const HostShare hs = offload_split(D, lengths, n, on_host);
    if (hs.idx.empty()) {
        std::vector<ShaJob> jobs;
        jobs.reserve(n);
        for (uint64_t i = 0; i < n; ++i) jobs.push_back(full_job(data_dev[i], lengths[i], (uint32_t)i));
        return run_jobs(D, jobs, digests_dev, nullptr, s);
    }
    Event ready;
    KRK_HIP(ready.create());
    KRK_CHECK(hipEventRecord(ready, s) == hipSuccess, KRK_EHIP, "sha256_dev: event record failed");
    ShaHostShare sh(hs);
    sh.launch(D, on_host, data_dev, lengths, n, digests_dev, s);  // the GPU part runs while the host hashes
    return sh.finish(D, data_dev, lengths, ready, digests_dev, s, s);
}

int krk_sha256_dev_on_host(const uint8_t* const* data_dev, const uint64_t* lengths, uint64_t n, int threads,
                           void* stream, uint8_t* digests_host) {
    KRK_DEVICE(D);
    if (!n) return KRK_OK;
    KRK_CHECK(data_dev && lengths && digests_host, KRK_EINVAL, "sha256_dev_on_host: null argument");
    hipStream_t s = pick(D, stream);
    Event ready;
    KRK_HIP(ready.create());
    KRK_CHECK(hipEventRecord(ready, s) == hipSuccess, KRK_EHIP, "sha256_dev_on_host: event record failed");
    const std::vector<const uint8_t*> p(data_dev, data_dev + n);
    const std::vector<uint64_t> l(lengths, lengths + n);
    return offload_hash(D, p, l, threads > 0 ? threads : host_threads_for_call(), ready, digests_host);
}

static thread_local int t_last_ih_place = KRK_PLACE_HOST;  // krk_metainfo_batch_last_placement

int krk_metainfo_batch_last_placement(int* placement) {
    KRK_CHECK(placement, KRK_EINVAL, "metainfo_batch_last_placement: null argument");
    *placement = t_last_ih_place;
    return KRK_OK;
}

// krk_metainfo_batch_dev with the InfoHash on the device (krk_set_info_hash_placement): the
// CRC launches on D->s_a, the InfoHash launches (info_hash.hip) on D->s_b, group g's InfoHash
// after group g's CRC by an event and beside group g+1's CRC; both forked from and joined
// back into s, where the sums and the hashes are copied back once.  No host thread is started.
// One group (KRK_INFOHASH_GROUPS): a second CRC launch's ramp and tail cost about what the
// InfoHash launch it would hide takes (C5 regen: 0.22 ms).  C5 regen 9.45 / 9.49 ms a step with
// one group, 9.45 / 9.27 with two, 9.92 / 9.85 with four; the host placement 9.21-9.45
// (profiles/r07/infohash_dev.json).
static int metainfo_batch_gpu(Device* D, const krk_blob* blobs, uint64_t n, const char* names,
                              const uint64_t* name_off, uint32_t* sums_dev, uint32_t* sums_host, uint8_t* info_hash20,
                              hipStream_t s, const int64_t* pl, const int64_t* ln, const uint64_t* so,
                              const uint64_t* ns, uint64_t total) {
    static const uint64_t kGroups = [] {
        const char* g = KRK_AB_ENV("KRK_INFOHASH_GROUPS");
        return (uint64_t)std::max(1, g ? atoi(g) : 1);
    }();
    const uint64_t G = std::min<uint64_t>(n, kGroups);
    std::vector<uint64_t> cut{0};
    for (uint64_t i = 0, acc = 0; i < n && cut.size() < G; ++i) {
        acc += blobs[i].length;
        if ((double)acc * (double)G >= (double)total * (double)cut.size() && i + 1 < n) cut.push_back(i + 1);
    }
    cut.push_back(n);
    const size_t ng = cut.size() - 1;
    uint8_t* d_ih = nullptr;
    KRK_HIP(scratch_alloc(D, &d_ih, 20 * n, s));
    Event fork, join;
    std::vector<Event> ev(ng);
    int r = KRK_OK;
    auto hip = [&r](hipError_t e, const char* what) {
        if (e != hipSuccess && !r) {
            set_error(KRK_EHIP, "metainfo_batch_dev: %s: %s", what, hipGetErrorString(e));
            r = KRK_EHIP;
        }
        return e == hipSuccess;
    };
    bool forked = hip(fork.create(), "event create") && hip(join.create(), "event create") &&
                  hip(hipEventRecord(fork, s), "event record") && hip(hipStreamWaitEvent(D->s_a, fork, 0), "fork") &&
                  hip(hipStreamWaitEvent(D->s_b, fork, 0), "fork");
    for (size_t g = 0; forked && g < ng && !r; ++g) {
        const uint64_t a = cut[g], m = cut[g + 1] - cut[g];
        if (!hip(ev[g].create(), "event create")) break;
        r = piece_sums_dev(D, blobs + a, m, sums_dev, D->s_a);
        if (r || !hip(hipEventRecord(ev[g], D->s_a), "event record") ||
            !hip(hipStreamWaitEvent(D->s_b, ev[g], 0), "event wait"))
            break;
        r = info_hash_dev(D, pl + a, sums_dev, so + a, ns + a, names, name_off + a, ln + a, m, d_ih + 20 * a, D->s_b);
    }
    if (forked) {  // s follows everything queued on the two streams, failed batch or not
        hip(hipEventRecord(join, D->s_a), "event record");
        hip(hipStreamWaitEvent(s, join, 0), "join");
        Event join_b;
        if (hip(join_b.create(), "event create") && hip(hipEventRecord(join_b, D->s_b), "event record"))
            hip(hipStreamWaitEvent(s, join_b, 0), "join");
        if (r) {  // an event was missing somewhere: wait for the streams themselves
            hipStreamSynchronize(D->s_a);
            hipStreamSynchronize(D->s_b);
        }
    }
    if (!r) {
        uint64_t lo, hi;
        sums_span(blobs, n, &lo, &hi);
        if (hi > lo) hip(hipMemcpyAsync(sums_host + lo, sums_dev + lo, (hi - lo) * 4, hipMemcpyDeviceToHost, s), "sums copy");
        hip(hipMemcpyAsync(info_hash20, d_ih, 20 * n, hipMemcpyDeviceToHost, s), "hash copy");
    }
    hip(hipStreamSynchronize(s), "sync");
    scratch_free(D, d_ih, s);
    return r;
}

int krk_metainfo_batch_dev(const krk_blob* blobs, uint64_t n_blobs, const char* names, const uint64_t* name_off,
                           uint32_t* sums_dev, uint32_t* sums_host, uint8_t* info_hash20, void* stream) {
    KRK_DEVICE(D);
    int r = validate_blobs(blobs, n_blobs);
    if (r) return r;
    if (!n_blobs) return KRK_OK;
    KRK_CHECK(sums_dev && sums_host && info_hash20 && name_off, KRK_EINVAL, "metainfo_batch_dev: null argument");
    hipStream_t s = pick(D, stream);
    // Groups of about equal bytes, run back to back on `s`; the host hashes group g
    // while the device runs groups g+1.. (one event per group).
    std::vector<int64_t> pl(n_blobs), ln(n_blobs);
    std::vector<uint64_t> so(n_blobs), ns(n_blobs);
    uint64_t total = 0;
    for (uint64_t i = 0; i < n_blobs; ++i) {
        pl[i] = blobs[i].piece_length;
        ln[i] = (int64_t)blobs[i].length;
        so[i] = blobs[i].sums_offset;
        ns[i] = krk_num_pieces(blobs[i].length, blobs[i].piece_length);
        total += blobs[i].length;
    }
    t_last_ih_place = info_hash_placement_resolved();
    if (t_last_ih_place == KRK_PLACE_GPU)
        return metainfo_batch_gpu(D, blobs, n_blobs, names, name_off, sums_dev, sums_host, info_hash20, s, pl.data(),
                                  ln.data(), so.data(), ns.data(), total);
    // Four groups (KRK_REGEN_GROUPS): C5 regen 9.84-9.90 ms a step against 10.14-10.16
    // with eight (each launch's ramp and tail cost more than the InfoHash overlap buys) and
    // 9.70-10.07 with one (profiles/r03/regen_groups_ab.txt).
    static const uint64_t kGroups = [] {
        const char* g = KRK_AB_ENV("KRK_REGEN_GROUPS");
        return (uint64_t)std::max(1, g ? atoi(g) : 4);
    }();
    const uint64_t G = std::min<uint64_t>(n_blobs, kGroups);
    // The host's InfoHash of the last group is the only host work not hidden behind a later
    // group's kernel, so that group is small: 4 % of the bytes (KRK_REGEN_TAIL; <= 0 or >= 1:
    // equal groups), the others sharing the rest equally.  C5 regen 5.10-5.24 TB/s with equal
    // groups, 5.44-5.58 with a 4 % tail, 5.35-5.41 with 2 % (profiles/r03/regen_tail_ab.txt).
    static const double kTail = [] {
        const char* t = KRK_AB_ENV("KRK_REGEN_TAIL");
        return t ? atof(t) : 0.04;
    }();
    const double tail = (kTail > 0 && kTail < 1 && G > 1) ? kTail : 1.0 / (double)G;
    std::vector<uint64_t> cut{0};
    for (uint64_t i = 0, acc = 0; i < n_blobs && cut.size() < G; ++i) {
        acc += blobs[i].length;
        const double want = G > 1 ? (1.0 - tail) * (double)cut.size() / (double)(G - 1) : 1.0;
        if ((double)acc >= (double)total * want && i + 1 < n_blobs) cut.push_back(i + 1);
    }
    cut.push_back(n_blobs);
    const size_t ng = cut.size() - 1;
    std::vector<Event> ev(ng);
    // sums copies on one of the context's other non-blocking streams (creating a stream
    // per call costs milliseconds on ROCm)
    hipStream_t cs = s == D->s_b ? D->s_a : D->s_b;
    size_t launched = 0;
    for (size_t g = 0; g < ng && !r; ++g) {
        if (ev[g].create() != hipSuccess) {
            set_error(KRK_EHIP, "metainfo_batch_dev: event create");
            r = KRK_EHIP;
            break;
        }
        r = piece_sums_dev(D, blobs + cut[g], cut[g + 1] - cut[g], sums_dev, s);
        if (!r && hipEventRecord(ev[g], s) != hipSuccess) {
            set_error(KRK_EHIP, "metainfo_batch_dev: event record");
            r = KRK_EHIP;
        }
        if (!r) ++launched;
    }
    for (size_t g = 0; g < launched; ++g) {
        if (hipEventSynchronize(ev[g]) != hipSuccess) {
            if (!r) { set_error(KRK_EHIP, "metainfo_batch_dev: kernel failed"); r = KRK_EHIP; }
            continue;
        }
        if (r) continue;  // keep draining the launched groups before returning
        uint64_t lo = UINT64_MAX, hi = 0;
        for (uint64_t i = cut[g]; i < cut[g + 1]; ++i)
            if (ns[i]) { lo = std::min(lo, so[i]); hi = std::max(hi, so[i] + ns[i]); }
        if (hi > lo) {
            if (hipMemcpyAsync(sums_host + lo, sums_dev + lo, (hi - lo) * 4, hipMemcpyDeviceToHost, cs) != hipSuccess ||
                hipStreamSynchronize(cs) != hipSuccess) {
                set_error(KRK_EHIP, "metainfo_batch_dev: sums copy");
                r = KRK_EHIP;
                continue;
            }
        }
        const uint64_t a = cut[g], m = cut[g + 1] - cut[g];
        r = krk_info_hash_batch(pl.data() + a, sums_host, so.data() + a, ns.data() + a, names, name_off + a,
                                ln.data() + a, m, info_hash20 + 20 * a);
    }
    if (hipStreamSynchronize(s) != hipSuccess && !r) { set_error(KRK_EHIP, "metainfo_batch_dev: sync"); r = KRK_EHIP; }
    return r;
}

int krk_metainfo_digest_dev(const krk_blob* blobs, uint64_t n_blobs, uint32_t* sums_dev, uint8_t* digests_dev,
                            void* stream) {
    KRK_DEVICE(D);
    int r = validate_blobs(blobs, n_blobs);
    if (r) return r;
    if (!n_blobs) return KRK_OK;
    KRK_CHECK(digests_dev, KRK_EINVAL, "digests_dev is NULL");
    hipStream_t s = pick(D, stream);
    Event fork, j1, j2;
    KRK_HIP(fork.create());
    KRK_HIP(j1.create());
    KRK_HIP(j2.create());
    KRK_HIP(hipEventRecord(fork, s));
    KRK_HIP(hipStreamWaitEvent(D->s_a, fork, 0));
    KRK_HIP(hipStreamWaitEvent(D->s_b, fork, 0));
    // The longest chains may go to host threads (krk_set_sha_host_offload), off by default.
    std::vector<uint64_t> lens(n_blobs);
    std::vector<const uint8_t*> ptrs(n_blobs);
    for (uint64_t i = 0; i < n_blobs; ++i) {
        lens[i] = blobs[i].length;
        ptrs[i] = blobs[i].data;
    }
    std::vector<char> on_host;
    const HostShare hs = offload_split(D, lens.data(), n_blobs, on_host);
    if (hs.idx.empty()) {
        // SHA first: it is the long pole; the CRC kernel fills the rest of the chip.
        std::vector<ShaJob> jobs;
        jobs.reserve(n_blobs);
        for (uint64_t i = 0; i < n_blobs; ++i) jobs.push_back(full_job(blobs[i].data, blobs[i].length, (uint32_t)i));
        r = run_jobs(D, jobs, digests_dev, nullptr, D->s_a);
        if (!r) r = piece_sums_dev(D, blobs, n_blobs, sums_dev, D->s_b);
        hipEventRecord(j1, D->s_a);
        hipEventRecord(j2, D->s_b);
        hipStreamWaitEvent(s, j1, 0);
        hipStreamWaitEvent(s, j2, 0);
    } else {
        // SHA first here too (the long pole), then the CRC, then the host share, which
        // returns once the host is done
        ShaHostShare sh(hs);
        r = sh.launch(D, on_host, ptrs.data(), lens.data(), n_blobs, digests_dev, D->s_a);
        if (!r) r = piece_sums_dev(D, blobs, n_blobs, sums_dev, D->s_b);
        hipEventRecord(j2, D->s_b);
        hipStreamWaitEvent(s, j2, 0);
        const int rf = sh.finish(D, ptrs.data(), lens.data(), fork, digests_dev, D->s_a, s);
        if (!r) r = rf;
        hipEventRecord(j1, D->s_a);
        hipStreamWaitEvent(s, j1, 0);
    }
    return r;
}

// crc_only: chunks of one blob may repeat (their CRCs XOR into the sums independently); a
// SHA-256 step takes at most one chunk a blob slot (one midstate each).
static int validate_chunks(const krk_chunk* c, uint64_t n, bool crc_only = false) {
    KRK_CHECK(n == 0 || c, KRK_EINVAL, "chunks is NULL");
    std::unordered_map<uint64_t, uint64_t> seen;
    seen.reserve(n);
    for (uint64_t i = 0; i < n; ++i) {
        KRK_CHECK(crc_only || seen.emplace(c[i].blob, i).second, KRK_EINVAL, "blob slot %llu appears twice in one call",
                  (unsigned long long)c[i].blob);
        KRK_CHECK(c[i].piece_length > 0, KRK_EINVAL, "piece length must be positive");
        KRK_CHECK(c[i].length == 0 || c[i].data, KRK_EINVAL, "chunk %llu: data is NULL", (unsigned long long)i);
        KRK_CHECK(c[i].offset + c[i].length <= c[i].blob_length, KRK_ERANGE, "chunk %llu runs past its blob",
                  (unsigned long long)i);
        KRK_CHECK(c[i].offset % 64 == 0, KRK_EINVAL, "chunk %llu: offset is not a multiple of 64",
                  (unsigned long long)i);
        KRK_CHECK(c[i].length % 64 == 0 || c[i].offset + c[i].length == c[i].blob_length, KRK_EINVAL,
                  "chunk %llu: only a blob's last chunk may be a partial block", (unsigned long long)i);
        KRK_CHECK(c[i].blob <= 0xFFFFFFFFull, KRK_EINVAL, "blob slot exceeds 2^32");
        KRK_CHECK(c[i].sums_offset + krk_num_pieces(c[i].blob_length, c[i].piece_length) <= 0xFFFFFFFFull,
                  KRK_EINVAL, "sums index exceeds 2^32 in one call");
    }
    return KRK_OK;
}

// One window step over device chunks: SHA jobs on D->s_a, CRC items on D->s_b, both
// forked from and joined back into s.  With the caller's SHA stream `ks`, the CRC items run
// on s itself: a caller that keeps its window streams at high priority (the C3 tail
// handoff, kraken_amd/windowed.py) then leaves no fork / join barrier of a window on the
// library's normal-priority streams, whose hardware queues its copy threads share -- a
// barrier waiting for a window's ~70 ms SHA launch blocks every packet behind it there.
//
// crc_after_sha (with ks): the CRC items are queued on s only once the SHA-256 launch has
// ended.  A launch on a high-priority queue whose workgroups wait for CUs (the CRC's 144 KiB
// of LDS, with a window's SHA workgroups holding every CU) keeps the dispatcher from the
// normal-priority queues meanwhile: device-to-host copies of other streams stall for the
// whole window (tools/tail_probe.py, profiles/r06/tail_probe.jsonl: 36 -> 0.18 GB/s).
static int chunks_step(Device* D, const krk_chunk* c, uint64_t n, uint32_t* state_dev, uint32_t* sums_dev,
                       uint8_t* digests_dev, hipStream_t s, ItemBuilder& B, hipStream_t ks = nullptr,
                       bool crc_after_sha = false) {
    const hipStream_t kc = ks ? s : D->s_b;
    if (!ks) ks = D->s_a;
    std::vector<ShaJob> jobs(n);
    CrcBatch items;
    for (uint64_t i = 0; i < n; ++i) {
        jobs[i] = chunk_job(c[i].data, c[i].offset, c[i].length, c[i].blob_length, (uint32_t)c[i].blob);
        if (c[i].length)
            B.add(items, jobs[i].ptr, c[i].offset, c[i].offset + c[i].length, c[i].blob_length,
                  (uint64_t)c[i].piece_length, c[i].sums_offset);
    }
    Event fork, j1, j2;
    KRK_HIP(fork.create());
    KRK_HIP(j1.create());
    KRK_HIP(j2.create());
    KRK_HIP(hipEventRecord(fork, s));
    KRK_HIP(hipStreamWaitEvent(ks, fork, 0));
    if (kc != s) KRK_HIP(hipStreamWaitEvent(kc, fork, 0));
    int r = run_jobs(D, jobs, digests_dev, state_dev, ks);
    hipEventRecord(j1, ks);
    if (crc_after_sha && kc == s) {
        hipStreamWaitEvent(s, j1, 0);
        if (!r) r = run_items(D, items, sums_dev, kc);
    } else {
        if (!r) r = run_items(D, items, sums_dev, kc);
        hipStreamWaitEvent(s, j1, 0);
        if (kc != s) {
            hipEventRecord(j2, kc);
            hipStreamWaitEvent(s, j2, 0);
        }
    }
    return r;
}

// The chunk entry points: one window step on `stream`; with sha_stream the SHA-256 launch
// goes there and the CRC items on `stream` itself, `after`: only once that launch has ended.
static int chunks_call(const krk_chunk* chunks, uint64_t n, uint32_t* state_dev, uint32_t* sums_dev,
                       uint8_t* digests_dev, void* stream, void* sha_stream, bool after) {
    KRK_DEVICE(D);
    int r = validate_chunks(chunks, n);
    if (r || !n) return r;
    if (after)
        KRK_CHECK(state_dev && sums_dev && digests_dev && sha_stream, KRK_EINVAL, "chunks_dev_after: null argument");
    KRK_CHECK(state_dev && sums_dev && digests_dev, KRK_EINVAL, "chunks_dev: null output");
    ItemBuilder B;
    return chunks_step(D, chunks, n, state_dev, sums_dev, digests_dev, pick(D, stream), B,
                       static_cast<hipStream_t>(sha_stream), after);
}

int krk_metainfo_digest_chunks_dev(const krk_chunk* chunks, uint64_t n, uint32_t* state_dev, uint32_t* sums_dev,
                                   uint8_t* digests_dev, void* stream) {
    return chunks_call(chunks, n, state_dev, sums_dev, digests_dev, stream, nullptr, false);
}

int krk_metainfo_digest_chunks_dev_on(const krk_chunk* chunks, uint64_t n, uint32_t* state_dev, uint32_t* sums_dev,
                                      uint8_t* digests_dev, void* stream, void* sha_stream) {
    return chunks_call(chunks, n, state_dev, sums_dev, digests_dev, stream, sha_stream, false);
}

int krk_metainfo_digest_chunks_dev_after(const krk_chunk* chunks, uint64_t n, uint32_t* state_dev, uint32_t* sums_dev,
                                         uint8_t* digests_dev, void* stream, void* sha_stream) {
    return chunks_call(chunks, n, state_dev, sums_dev, digests_dev, stream, sha_stream, true);
}

// The piece CRCs of device chunks alone (no SHA-256): the tail bytes of chains whose
// SHA-256 a host thread finishes (the windowed tail handoff, kraken_amd/windowed.py) still
// get their piece sums on the GPU, XOR-accumulated like a window's.
int krk_chunks_crc_dev(const krk_chunk* chunks, uint64_t n, uint32_t* sums_dev, void* stream) {
    KRK_DEVICE(D);
    int r = validate_chunks(chunks, n, /*crc_only=*/true);
    if (r || !n) return r;
    KRK_CHECK(sums_dev, KRK_EINVAL, "chunks_crc_dev: sums_dev is NULL");
    ItemBuilder B;
    CrcBatch items;
    for (uint64_t i = 0; i < n; ++i)
        if (chunks[i].length)
            B.add(items, reinterpret_cast<uint64_t>(chunks[i].data), chunks[i].offset,
                  chunks[i].offset + chunks[i].length, chunks[i].blob_length, (uint64_t)chunks[i].piece_length,
                  chunks[i].sums_offset);
    return run_items(D, items, sums_dev, pick(D, stream));
}

int krk_verify_pieces_dev(const krk_blob* blob, const uint32_t* expected_host, uint8_t* ok_out_host, void* stream) {
    KRK_CHECK(blob && expected_host && ok_out_host, KRK_EINVAL, "verify: null argument");
    KRK_DEVICE(D);
    hipStream_t s = pick(D, stream);
    krk_blob b = *blob;
    b.sums_offset = 0;
    const uint64_t np = krk_num_pieces(b.length, b.piece_length);
    int r = validate_blobs(&b, 1);
    if (r || !np) return r;
    uint32_t* d_sums = nullptr;
    uint8_t* d_ok = nullptr;
    KRK_HIP(scratch_alloc(D, reinterpret_cast<void**>(&d_sums), np * 4, s));
    KRK_HIP(scratch_alloc(D, reinterpret_cast<void**>(&d_ok), np, s));
    r = piece_sums_dev(D, &b, 1, d_sums, s);
    void* d_exp = nullptr;
    if (!r) r = upload(D, expected_host, np * 4, &d_exp, s);
    if (!r) {
        hipError_t e = launch_crc_verify(d_sums, static_cast<const uint32_t*>(d_exp), d_ok, (uint32_t)np, s);
        if (e != hipSuccess) { set_error(KRK_EHIP, "verify launch: %s", launch_error_text(e)); r = KRK_EHIP; }
    }
    if (hipStreamSynchronize(s) != hipSuccess && !r) { set_error(KRK_EHIP, "verify sync"); r = KRK_EHIP; }
    if (!r && hipMemcpy(ok_out_host, d_ok, np, hipMemcpyDeviceToHost) != hipSuccess) r = KRK_EHIP;
    scratch_free(D, d_sums, s);
    scratch_free(D, d_ok, s);
    if (d_exp) scratch_free(D, d_exp, s);
    if (hipStreamSynchronize(s) != hipSuccess && !r) { set_error(KRK_EHIP, "verify sync"); r = KRK_EHIP; }
    return r;
}

}  // extern "C"
