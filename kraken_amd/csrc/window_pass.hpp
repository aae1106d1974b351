// window_pass.hpp -- internal to libkraken_hip: the one pass that moves host-resident bytes
// (caller buffers, cache files) window by window through the pinned staging ring to the
// SHA-256 and CRC kernels, its two sources and the descriptor budget of the
// file batches.  The entry points are in windows.cpp (the digest calls, WindowSched) and
// crc_host.cpp (the CRC-only calls, PackSched).
#pragma once
#include "host_register.hpp"
#include "staging.hpp"

namespace krk {

// Bytes [off, off + len) of blob b into dst (host, pinned).  A blob of no bytes has a task too
// where the schedule gives it a chunk (WindowSched): its file is opened.
struct FillTask {
    uint32_t b;
    uint64_t off, len;
    uint8_t* dst;
};

// The caller's buffers.  Page-locked ones (krk_host_alloc) go up straight from the caller's
// pages, pageable ones through the pinned host window or, registered for the call
// (host_register.hpp), by the gather.
struct MemSource {
    static constexpr bool kMemory = true;
    const krk_blob* blobs;
    uint64_t n;
    bool pinned = false;  // every windowed blob page-locked: no staging copy
    bool mapped = false;  // ... at device addresses equal to the host ones (the gather reads them there)
    std::unique_ptr<HostRegistry> reg;    // pageable blobs registered for the gather
    hipStream_t gather_stream = nullptr;  // where the gathers run (drained before unregistering)
    MemSource(const krk_blob* b, uint64_t n_) : blobs(b), n(n_) {}
    ~MemSource() {
        if (reg) reg->finish(gather_stream);
    }
    // Every blob of bytes not in `skip` (empty: none skipped) is page-locked.
    bool all_pinned(const std::vector<char>& skip) const;
    // pinned_: what all_pinned said and the caller allows.  gather_mode (KRK_HOST_GATHER): 0 never
    // gather, 1 register pageable blobs for it, -1 gather page-locked blobs only.  cp: the
    // pass's copy stream.
    void setup(const std::vector<char>& skip, bool pinned_, int gather_mode, hipStream_t cp);
    // Tell the registry which pages each window reads (a dry run of the pass's schedule) and
    // start its helpers.
    template <class Sched>
    void announce(Sched dry) {
        std::vector<WinChunk> win;
        for (int w = 0; dry.next(win); ++w)
            for (const WinChunk& c : win) reg->need(w, at(c.blob, c.off), c.len);
        reg->start(std::min(4, std::max(1, host_threads_for_call() / 4)));
    }
    const uint8_t* at(uint32_t b, uint64_t off) const { return blobs[b].data + off; }
    // Window wi may be gathered: every blob mapped, or its pages registered by now (a
    // registration that failed stages this window and every later one).
    bool gather_ready(int wi) { return reg ? (reg_ok_ = reg_ok_ && reg->ready(wi)) : mapped; }
    int fill(const std::vector<FillTask>& tasks);  // par_copy

  private:
    bool reg_ok_ = true;
};

// The cache files.  A blob's file is opened at its first chunk (O_DIRECT if wanted and the
// file system has it) and closed after its last; live blobs <= the descriptor budget, so no
// descriptor is reopened.
struct FileSource {
    static constexpr bool kMemory = false;
    // async: O_DIRECT chunks by Linux AIO and page-cache reads with readahead marks (the
    // digest pass); else every read by par_read alone (the CRC-only pass).
    FileSource(const krk_file_blob* f, uint64_t n, bool want_direct, bool async);
    ~FileSource();
    int fill(const std::vector<FillTask>& tasks);

  private:
    int open_file(uint32_t i);
    const krk_file_blob* files_;
    bool direct_, async_;
    std::vector<int> fd_;
    std::vector<char> is_direct_;
    std::unique_ptr<std::atomic<uint64_t>[]> ra_;  // each file's readahead mark (par_read)
    AioReader aio_;                                  // the O_DIRECT chunks of a window
};

// File descriptors the file batches may hold open, shared by the whole process: a lease of
// the budget (window_pass.cpp FdPool).  A call waits only while every descriptor is leased,
// and then takes at least one.
struct FdLease {
    uint64_t n;
    explicit FdLease(uint64_t want);
    ~FdLease();
    FdLease(const FdLease&) = delete;
    FdLease& operator=(const FdLease&) = delete;
};

// What a digest call's pass did (krk_windows_last_*).
struct PassStats {
    uint64_t max_live = 0;
    int windows = 0;
    int direct_windows = 0;  // windows DMA'd straight from the caller's page-locked memory
    int gather_windows = 0;  // windows gathered by the GPU from page-locked / registered caller memory
    uint64_t host_blobs = 0;
    uint64_t registered_bytes = 0;  // caller bytes registered for the gather
    double register_s = 0;          // helper-thread seconds spent registering them
    // the window loop's wall seconds and where it waited: for a free window (acquire), filling
    // windows from the source (fill: staging copies or file reads), enqueueing copies + kernels
    double loop_s = 0, acquire_s = 0, fill_s = 0, enqueue_s = 0;
    double resident = -1;  // file batches: the page-cache resident share of the sampled files
    bool direct_reads = false;  // file batches: read with O_DIRECT
    uint64_t live_at_copyout = 0;  // registry segments still registered when the results were copied out
};

// One pass.  Asynchronous on its streams: run_windows returns once the last window is queued
// and the caller synchronises cp / ks / kc.
struct WindowPass {
    const char* what;  // in the error texts
    Device* D;
    std::function<bool(std::vector<WinChunk>&)> next;  // the schedule: the next window's chunks
    size_t place;  // chunk k + 1 starts at pos_k + round_up(len_k, place) in its window
    size_t lease;  // staging bytes a window (no window the schedule builds places more)
    // copies on cp; SHA-256 on ks and CRC on kc, each skipped when its stream is null
    hipStream_t cp, ks, kc;
    const uint64_t* lens;  // per blob, indexed like the chunks' blobs
    const int64_t* plens;
    const uint64_t* soff;
    uint8_t* d_dig;  // device outputs, indexed like the blobs (sums by soff)
    uint32_t *d_state, *d_sums;
    size_t build_ahead;  // windows a helper thread builds ahead of the loop (0: built in the loop)
    PassStats* st;       // or null
};
template <class Source>
int run_windows(const WindowPass& p, Source& src);
extern template int run_windows<MemSource>(const WindowPass&, MemSource&);
extern template int run_windows<FileSource>(const WindowPass&, FileSource&);

}  // namespace krk
