// direct_read.hpp -- internal to libkraken_hip, no HIP: the O_DIRECT read of a block-aligned
// request into a pinned staging window (direct_pread), the process-wide switch to reads through
// a bounce buffer where the windows refuse the disk's DMA, the counters that say which way a
// file batch's bytes came, and the diag build's simulated refusal.  staging.hpp's readers
// (par_read, AioReader) are built on it; tests/native/direct_read_main.cpp drives it alone.
#pragma once
#include <errno.h>
#include <stdint.h>
#include <string.h>
#include <sys/types.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>

#include "knobs.hpp"

namespace krk {

// Which way the bytes of one file batch came (FileSource; krk_windows_last_reads).  Bytes are
// those delivered toward a task's length, not the block-rounded requests, so a batch that
// succeeds has window + bounce + cached == the sum of its files' lengths.  Relaxed atomics:
// the pool's threads count concurrently and the call reads them once they have joined.
struct ReadCounts {
    std::atomic<uint64_t> direct_files{0};    // files opened O_DIRECT
    std::atomic<uint64_t> buffered_files{0};  // O_DIRECT wanted and refused at open: buffered instead
    std::atomic<uint64_t> window_bytes{0};    // read O_DIRECT straight into a window
    std::atomic<uint64_t> bounce_bytes{0};    // read O_DIRECT into the bounce buffer and copied
    std::atomic<uint64_t> bounce_preads{0};   // preads the bounce loop made
    std::atomic<uint64_t> cached_bytes{0};    // read through the page cache
    std::atomic<uint64_t> aio_reaped{0};      // AIO requests reaped
    std::atomic<uint64_t> aio_rereads{0};     // tasks the AIO reader read synchronously (not submitted, short, refused)
    void add(std::atomic<uint64_t> ReadCounts::*m, uint64_t v) { (this->*m).fetch_add(v, std::memory_order_relaxed); }
};
constexpr int kReadCountWords = 9;  // the eight above and the bounce switch, in that order

// O_DIRECT reads land in the pinned windows by the disk's DMA only where the kernel can pin
// the windows' pages itself.  Where the runtime backs page-locked memory with device-mapped
// pages (a GPU passed through to a virtual machine), the read is refused with EFAULT before
// a byte moves: from the first such refusal on, the process reads O_DIRECT into an ordinary
// page-aligned buffer of the reading thread and copies into the window -- still no page
// cache, one host copy more.
inline std::atomic<bool>& direct_reads_bounce() {
    static std::atomic<bool> on{false};
    return on;
}

// KRK_DIRECT_REFUSE=N (diag build): from the N-th O_DIRECT read aimed at a window in this
// process -- synchronous reads and AIO completions alike -- every such read is taken as
// refused (EFAULT, no byte moved), as on a machine whose windows take no disk DMA.  The
// production build refuses nothing and does not hold the name.
inline bool direct_refuse_now() {
#ifdef KRK_DIAG
    static const long n = [] {
        const char* v = KRK_AB_ENV("KRK_DIRECT_REFUSE");
        return v ? atol(v) : 0L;
    }();
    if (n < 1) return false;
    static std::atomic<long> aimed{0};
    return aimed.fetch_add(1, std::memory_order_relaxed) + 1 >= n;
#else
    return false;
#endif
}
constexpr uint8_t kRefusedFiller = 0xA5;  // what a simulated refusal of an AIO read leaves in its range

constexpr size_t kBounce = size_t(1) << 20;

// pread of a block-aligned request on an O_DIRECT descriptor into a pinned window.  Of the
// bytes read, at most `useful` (the part of `want` that is not block padding) are counted.
inline ssize_t direct_pread(int fd, uint8_t* dst, size_t want, off_t off, ReadCounts* rc = nullptr,
                            size_t useful = ~size_t(0)) {
    if (!direct_reads_bounce().load(std::memory_order_relaxed)) {
        ssize_t got = -1;
        if (direct_refuse_now()) errno = EFAULT;
        else got = pread(fd, dst, want, off);
        if (!(got < 0 && errno == EFAULT)) {
            if (rc && got > 0) rc->add(&ReadCounts::window_bytes, std::min((size_t)got, useful));
            return got;
        }
        direct_reads_bounce().store(true, std::memory_order_relaxed);
    }
    struct Bounce {
        void* p = nullptr;
        ~Bounce() { free(p); }
    };
    static thread_local Bounce bounce;
    if (!bounce.p && posix_memalign(&bounce.p, 4096, kBounce) != 0) {
        bounce.p = nullptr;
        errno = ENOMEM;
        return -1;
    }
    size_t done = 0;
    while (done < want) {
        const size_t ask = std::min(kBounce, want - done);
        const ssize_t got = pread(fd, bounce.p, ask, off + (off_t)done);
        if (rc) rc->add(&ReadCounts::bounce_preads, 1);
        if (got < 0 && errno == EINTR) continue;
        if (got < 0 && !done) return -1;
        if (got <= 0) break;  // what is in so far; the caller's next read meets the error or EOF
        memcpy(dst + done, bounce.p, (size_t)got);
        done += (size_t)got;
        if ((size_t)got < ask) break;
    }
    if (rc) rc->add(&ReadCounts::bounce_bytes, std::min(done, useful));
    return (ssize_t)done;
}

}  // namespace krk
