// window_math.hpp -- the arithmetic of the host-resident window passes, free of any runtime:
// the two schedules (which bytes of which blob a window carries: WindowSched for the digest
// calls, PackSched for the CRC-only ones; run by window_pass.cpp) and the cut of a window's
// fill into per-thread spans (par_copy / par_read, staging.hpp).  Included by the library and
// by tests/native/window_math_main.cpp, which checks all three against a byte walk.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace krk {

// ----------------------------------------------------------------- the window schedule
struct WinChunk {
    uint32_t blob;
    uint64_t off, len;
};

class WindowSched {
  public:
    // blobs: the windowed blobs' indices into lens; chunks a multiple of `align` bytes
    // (64: SHA-256 blocks; 4 KiB for O_DIRECT file reads) except each blob's last.
    WindowSched(const uint64_t* lens, std::vector<uint32_t> blobs, uint64_t W, uint64_t cap, uint64_t align = 64)
        : L_(lens), W_(W), cap_(std::max<uint64_t>(cap, 1)), align_(std::max<uint64_t>(align, 64)), queue_(std::move(blobs)) {
        std::stable_sort(queue_.begin(), queue_.end(), [&](uint32_t a, uint32_t b) { return L_[a] > L_[b]; });
    }
    // The next window's chunks (in admission order); false once every blob is done.
    bool next(std::vector<WinChunk>& out) {
        out.clear();
        while (live_.size() < cap_ && q_ < queue_.size()) live_.push_back({queue_[q_++], 0});
        if (live_.empty()) return false;
        max_live_ = std::max<uint64_t>(max_live_, live_.size());
        const uint64_t c = std::max(align_, std::min(max_chunk_, W_ / live_.size()) / align_ * align_);
        size_t keep = 0;
        for (size_t k = 0; k < live_.size(); ++k) {
            auto [b, pos] = live_[k];
            const uint64_t take = std::min(c, L_[b] - pos);
            out.push_back({b, pos, take});
            pos += take;
            if (pos < L_[b]) live_[keep++] = {b, pos};
        }
        live_.resize(keep);
        return true;
    }
    uint64_t max_live() const { return max_live_; }
    // At most `c` bytes a chunk (rounded down to the alignment): the windows stay short once
    // few blobs are live (the tail handoff hands chains over at window boundaries).
    void set_max_chunk(uint64_t c) { max_chunk_ = std::max<uint64_t>(c, 1); }
    // Take blob b out of the schedule (its chain continues elsewhere): a live blob's slot goes
    // to the next waiting blob at the next window; a waiting one is never admitted.  *done:
    // the bytes the windows gave it (0 for a waiting blob).
    bool drop(uint32_t b, uint64_t* done) {
        for (size_t k = 0; k < live_.size(); ++k)
            if (live_[k].first == b) {
                *done = live_[k].second;
                live_.erase(live_.begin() + (long)k);
                return true;
            }
        for (size_t k = q_; k < queue_.size(); ++k)
            if (queue_[k] == b) {
                *done = 0;
                queue_.erase(queue_.begin() + (long)k);
                return true;
            }
        return false;
    }

  private:
    const uint64_t* L_;
    uint64_t W_, cap_, align_;
    std::vector<uint32_t> queue_;
    size_t q_ = 0;
    std::vector<std::pair<uint32_t, uint64_t>> live_;  // blob, bytes done
    uint64_t max_live_ = 0;
    uint64_t max_chunk_ = UINT64_MAX;
};

// The packing schedule of the CRC-only passes: blobs in index order, a portion of
// min(rest of the blob, W - fill), `fill` rounded up to `place` after every portion; a window
// ends at fill >= W or with the last blob, and a zero-length blob yields no chunk.
// Precondition: W % place == 0 (W - fill wraps otherwise).
class PackSched {
  public:
    PackSched(const uint64_t* lens, uint64_t n, uint64_t W, uint64_t place) : L_(lens), n_(n), W_(W), place_(place) {}
    // The next window's chunks; false once every byte has been handed out.
    bool next(std::vector<WinChunk>& out) {
        out.clear();
        for (uint64_t fill = 0; b_ < n_ && fill < W_;) {
            const uint64_t take = std::min(L_[b_] - off_, W_ - fill);
            if (take) out.push_back({(uint32_t)b_, off_, take});
            off_ += take;
            fill = (fill + take + place_ - 1) / place_ * place_;
            if (off_ >= L_[b_]) ++b_, off_ = 0;
        }
        return !out.empty();
    }

  private:
    const uint64_t* L_;
    uint64_t n_, W_, place_, b_ = 0, off_ = 0;
};

// Both schedules place a window's chunks by one rule, which the pass applies (window_pass.cpp):
// chunk k + 1 starts at pos_k + round_up(len_k, place).

// ------------------------------------------------------------- a window's fill, cut in spans
// A window's fill tasks laid end to end form one byte stream, cut into spans that threads
// take one each.  With `padded` every task occupies its length rounded up to 4 KiB in the
// stream (O_DIRECT reads: a span boundary on a 4 KiB multiple of the stream is then one of
// its task too); the padding itself carries no bytes.

// Fills below this many bytes run on the calling thread alone.
constexpr size_t kSplitMinBytes = size_t(8) << 20;

inline size_t span_padded(size_t n, bool padded) { return padded ? (n + 4095) & ~size_t(4095) : n; }

// The span length of a stream of `total` bytes over T threads: equal shares for memory copies,
// shares rounded up to 1 MiB (at least 1 MiB) for file reads.
inline size_t copy_span_bytes(size_t total, unsigned T) { return (total + T - 1) / T; }
inline size_t read_span_bytes(size_t total, unsigned T) {
    constexpr size_t kAlign = size_t(1) << 20;
    return std::max(kAlign, ((total + T - 1) / T + kAlign - 1) & ~(kAlign - 1));
}

// The pieces of span [lo, hi) of the stream: emit(task, a, b) for bytes [a, b) of task `task`,
// in task order; len(i) is task i's length, i < count.
template <class Len, class Emit>
inline void cut_span(size_t count, Len&& len, size_t lo, size_t hi, bool padded, Emit&& emit) {
    size_t pos = 0;
    for (size_t i = 0; i < count && pos < hi; ++i) {
        const size_t n = len(i);
        const size_t a = std::max(lo, pos), b = std::min(hi, pos + n);
        if (a < b) emit(i, a - pos, b - pos);
        pos += span_padded(n, padded);
    }
}

}  // namespace krk
