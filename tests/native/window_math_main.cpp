// The arithmetic of the host-resident window passes (kraken_amd/csrc/window_math.hpp) as a stand-alone program:
//  1. WindowSched against a byte walk.  Lists of n <= 4 blobs; W in {align, 3 align, 8 align + 1}; cap 1-5; align
//     64 and 4096; with and without set_max_chunk; and a drop of a live and of a waiting blob after the first
//     window.  Lengths: every length 0 ... 3 align + 1 for n <= 2 at align 64 (37,636 pairs, without the drops),
//     and the ten lengths of that range at which the schedule can change course {0, 1, align - 1, align,
//     align + 1, 2 align - 1, 2 align, 2 align + 1, 3 align, 3 align + 1} for n <= 4 at both alignments (seven of
//     them for the fourth blob; the whole range to the fourth power is 1.4e9 lists at align 64, and the program
//     runs under two sanitizers).  Required of every schedule: each blob's bytes are covered exactly once
//     and in order, every non-final chunk is min(c, rest) for the window's c (a positive multiple of align), a
//     blob has one chunk a window, blobs are admitted longest first in stable order, live <= cap, max_live is the
//     widest window, a dropped blob reports the bytes it was given and never returns.
//  2. cut_span with copy_span_bytes / read_span_bytes (what par_copy and par_read run) over T = 1 ... 17: the
//     pieces cover each task's bytes exactly once and in order; padded, every piece starts on a 4 KiB multiple of
//     its task and ends on one or at the task's end.
//  3. PackSched against a byte walk.  Lists of n <= 4 blobs; place 16 and 4096; W in {place, 3 place, 8 place};
//     lengths from the nine values at which the packing can change course {0, 1, place - 1, place, place + 1,
//     W - 1, W, W + 1, 2 W + 1} (2 x 3 x (1 + 9 + 81 + 729 + 6,561) = 44,286 lists).  Required of every schedule:
//     each blob's bytes are covered exactly once and in order with blobs in index order, no chunk is empty, every
//     chunk starts on a multiple of place in its window (placed as the pass places them: chunk k + 1 at
//     pos_k + round_up(len_k, place)) and ends at or before W, every window but the last is full (its rounded
//     fill equals W), and the schedule ends.
#include <stdio.h>

#include "../../kraken_amd/csrc/window_math.hpp"

using namespace krk;

static long g_cases = 0, g_bad = 0, g_windows = 0, g_drops = 0, g_pieces = 0;
#define CHECK(cond, ...)                        \
    do {                                        \
        if (!(cond)) {                          \
            if (g_bad++ < 20) {                 \
                printf("MISMATCH %s: ", #cond); \
                printf(__VA_ARGS__);            \
                printf("\n");                   \
            }                                   \
        }                                       \
    } while (0)

// drop: 0 none, 1 a live blob, 2 a waiting blob (after the first window, when there is one)
static void walk(const std::vector<uint64_t>& L, uint64_t W, uint64_t cap, uint64_t align, uint64_t max_chunk, int drop) {
    const size_t n = L.size();
    std::vector<uint32_t> all(n);
    for (size_t i = 0; i < n; ++i) all[i] = (uint32_t)i;
    WindowSched s(L.data(), all, W, cap, align);
    if (max_chunk) s.set_max_chunk(max_chunk);
    // the admission order: longest first, equal lengths in index order
    std::vector<uint32_t> order;
    for (size_t k = 0; k < n; ++k) {
        size_t best = n;
        for (size_t i = 0; i < n; ++i) {
            bool used = false;
            for (uint32_t o : order) used |= o == i;
            if (!used && (best == n || L[i] > L[best])) best = i;
        }
        order.push_back((uint32_t)best);
    }
    std::vector<uint64_t> pos(n, 0);
    std::vector<char> seen(n, 0), gone(n, 0);
    size_t admitted = 0;
    uint64_t widest = 0;
    std::vector<WinChunk> win;
    ++g_cases;
    for (int wi = 0; s.next(win); ++wi) {
        ++g_windows;
        CHECK(wi < 100000, "schedule does not end");
        if (wi >= 100000) return;
        CHECK(!win.empty() && win.size() <= cap, "window %d has %zu chunks, cap %llu", wi, win.size(), (unsigned long long)cap);
        widest = std::max<uint64_t>(widest, win.size());
        const uint64_t mc = max_chunk ? max_chunk : UINT64_MAX;
        const uint64_t c = std::max(align, std::min(mc, W / win.size()) / align * align);
        CHECK(c && c % align == 0, "c %llu", (unsigned long long)c);
        std::vector<char> in_window(n, 0);
        for (const WinChunk& ch : win) {
            CHECK(ch.blob < n && !gone[ch.blob] && !in_window[ch.blob], "window %d: blob %u twice or after its drop", wi, ch.blob);
            if (ch.blob >= n) return;
            in_window[ch.blob] = 1;
            if (!seen[ch.blob]) {  // admitted now: the next of the order that was not dropped while waiting
                while (admitted < n && gone[order[admitted]]) ++admitted;
                CHECK(admitted < n && order[admitted] == ch.blob, "window %d: blob %u admitted out of order", wi, ch.blob);
                ++admitted;
                seen[ch.blob] = 1;
                CHECK(ch.off == 0, "first chunk of blob %u at %llu", ch.blob, (unsigned long long)ch.off);
            } else {
                CHECK(pos[ch.blob] < L[ch.blob], "blob %u goes on after its end", ch.blob);
            }
            CHECK(ch.off == pos[ch.blob], "blob %u: chunk at %llu, %llu covered", ch.blob, (unsigned long long)ch.off,
                  (unsigned long long)pos[ch.blob]);
            CHECK(ch.len == std::min(c, L[ch.blob] - ch.off), "blob %u: chunk of %llu, c %llu, rest %llu", ch.blob,
                  (unsigned long long)ch.len, (unsigned long long)c, (unsigned long long)(L[ch.blob] - ch.off));
            if (ch.off + ch.len < L[ch.blob]) CHECK(ch.len && ch.len % align == 0, "non-final chunk of %llu", (unsigned long long)ch.len);
            pos[ch.blob] = ch.off + ch.len;
        }
        if (wi == 0 && drop) {
            uint32_t victim = UINT32_MAX;
            for (size_t k = 0; k < n && victim == UINT32_MAX; ++k) {
                const uint32_t b = order[k];
                if (drop == 1 ? (seen[b] && pos[b] < L[b]) : !seen[b]) victim = b;
            }
            if (drop == 2)  // the last waiting blob, not the next to be admitted
                for (size_t k = 0; k < n; ++k)
                    if (!seen[order[k]]) victim = order[k];
            if (victim != UINT32_MAX) {
                uint64_t done = ~0ull;
                CHECK(s.drop(victim, &done), "drop of blob %u refused", victim);
                CHECK(done == pos[victim], "drop of blob %u: %llu done, %llu given", victim, (unsigned long long)done,
                      (unsigned long long)pos[victim]);
                uint64_t again = 0;
                CHECK(!s.drop(victim, &again), "blob %u dropped twice", victim);
                gone[victim] = 1;
                ++g_drops;
            }
        }
    }
    for (size_t i = 0; i < n; ++i)
        if (!gone[i]) CHECK(seen[i] && pos[i] == L[i], "blob %zu: %llu of %llu bytes", i, (unsigned long long)pos[i], (unsigned long long)L[i]);
    CHECK(s.max_live() == widest, "max_live %llu, widest window %llu", (unsigned long long)s.max_live(), (unsigned long long)widest);
}

static void all_settings(const std::vector<uint64_t>& L, uint64_t align, bool drops = true) {
    const uint64_t Ws[3] = {align, 3 * align, 8 * align + 1};
    for (uint64_t W : Ws)
        for (uint64_t cap = 1; cap <= 5; ++cap)
            for (uint64_t mc : {uint64_t(0), 2 * align + 1})
                for (int drop = 0; drop < 3; ++drop) {
                    if (drop && (L.size() < 2 || !drops)) continue;
                    walk(L, W, cap, align, mc, drop);
                }
}

static void schedules() {
    for (uint64_t align : {uint64_t(64), uint64_t(4096)}) {
        const uint64_t edge[10] = {0, 1, align - 1, align, align + 1, 2 * align - 1, 2 * align, 2 * align + 1, 3 * align, 3 * align + 1};
        const uint64_t edge4[7] = {0, 1, align - 1, align, align + 1, 2 * align + 1, 3 * align + 1};  // the fourth blob
        all_settings({}, align);
        for (uint64_t a : edge) {
            all_settings({a}, align);
            for (uint64_t b : edge) {
                all_settings({a, b}, align);
                for (uint64_t c : edge) {
                    all_settings({a, b, c}, align);
                    for (uint64_t d : edge4) all_settings({a, b, c, d}, align);
                }
            }
        }
    }
    for (uint64_t a = 0; a <= 3 * 64 + 1; ++a) {  // every length of the range, n <= 2, align 64
        all_settings({a}, 64);
        for (uint64_t b = 0; b <= 3 * 64 + 1; ++b) all_settings({a, b}, 64, /*drops=*/false);
    }
}

// ---------------------------------------------------------------- the span cutting
static void cut(const std::vector<size_t>& tasks, unsigned T, bool padded, bool read) {
    size_t total = 0;
    for (size_t n : tasks) total += span_padded(n, padded);
    if (!total) return;
    ++g_cases;
    const size_t span = read ? read_span_bytes(total, T) : copy_span_bytes(total, T);
    CHECK(span > 0, "span of %zu bytes over %u threads", total, T);
    if (!span) return;
    const size_t spans = (total + span - 1) / span;
    CHECK(read || spans <= T, "%zu spans for %u threads", spans, T);
    std::vector<size_t> next(tasks.size(), 0);
    size_t last_task = 0;
    for (size_t i = 0; i < spans; ++i) {
        const size_t lo = i * span, hi = std::min(total, (i + 1) * span);
        cut_span(
            tasks.size(), [&](size_t k) { return tasks[k]; }, lo, hi, padded, [&](size_t k, size_t a, size_t b) {
                ++g_pieces;
                CHECK(k < tasks.size() && k >= last_task, "task %zu after task %zu", k, last_task);
                if (k >= tasks.size()) return;
                last_task = k;
                CHECK(a < b && b <= tasks[k], "task %zu: piece [%zu, %zu) of %zu", k, a, b, tasks[k]);
                CHECK(a == next[k], "task %zu: piece at %zu, %zu covered", k, a, next[k]);
                CHECK(b - a <= hi - lo, "task %zu: piece of %zu in a span of %zu", k, b - a, hi - lo);
                if (padded) {
                    CHECK(a % 4096 == 0, "task %zu: padded piece starts at %zu", k, a);
                    CHECK(b % 4096 == 0 || b == tasks[k], "task %zu: padded piece ends at %zu of %zu", k, b, tasks[k]);
                }
                next[k] = b;
            });
    }
    for (size_t k = 0; k < tasks.size(); ++k) CHECK(next[k] == tasks[k], "task %zu: %zu of %zu bytes", k, next[k], tasks[k]);
}

static void cuts() {
    const size_t M = size_t(1) << 20;
    const std::vector<std::vector<size_t>> lists = {
        {1},
        {4096},
        {9 * M},
        {3 * M, 3 * M, 3 * M},                       // group D's first window
        {3 * M, 3 * M, 1},
        {3 * M, 5, 70001},
        {0, 8 * M + 1, 0, 1, 4095, 4096, 4097, 0},
        {1, 1, 1, 8 * M, 1, 1, 1},
        {4097, 3 * M + 5, 12289, M - 1, 5 * M + 4095, 17},
        {M, M, M, M, M, M, M, M},
        {M + 1, M + 4095, M + 4096, M + 4097, 2 * M - 1, 3 * M + 1},
        {100, 200, 300},
    };
    std::vector<size_t> many;
    for (size_t k = 0; k < 3000; ++k) many.push_back(1 + (k * 2654435761u) % 9000);
    for (unsigned T = 1; T <= 17; ++T) {
        for (const auto& l : lists)
            for (int mode = 0; mode < 3; ++mode) cut(l, T, mode == 2, mode >= 1);
        for (int mode = 0; mode < 3; ++mode) cut(many, T, mode == 2, mode >= 1);
    }
}

// ---------------------------------------------------------------- the packing schedule
static long g_pack_windows = 0;
static void pack(const std::vector<uint64_t>& L, uint64_t W, uint64_t place) {
    ++g_cases;
    uint64_t total = 0;
    for (uint64_t l : L) total += l;
    PackSched s(L.data(), L.size(), W, place);
    std::vector<WinChunk> win;
    size_t b = 0;       // the blob the walk stands in
    uint64_t off = 0;   // ... and the bytes of it covered
    bool short_window = false;
    for (uint64_t wi = 0; s.next(win); ++wi) {
        ++g_pack_windows;
        CHECK(wi <= total, "schedule does not end");  // every window carries a byte
        if (wi > total) return;
        CHECK(!short_window, "window %llu follows one that was not full", (unsigned long long)wi);
        CHECK(!win.empty(), "window %llu is empty", (unsigned long long)wi);
        uint64_t fill = 0;
        for (const WinChunk& c : win) {
            while (b < L.size() && off == L[b]) ++b, off = 0;  // blobs in index order, empty ones passed over
            CHECK(c.len > 0, "empty chunk of blob %u", c.blob);
            CHECK(b < L.size() && c.blob == b && c.off == off, "chunk of blob %u at %llu, the walk stands in blob %zu at %llu",
                  c.blob, (unsigned long long)c.off, b, (unsigned long long)off);
            if (b >= L.size() || c.blob != b) return;
            CHECK(c.off + c.len <= L[b], "blob %u: chunk ends at %llu of %llu", c.blob, (unsigned long long)(c.off + c.len),
                  (unsigned long long)L[b]);
            CHECK(fill % place == 0 && fill + c.len <= W, "chunk of %llu bytes at +%llu of a window of %llu",
                  (unsigned long long)c.len, (unsigned long long)fill, (unsigned long long)W);
            off = c.off + c.len;
            fill += (c.len + place - 1) / place * place;
        }
        short_window = fill != W;
    }
    while (b < L.size() && off == L[b]) ++b, off = 0;
    CHECK(b == L.size(), "the schedule ended in blob %zu at %llu", b, (unsigned long long)off);
}

static void packs() {
    for (uint64_t place : {uint64_t(16), uint64_t(4096)})
        for (uint64_t W : {place, 3 * place, 8 * place}) {
            const uint64_t edge[9] = {0, 1, place - 1, place, place + 1, W - 1, W, W + 1, 2 * W + 1};
            pack({}, W, place);
            for (uint64_t a : edge) {
                pack({a}, W, place);
                for (uint64_t b : edge) {
                    pack({a, b}, W, place);
                    for (uint64_t c : edge) {
                        pack({a, b, c}, W, place);
                        for (uint64_t d : edge) pack({a, b, c, d}, W, place);
                    }
                }
            }
        }
}

int main() {
    schedules();
    const long sched_cases = g_cases;
    cuts();
    const long cut_cases = g_cases - sched_cases;
    packs();
    printf("window_math: %ld schedules (%ld windows, %ld drops), %ld cuts (%ld pieces), %ld packings (%ld windows), "
           "%ld mismatches\n",
           sched_cases, g_windows, g_drops, cut_cases, g_pieces, g_cases - sched_cases - cut_cases, g_pack_windows, g_bad);
    return g_bad ? 1 : 0;
}
