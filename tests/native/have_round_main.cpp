// have_round_main.cpp -- kraken_amd/csrc/have_round_math.hpp stand-alone under ASan + UBSan: one
// torrent's round a line on standard input (tests/test_have_round_math_native.py).  The row, the
// sidecar span, the verify words, both lists (min(cap, n) entries) and both emitted spans each live
// in a heap block of exactly their size; the outputs, the lists, the spans and the row are printed.
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../kraken_amd/csrc/have_round_math.hpp"

using namespace krk;

static bool get(long long* v) { return scanf("%lld", v) == 1; }
template <class T>
static std::vector<T> block(size_t n) {  // n numbers as an exact heap block of T
    std::vector<T> out(n);
    for (T& x : out) {
        long long v = 0;
        get(&v);
        x = (T)v;
    }
    return out;
}

int main() {
    long long n, flags, piece_length, length, changed_cap, missing_cap, status_len;
    while (get(&n) && get(&flags) && get(&piece_length) && get(&length) && get(&changed_cap) && get(&missing_cap) && get(&status_len)) {
        if (hv::flags_error((uint32_t)flags)) return 2;
        const size_t W = (size_t)pr::words((uint64_t)n), N = (size_t)n;
        const std::vector<uint8_t> status = block<uint8_t>((size_t)status_len);
        std::vector<uint64_t> row = block<uint64_t>(W);
        const std::vector<uint64_t> ok = block<uint64_t>(W);
        std::vector<uint32_t> changed(std::min(N, (size_t)changed_cap)), missing(std::min(N, (size_t)missing_cap));
        std::vector<uint8_t> status_out(flags & hv::kEmitStatus ? N : 0), wire_out(flags & hv::kEmitWire ? 8 + 8 * W : 0);
        const hv::Torrent T = {(uint32_t)flags,  piece_length,          length,         status.data(),     (uint64_t)status_len, ok.data(),
                               changed.data(),   (uint64_t)changed_cap, missing.data(), (uint64_t)missing_cap, status_out.data(),
                               wire_out.data()};
        const hv::Out o = hv::round_torrent(row.data(), (uint64_t)n, T);
        printf("%u %u %u %u %llu", o.flags, o.n_unexpected, o.n_changed, o.n_complete, (unsigned long long)o.bytes);
        const size_t n_missing = flags & hv::kEmitMissing ? std::min(missing.size(), N - o.n_complete) : 0;
        for (size_t k = 0; k < std::min(changed.size(), (size_t)o.n_changed); ++k) printf(" %u", changed[k]);
        for (size_t k = 0; k < n_missing; ++k) printf(" %u", missing[k]);
        for (uint8_t b : status_out) printf(" %u", b);
        for (uint8_t b : wire_out) printf(" %u", b);
        for (uint64_t w : row) printf(" %llu", (unsigned long long)w);
        printf("\n");
    }
    return 0;
}
