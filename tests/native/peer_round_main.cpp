// peer_round_main.cpp -- kraken_amd/csrc/peer_round_math.hpp stand-alone (nothing of the library
// linked), under AddressSanitizer and UndefinedBehaviorSanitizer: one torrent's round a line on standard
// input (tests/test_peer_round_math_native.py sends the named cases).  Every join runs as a round of its
// own with its span in a heap block of exactly the span's size, so that a read outside the span is
// reported; a last round applies the fulls and derives.  The rows and the outputs are printed.
#include <stdio.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "../../kraken_amd/csrc/peer_round_math.hpp"

using namespace krk;

static bool get(long long* v) { return scanf("%lld", v) == 1; }
template <class T>
static std::vector<T> words(size_t n) {  // n numbers as an exact heap block of T
    std::vector<T> out(n);
    for (T& x : out) {
        long long v = 0;
        get(&v);
        x = (T)v;
    }
    return out;
}

int main() {
    long long n, P, threshold, flags, n_joins, n_fulls;
    while (get(&n) && get(&P) && get(&threshold) && get(&flags)) {
        std::vector<uint64_t> rows = words<uint64_t>((size_t)((1 + 2 * P) * (long long)pr::words((uint64_t)n)));
        const std::vector<uint64_t> live = words<uint64_t>((size_t)((P + 63) / 64));
        std::vector<uint32_t> held((size_t)P), wanted((size_t)P), status((size_t)P), joined((size_t)P);
        uint32_t remaining = 0, tflags = 0;
        uint64_t at = 0;
        auto round = [&](const pe::Join* j, uint32_t nj, const uint32_t* f, uint32_t nf, const uint8_t* wire) {
            if (pe::lists_error(j, nj, f, nf, (uint32_t)P, &at)) return false;
            pe::round_torrent(rows.data(), (uint64_t)n, (uint32_t)P, live.data(), j, nj, f, nf, wire, (uint32_t)threshold,
                              (uint32_t)flags, &remaining, &tflags, held.data(), wanted.data(), status.data());
            return true;
        };
        get(&n_joins);
        for (long long k = 0; k < n_joins; ++k) {
            long long peer, len;
            get(&peer), get(&len);
            const std::vector<uint8_t> bytes = words<uint8_t>((size_t)len);
            std::unique_ptr<uint8_t[]> span(new uint8_t[(size_t)len]);  // exactly the span
            std::copy(bytes.begin(), bytes.end(), span.get());
            const pe::Join j{(uint32_t)peer, 0, 0, (uint64_t)len};
            if (!round(&j, 1, nullptr, 0, span.get())) return 2;
            joined[(size_t)peer] = status[(size_t)peer] & (pe::kJoined | pe::kBadBitfield);
        }
        get(&n_fulls);
        const std::vector<uint32_t> fulls = words<uint32_t>((size_t)n_fulls);
        if (!round(nullptr, 0, fulls.data(), (uint32_t)n_fulls, nullptr)) return 2;
        printf("%u %u", remaining, tflags);
        for (long long p = 0; p < P; ++p) printf(" %u %u %u", held[(size_t)p], wanted[(size_t)p], status[(size_t)p] | joined[(size_t)p]);
        for (uint64_t w : rows) printf(" %llu", (unsigned long long)w);
        printf("\n");
    }
    return 0;
}
