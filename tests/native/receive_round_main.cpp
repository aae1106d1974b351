// receive_round_main.cpp -- kraken_amd/csrc/receive_round_math.hpp stand-alone under ASan + UBSan:
// one torrent's round a line on standard input (tests/test_receive_round_math_native.py).  The row,
// the payloads, both sum arrays, the per-payload outputs, both lists and the per-slot arrays each
// live in a heap block of exactly their size; every output, the lists' used fronts and the row are
// printed.
#include <stdio.h>

#include <vector>

#include "../../kraken_amd/csrc/receive_round_math.hpp"

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
    long long n, slots, length, piece_length, n_pays, now;
    while (get(&n) && get(&slots) && get(&length) && get(&piece_length) && get(&n_pays) && get(&now)) {
        if (rv::torrent_error((uint64_t)n, (uint32_t)slots, length, piece_length, (uint64_t)n_pays)) return 2;
        const size_t R = (size_t)n_pays, S = (size_t)slots;
        std::vector<uint64_t> row = block<uint64_t>((size_t)pr::words((uint64_t)n));
        const std::vector<uint32_t> expected = block<uint32_t>((size_t)n), flat = block<uint32_t>(4 * R), sums = block<uint32_t>(R);
        std::vector<sv::Request> pays(R);
        for (size_t r = 0; r < R; ++r)
            pays[r] = {flat[4 * r], (int32_t)flat[4 * r + 1], (int32_t)flat[4 * r + 2], (int32_t)flat[4 * r + 3]};
        std::vector<uint32_t> status(R), arrived(R), from(R), good(S), dup(S);
        std::vector<int64_t> file_off(R), received(S, -1);
        std::vector<rv::Mark> marks(R);
        const rv::Totals o = rv::round_torrent(row.data(), (uint64_t)n, (uint32_t)slots, length, piece_length, pays.data(), sums.data(),
                                               expected.data(), (uint32_t)n_pays, now, status.data(), file_off.data(), arrived.data(),
                                               from.data(), marks.data(), good.data(), dup.data(), received.data());
        printf("%u %u %u %llu %u", o.n_arrived, o.n_marks, o.n_complete, (unsigned long long)o.bytes, o.flags);
        for (size_t r = 0; r < R; ++r) printf(" %u %lld", status[r], (long long)file_off[r]);
        for (uint32_t k = 0; k < o.n_arrived; ++k) printf(" %u %u", arrived[k], from[k]);
        for (uint32_t k = 0; k < o.n_marks; ++k) printf(" %u %u %u", marks[k].piece, marks[k].peer, marks[k].status);
        for (size_t p = 0; p < S; ++p) printf(" %u %u %lld", good[p], dup[p], (long long)received[p]);
        for (uint64_t w : row) printf(" %llu", (unsigned long long)w);
        printf("\n");
    }
    return 0;
}
