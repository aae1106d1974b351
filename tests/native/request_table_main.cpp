// request_table_main.cpp -- kraken_amd/csrc/request_table_math.hpp stand-alone (nothing of the library
// linked), under AddressSanitizer and UndefinedBehaviorSanitizer: one torrent's round a line on standard
// input (tests/test_request_table_math_native.py sends the named cases), run over heap blocks of exactly
// the documented sizes, state and outputs printed for the test to hold against the hand-worked values.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../kraken_amd/csrc/request_table_math.hpp"

using namespace krk;

static bool get(long long* v) { return scanf("%lld", v) == 1; }
template <class T>
static std::vector<T> words(size_t n) {  // n numbers as an exact heap block of T (4- or 8-byte words)
    std::vector<T> out(n);
    for (T& x : out) {
        long long v = 0;
        get(&v);
        x = (T)v;
    }
    return out;
}
template <class T>
static std::vector<T> list(uint32_t* n, size_t width) {  // a count, then count * width uint32 words, as T
    long long k = 0;
    get(&k);
    *n = (uint32_t)k;
    const std::vector<uint32_t> w = words<uint32_t>((size_t)k * width);
    std::vector<T> out((size_t)k);
    if (k) memcpy(out.data(), w.data(), w.size() * 4);
    return out;
}

int main() {
    long long n, P, flags, cap, limit, now, timeout, has_picks, ne;
    while (get(&n) && get(&P) && get(&flags) && get(&cap) && get(&limit) && get(&now) && get(&timeout) && get(&has_picks) && get(&ne)) {
        const rt::Round R{now, timeout, (uint32_t)limit};
        std::vector<rt::Entry> table((size_t)cap);
        for (long long e = 0; e < ne; ++e) {
            const std::vector<long long> f = words<long long>(4);
            table[(size_t)e] = {(uint32_t)f[0], (uint32_t)f[1], (uint32_t)f[2], 0, f[3]};
        }
        rt::Lists l{};
        const std::vector<uint32_t> arrived = list<uint32_t>(&l.n_arrived, 1), gone = list<uint32_t>(&l.n_gone, 1);
        const std::vector<rs::Failed> marks = list<rs::Failed>(&l.n_marks, 3);
        const std::vector<rt::Pair> holds = list<rt::Pair>(&l.n_holds, 2), records = list<rt::Pair>(&l.n_records, 2);
        l.arrived = arrived.data(), l.gone = gone.data(), l.marks = marks.data(), l.holds = holds.data(), l.records = records.data();
        std::vector<uint64_t> rows = words<uint64_t>((size_t)((1 + 2 * P) * (long long)pr::words((uint64_t)n)));
        const std::vector<uint32_t> picks = words<uint32_t>((size_t)(P * limit)), n_picked = words<uint32_t>((size_t)P);
        uint64_t at = 0;
        if (rt::round_error(R) || rt::lists_error(l, (uint64_t)n, (uint32_t)P, &at)) return 2;
        std::vector<uint64_t> keys((size_t)cap);
        std::vector<int32_t> quota((size_t)P);
        std::vector<rs::Failed> failed((size_t)cap);
        uint32_t count = (uint32_t)ne, nf = 0, nd = 0;
        rt::round_torrent(rows.data(), (uint64_t)n, (uint32_t)P, (uint32_t)flags, table.data(), &count, (uint32_t)cap, l,
                          has_picks ? picks.data() : nullptr, has_picks ? n_picked.data() : nullptr, R, keys.data(), quota.data(),
                          failed.data(), &nf, &nd);
        printf("%u %u", count, nd);
        for (int32_t q : quota) printf(" %d", q);
        printf(" %u", nf);
        for (uint32_t f = 0; f < nf; ++f) printf(" %u %u %u", failed[f].piece, failed[f].peer, failed[f].status);
        for (uint32_t e = 0; e < count; ++e)
            printf(" %u %u %u %lld", table[e].piece, table[e].peer, table[e].status, (long long)table[e].sent_at);
        for (uint64_t w : rows) printf(" %llu", (unsigned long long)w);
        printf("\n");
    }
    return 0;
}
