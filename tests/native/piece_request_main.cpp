// The piece request round's host arithmetic (kraken_amd/csrc/piece_request_math.hpp: what
// krk_piece_availability, krk_piece_select and krk_piece_request_round run) as a stand-alone
// program: availability, selection and whole rounds at every piece count around the word edges,
// both policies, with and without allow-duplicates, every quota from 0 to the maximum, into
// exactly sized heap arrays (so an overrun is the sanitizer's to report) whose rows carry set
// bits past n, against a piece-at-a-time reference that sorts every candidate.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../kraken_amd/csrc/piece_request_math.hpp"

using namespace krk;

static uint64_t rnd(uint64_t& x) {
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
    return x;
}

static bool bit(const uint64_t* row, uint64_t i) { return (row[i / 64] >> (i % 64)) & 1; }

static int check_round(uint64_t n, uint32_t n_peers, uint32_t flags, uint32_t limit, int density, int& cases) {
    uint64_t x = 0x9E3779B97F4A7C15ull * (n + 1) + n_peers * 131 + flags * 7 + limit + (uint64_t)density * 1000003;
    const uint64_t W = pr::words(n), seed = rnd(x);
    const uint64_t n_rows = 1 + 2 * (uint64_t)n_peers;
    uint64_t* rows = (uint64_t*)malloc(W * n_rows ? W * n_rows * 8 : 1);
    for (uint64_t r = 0; r < n_rows; ++r)
        for (uint64_t w = 0; w < W; ++w) {
            uint64_t v = rnd(x);
            if (r % 2 == 0) v &= rnd(x);                          // have, blocked: sparser
            if (density == 1 && r % 2 == 1) v = ~0ull;            // every peer has every piece: all counts equal
            if (density == 1 && r % 2 == 0) v = 0;
            if (r % 2 == 1 && w == W - 1 && n % 64) v |= ~0ull << (n % 64);  // past n: must not come through
            rows[r * W + w] = v;
        }
    int32_t* quota = (int32_t*)malloc(n_peers ? n_peers * 4 : 1);
    for (uint32_t p = 0; p < n_peers; ++p) quota[p] = (int32_t)(rnd(x) % (limit + 2)) - 1;  // -1 .. limit
    // the reference: counts piece by piece, then every candidate sorted by (key, index)
    std::vector<uint32_t> counts(n);
    for (uint64_t i = 0; i < n; ++i)
        for (uint32_t p = 0; p < n_peers; ++p) counts[i] += bit(rows + (1 + 2 * (uint64_t)p) * W, i);
    std::vector<uint32_t> want_picks((uint64_t)n_peers * limit, pr::kNone), want_n(n_peers);
    std::vector<bool> taken(n);
    for (uint32_t p = 0; p < n_peers; ++p) {
        const uint64_t* b = rows + (1 + 2 * (uint64_t)p) * W;
        std::vector<uint64_t> keyed;
        for (uint64_t i = 0; i < n; ++i)
            if (bit(b, i) && !bit(rows, i) && !bit(b + W, i) && !taken[i]) {
                const uint64_t key = (flags & pr::kPolicyMask) == pr::kSample
                                         ? pr::splitmix64(seed ^ ((uint64_t)p << 32 | i)) >> 32
                                         : counts[i];
                keyed.push_back(key << 32 | i);
            }
        std::sort(keyed.begin(), keyed.end());
        const uint64_t q = quota[p] <= 0 ? 0 : (uint64_t)quota[p];
        want_n[p] = (uint32_t)std::min<uint64_t>(q, keyed.size());
        for (uint32_t j = 0; j < want_n[p]; ++j) {
            want_picks[(uint64_t)p * limit + j] = (uint32_t)keyed[j];
            if (!(flags & pr::kAllowDuplicates)) taken[(uint32_t)keyed[j]] = true;
        }
    }
    int wrong = 0;
    uint32_t* got_counts = (uint32_t*)malloc(n ? n * 4 : 1);
    memset(got_counts, 0xA5, n * 4);
    pr::availability(rows + W, 2 * W, n_peers, n, got_counts);
    for (uint64_t i = 0; i < n; ++i) wrong += got_counts[i] != counts[i];
    uint64_t* scratch = (uint64_t*)malloc(W ? W * 8 : 1);
    memset(scratch, 0xA5, W * 8);
    uint32_t* picks = (uint32_t*)malloc(n_peers ? (uint64_t)n_peers * limit * 4 : 1);
    uint32_t* n_picked = (uint32_t*)malloc(n_peers ? n_peers * 4 : 1);
    memset(picks, 0xA5, (uint64_t)n_peers * limit * 4);
    memset(n_picked, 0xA5, n_peers * 4);
    pr::round_torrent(rows, n, n_peers, flags, seed, quota, limit, got_counts, scratch, picks, n_picked);
    for (uint32_t p = 0; p < n_peers; ++p) wrong += n_picked[p] != want_n[p];
    for (uint64_t k = 0; k < (uint64_t)n_peers * limit; ++k) wrong += picks[k] != want_picks[k];
    // one peer's selection on its own: the first peer of the round saw nothing taken
    if (n_peers) {
        uint32_t* one = (uint32_t*)malloc(limit * 4);
        const uint32_t q = quota[0] <= 0 ? 0 : (uint32_t)quota[0];
        const uint32_t m = pr::select(rows + W, rows, rows + 2 * W, nullptr, got_counts, n, q, flags & pr::kPolicyMask, seed, 0, one);
        wrong += m != want_n[0];
        for (uint32_t j = 0; j < m; ++j) wrong += one[j] != want_picks[j];
        free(one);
    }
    free(rows), free(quota), free(got_counts), free(scratch), free(picks), free(n_picked);
    ++cases;
    return wrong;
}

int main() {
    int mismatches = 0, cases = 0;
    const uint64_t want[][2] = {{0, 0}, {1, 1}, {63, 1}, {64, 1}, {65, 2}, {(1ull << 32) - 1, 1ull << 26}};
    for (auto& w : want) mismatches += pr::words(w[0]) != w[1];
    mismatches += pr::splitmix64(0) != 0xE220A8397B1DCDAFull;
    mismatches += pr::live_bits(64, 0) != ~0ull || pr::live_bits(65, 1) != 1 || pr::live_bits(63, 0) != ~0ull >> 1;
    mismatches += !pr::flags_ok(pr::kSample | pr::kAllowDuplicates) || pr::flags_ok(2) || pr::flags_ok(0x200);
    for (uint64_t n : {0, 1, 63, 64, 65, 127, 128, 129, 300})
        for (uint32_t n_peers : {0u, 1u, 2u, 7u})
            for (uint32_t flags : {pr::kRarestFirst, pr::kSample, pr::kRarestFirst | pr::kAllowDuplicates,
                                   pr::kSample | pr::kAllowDuplicates})
                for (uint32_t limit : {1u, 3u, pr::kMaxLimit})
                    for (int density = 0; density < 2; ++density)
                        mismatches += check_round(n, n_peers, flags, limit, density, cases);
    mismatches += check_round(2000, 300, pr::kRarestFirst, pr::kMaxLimit, 1, cases);  // counts past 255
    printf("piece_request_math: %d cases, %d mismatches\n", cases, mismatches);
    return mismatches != 0;
}
