// The resend round's host arithmetic (kraken_amd/csrc/piece_resend_math.hpp: what
// krk_piece_resend_round runs) as a stand-alone program: whole torrents at every piece count
// around the word edges, few and many peers, with and without allow-duplicates, lists with runs of
// one piece, every status, gone peers and every small quota, into exactly sized heap arrays (so an
// overrun is the sanitizer's to report) whose rows carry set bits past n, against a quadratic
// reference that finds "an earlier entry with the same piece" by scanning the earlier outputs; and
// the list check at each of its refusals.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../kraken_amd/csrc/piece_resend_math.hpp"

using namespace krk;

static uint64_t rnd(uint64_t& x) {
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
    return x;
}

static bool bit(const uint64_t* row, uint64_t i) { return (row[i / 64] >> (i % 64)) & 1; }

static int check_torrent(uint64_t n, uint32_t n_peers, uint32_t flags, uint64_t n_failed, int density, int& cases) {
    uint64_t x = 0x9E3779B97F4A7C15ull * (n + 1) + n_peers * 131 + flags * 7 + n_failed * 977 + (uint64_t)density * 1000003;
    const uint64_t W = pr::words(n);
    const uint64_t n_rows = 1 + 2 * (uint64_t)n_peers;
    uint64_t* rows = (uint64_t*)malloc(W * n_rows ? W * n_rows * 8 : 1);
    for (uint64_t r = 0; r < n_rows; ++r)
        for (uint64_t w = 0; w < W; ++w) {
            uint64_t v = rnd(x);
            if (r % 2 == 0) v &= rnd(x) & rnd(x);                  // have, blocked: sparser
            if (density == 1 && r % 2 == 1) v &= rnd(x) & rnd(x);  // few holders: peers far down the order win
            if (r % 2 == 1 && w == W - 1 && n % 64) v |= ~0ull << (n % 64);  // past n: never read
            rows[r * W + w] = v;
        }
    int32_t* quota = (int32_t*)malloc(n_peers ? n_peers * 4 : 1);
    for (uint32_t p = 0; p < n_peers; ++p) quota[p] = (int32_t)(rnd(x) % 6) - 1;  // -1 .. 4
    rs::Failed* failed = (rs::Failed*)malloc(n_failed ? n_failed * sizeof(rs::Failed) : 1);
    std::vector<uint32_t> pieces(n_failed);
    for (auto& i : pieces) i = (uint32_t)(rnd(x) % n);
    for (uint64_t f = 1; f < n_failed; f += 2) pieces[f] = pieces[f - 1];  // runs of one piece
    std::sort(pieces.begin(), pieces.end());
    for (uint64_t f = 0; f < n_failed; ++f) {
        const uint32_t peer = (uint32_t)(rnd(x) % (n_peers + 1));
        failed[f] = {pieces[f], peer == n_peers ? pr::kNone : peer, (uint32_t)(rnd(x) % 3) + 1};
    }
    // the reference: every (entry, peer) pair, the same-piece rule from the outputs before it
    std::vector<uint32_t> want(n_failed, pr::kNone);
    std::vector<int32_t> want_left(n_peers);
    uint32_t want_resent = 0;
    for (uint32_t p = 0; p < n_peers; ++p) want_left[p] = quota[p] < 0 ? 0 : quota[p];
    for (uint64_t f = 0; f < n_failed; ++f) {
        const uint32_t i = failed[f].piece;
        for (uint32_t p = 0; p < n_peers && want[f] == pr::kNone; ++p) {
            const uint64_t* b = rows + (1 + 2 * (uint64_t)p) * W;
            if ((failed[f].status == rs::kExpired || failed[f].status == rs::kInvalid) && p == failed[f].peer) continue;
            if (!bit(b, i) || bit(rows, i) || want_left[p] == 0 || bit(b + W, i)) continue;
            bool earlier = false;
            for (uint64_t g = 0; g < f; ++g)
                if (failed[g].piece == i && want[g] != pr::kNone && ((flags & pr::kAllowDuplicates) == 0 || want[g] == p))
                    earlier = true;
            if (earlier) continue;
            want[f] = p;
            --want_left[p];
            ++want_resent;
        }
    }
    int wrong = 0;
    uint64_t at = 0;
    wrong += rs::list_error(failed, n_failed, n, n_peers, &at) != nullptr;
    uint32_t* mark = (uint32_t*)malloc(n_peers ? n_peers * 4 : 1);
    uint32_t* target = (uint32_t*)malloc(n_failed ? n_failed * 4 : 1);
    int32_t* left = (int32_t*)malloc(n_peers ? n_peers * 4 : 1);
    memset(mark, 0xA5, n_peers * 4);
    memset(target, 0xA5, n_failed * 4);
    memset(left, 0xA5, n_peers * 4);
    wrong += rs::resend_torrent(rows, n, n_peers, flags, quota, failed, n_failed, mark, target, left) != want_resent;
    for (uint64_t f = 0; f < n_failed; ++f) wrong += target[f] != want[f];
    for (uint32_t p = 0; p < n_peers; ++p) wrong += left[p] != want_left[p];
    free(rows), free(quota), free(failed), free(mark), free(target), free(left);
    ++cases;
    return wrong;
}

static int check_lists() {
    int wrong = 0;
    uint64_t at = 99;
    const rs::Failed ok[] = {{0, 0, 1}, {0, pr::kNone, 2}, {64, 2, 3}};
    wrong += rs::list_error(ok, 3, 65, 3, &at) != nullptr;
    wrong += rs::list_error(nullptr, 0, 0, 0, &at) != nullptr;
    const rs::Failed bad[][2] = {{{0, 0, 1}, {65, 0, 1}}, {{0, 0, 1}, {1, 3, 1}},          {{0, 0, 1}, {1, 0, 0}},
                                 {{0, 0, 1}, {1, 0, 4}},  {{5, 0, 1}, {4, 0, 1}}, {{0, 0, 1}, {1, pr::kNone - 1, 1}}};
    for (auto& b : bad) wrong += rs::list_error(b, 2, 65, 3, &at) == nullptr || at != 1;
    wrong += !rs::flags_ok(pr::kSample | pr::kAllowDuplicates) || !rs::flags_ok(0xFF) || rs::flags_ok(0x200);
    wrong += rs::quota_left(-5) != 0 || rs::quota_left(0) != 0 || rs::quota_left(7) != 7;
    wrong += rs::excludes_own_peer(rs::kUnsent) || !rs::excludes_own_peer(rs::kExpired) || !rs::excludes_own_peer(rs::kInvalid);
    return wrong;
}

int main() {
    int mismatches = check_lists(), cases = 0;
    for (uint64_t n : {1, 2, 63, 64, 65, 127, 128, 129, 300})
        for (uint32_t n_peers : {0u, 1u, 2u, 7u, 70u})
            for (uint32_t flags : {0u, pr::kAllowDuplicates, pr::kSample | pr::kAllowDuplicates})
                for (uint64_t n_failed : {0, 1, 2, 9, 200})
                    for (int density = 0; density < 2; ++density)
                        mismatches += check_torrent(n, n_peers, flags, n_failed, density, cases);
    mismatches += check_torrent(4097, 600, pr::kAllowDuplicates, 500, 1, cases);
    printf("piece_resend_math: %d cases, %d mismatches\n", cases, mismatches);
    return mismatches != 0;
}
