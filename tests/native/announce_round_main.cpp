// The announce round's host arithmetic (kraken_amd/csrc/announce_math.hpp: what
// krk_announce_handout and krk_announce_round run) as a stand-alone program: peer stores at every
// peer count around the word edges, every window count with every cur_row, the limits 1, 50 and
// 64, every origin count, both policies, sources inside, outside and absent, complete announcers,
// into exactly sized heap arrays (so an overrun is the sanitizer's to report) whose rows carry set
// bits past P, against a quadratic reference that orders by repeated minimum search; and the
// checks at each of their refusals.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../kraken_amd/csrc/announce_math.hpp"

using namespace krk;

static uint64_t rnd(uint64_t& x) {
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
    return x;
}

static bool bit(const uint64_t* row, uint64_t i) { return (row[i / 64] >> (i % 64)) & 1; }

// The handout by definition: every window's whole member list ordered by repeated minimum search.
static std::vector<uint32_t> want_handout(const uint64_t* rows, const an::Torrent& t, const an::Announce& a, uint32_t limit,
                                          uint32_t policy, uint32_t labels[3]) {
    labels[0] = labels[1] = labels[2] = 0;
    std::vector<uint32_t> out;
    if (a.flags & an::kComplete) return out;
    const uint64_t wp = pr::words(t.n_peers);
    std::vector<uint32_t> windows(t.n_windows);
    for (uint32_t w = 0; w < t.n_windows; ++w) windows[w] = w;
    std::sort(windows.begin(), windows.end(), [&](uint32_t x, uint32_t y) {
        return std::make_pair(an::wkey(a.seed, x), x) < std::make_pair(an::wkey(a.seed, y), y);
    });
    std::vector<std::pair<uint32_t, bool>> sel;
    for (uint32_t w : windows) {
        if (sel.size() >= limit) break;
        const uint64_t* member = rows + 2 * (uint64_t)((t.cur_row + w) % t.n_windows) * wp;
        std::vector<std::pair<uint32_t, uint32_t>> keyed;
        for (uint32_t i = 0; i < t.n_peers; ++i)
            if (bit(member, i)) keyed.push_back({an::pkey(a.seed, w, i), i});
        std::sort(keyed.begin(), keyed.end());
        keyed.resize(std::min<size_t>(keyed.size(), limit - sel.size()));
        for (auto& k : keyed) {
            const bool c = bit(member + wp, k.second);
            auto it = std::find_if(sel.begin(), sel.end(), [&](auto& s) { return s.first == k.second; });
            if (it == sel.end()) sel.push_back({k.second, c});
            else it->second = it->second || c;
        }
    }
    struct E {
        uint32_t prio, key, c, word;
    };
    std::vector<E> es;
    for (auto& s : sel)
        if (s.first != a.source)
            es.push_back({policy == an::kCompleteness ? (s.second ? 0u : 2u) : 0u, an::okey(a.seed, s.first), s.first,
                          s.first | (s.second ? an::kCompleteBit : 0)});
    for (uint32_t o = 0; o < t.n_origins; ++o)
        es.push_back({policy == an::kCompleteness ? 1u : 0u, an::okey(a.seed, an::kOrigin | o), an::kOrigin | o, an::kOrigin | o});
    std::sort(es.begin(), es.end(), [](const E& x, const E& y) {
        return x.prio != y.prio ? x.prio < y.prio : x.key != y.key ? x.key < y.key : x.c < y.c;
    });
    for (auto& e : es) {
        out.push_back(e.word);
        ++labels[e.prio];
    }
    return out;
}

static int check_store(uint64_t P, uint32_t W, uint32_t cur, uint32_t O, uint32_t limit, uint32_t policy, int density,
                       int& cases) {
    uint64_t x = 0x9E3779B97F4A7C15ull * (P + 1) + W * 131 + cur * 7 + O * 977 + limit * 31 + policy + (uint64_t)density * 1000003;
    const uint64_t wp = pr::words(P), n_words = 2 * (uint64_t)W * wp;
    uint64_t* rows = (uint64_t*)malloc(n_words * 8);
    for (uint64_t r = 0; r < 2 * (uint64_t)W; ++r)
        for (uint64_t w = 0; w < wp; ++w) {
            uint64_t v = rnd(x);
            if (density == 1) v &= rnd(x) & rnd(x) & rnd(x);
            if (density == 2 && r / 2 % 2) v = 0;  // every other window empty
            if (w == wp - 1 && P % 64) v |= ~0ull << (P % 64);  // past P: never read as a peer
            rows[r * wp + w] = v;
        }
    const an::Torrent t = {P, W, cur, O, 0, 0};
    int wrong = an::torrent_error(t) != nullptr;
    for (int k = 0; k < 6; ++k) {
        an::Announce a = {0, (uint32_t)(rnd(x) % P), k == 4 ? an::kComplete : 0u, 0, rnd(x)};
        a.source = k % 3 == 0 ? an::kNone : k % 3 == 1 ? a.peer : (uint32_t)(rnd(x) % P);
        wrong += an::announce_error(a, &t, 1) != nullptr;
        // the update sets its two bits and nothing else
        std::vector<uint64_t> before(rows, rows + n_words);
        an::update(rows, t, a);
        before[2 * (uint64_t)cur * wp + a.peer / 64] |= 1ull << (a.peer % 64);
        if (a.flags & an::kComplete) before[(2 * (uint64_t)cur + 1) * wp + a.peer / 64] |= 1ull << (a.peer % 64);
        wrong += memcmp(before.data(), rows, n_words * 8) != 0;
        uint32_t want_labels[3], labels[3] = {9, 9, 9};
        const std::vector<uint32_t> want = want_handout(rows, t, a, limit, policy, want_labels);
        const uint32_t cap = limit + an::kMaxOrigins;
        uint32_t* out = (uint32_t*)malloc(cap * 4);
        memset(out, 0xA5, cap * 4);
        const uint32_t n = an::handout(rows, t, a, limit, policy, out, labels);
        wrong += n != want.size() || memcmp(labels, want_labels, sizeof labels) != 0;
        for (uint32_t j = 0; j < cap; ++j) wrong += out[j] != (j < want.size() ? want[j] : an::kNone);
        free(out);
        ++cases;
    }
    free(rows);
    return wrong;
}

static int check_refusals() {
    int wrong = 0;
    const an::Torrent ok = {65, 5, 4, 8, 0, 123};
    wrong += an::torrent_error(ok) != nullptr;
    an::Torrent bad[] = {ok, ok, ok, ok, ok, ok, ok};
    bad[0].n_peers = 1ull << 30;
    bad[1].n_windows = 0;
    bad[2].n_windows = 9, bad[2].cur_row = 0;
    bad[3].cur_row = 5;
    bad[4].n_origins = 9;
    bad[5].reserved = 1;
    bad[6].bits_off = 1ull << 48;
    for (auto& b : bad) wrong += an::torrent_error(b) == nullptr;
    const an::Announce fine = {0, 64, an::kComplete, an::kNone, ~0ull};
    wrong += an::announce_error(fine, &ok, 1) != nullptr;
    an::Announce worse[] = {fine, fine, fine, fine, fine};
    worse[0].torrent = 1;
    worse[1].peer = 65;
    worse[2].source = 65;
    worse[3].source = an::kNone - 1;
    worse[4].flags = 3;
    for (auto& a : worse) wrong += an::announce_error(a, &ok, 1) == nullptr;
    wrong += an::announce_error(fine, nullptr, 0) == nullptr;
    wrong += an::scalars_error(1, 0) != nullptr || an::scalars_error(64, 1) != nullptr;
    wrong += an::scalars_error(0, 0) == nullptr || an::scalars_error(65, 0) == nullptr || an::scalars_error(50, 2) == nullptr;
    wrong += an::priority(an::kDefault, true, true) != 0 || an::priority(an::kCompleteness, true, true) != 1 ||
             an::priority(an::kCompleteness, false, true) != 0 || an::priority(an::kCompleteness, false, false) != 2;
    wrong += an::live_bits(65, 0) != ~0ull || an::live_bits(65, 1) != 1 || an::live_bits(64, 0) != ~0ull;
    return wrong;
}

int main() {
    int mismatches = check_refusals(), cases = 0;
    for (uint64_t P : {1, 2, 63, 64, 65, 127, 128, 129, 300})
        for (uint32_t W : {1u, 2u, 5u, 8u})
            for (uint32_t limit : {1u, 50u, 64u})
                for (int density = 0; density < 3; ++density) {
                    const uint32_t cur = (uint32_t)((P + limit + density) % W), O = (uint32_t)((P + W + density) % 9);
                    mismatches += check_store(P, W, cur, O, limit, (uint32_t)((P + density) % 2), density, cases);
                }
    mismatches += check_store(4097, 8, 7, 8, 64, an::kCompleteness, 0, cases);
    mismatches += check_store(4097, 5, 2, 3, 50, an::kDefault, 1, cases);
    printf("announce_math: %d cases, %d mismatches\n", cases, mismatches);
    return mismatches != 0;
}
