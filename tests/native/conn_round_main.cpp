// The connection round's host arithmetic (kraken_amd/csrc/conn_math.hpp: what krk_conn_round and
// krk_conn_preempt run) as a stand-alone program: torrents at every peer count around the word
// edges, lists of every length around the 64-entry step, random active, pending and blacklist
// state, into exactly sized heap arrays (so an overrun is the sanitizer's to report) whose rows
// carry set bits past P, against a naive loop over std::set that shares nothing with the header
// but its constants; the sweep at its thresholds; and the checks at each of their refusals.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <set>
#include <vector>

#include "../../kraken_amd/csrc/conn_math.hpp"

using namespace krk;

static uint64_t rnd(uint64_t& x) {
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
    return x;
}

struct Naive {
    std::set<uint32_t> active, pending;
    std::map<uint32_t, int64_t> expiry;
    uint32_t cap;
    bool blacklisted(uint32_t p, int64_t now) { return expiry.count(p) && expiry[p] > now; }
    uint32_t blacklist(uint32_t p, const cn::Round& r) {
        if (r.flags & cn::kDisableBlacklist) return 0;
        if (blacklisted(p, r.now)) return cn::kStillBlacklisted;
        expiry[p] = r.now + r.blacklist_duration;
        return cn::kBlacklistedNow;
    }
    uint32_t add_pending(uint32_t p, const std::vector<uint32_t>* neigh, uint32_t max_mutual) {
        if (cap == 0) return cn::kAtCapacity;
        if (pending.count(p)) return cn::kAlreadyPending;
        if (active.count(p)) return cn::kAlreadyActive;
        if (neigh) {
            uint32_t n = 0;
            for (uint32_t q : *neigh) n += active.count(q) || pending.count(q);
            if (n > max_mutual) return cn::kTooManyMutual;
        }
        pending.insert(p);
        --cap;
        return cn::kOk;
    }
};

static int check_torrent(uint32_t P, uint64_t n_tr, uint64_t n_in, uint64_t n_dial, uint32_t cap, uint32_t tflags,
                         uint32_t rflags, uint32_t max_mutual, int& cases) {
    uint64_t x = 0x9E3779B97F4A7C15ull * (P + 1) + n_tr * 131 + n_in * 7 + n_dial * 977 + cap * 31 + tflags + rflags * 3;
    const uint64_t wp = pr::words(P);
    const cn::Round R = {1000, 30, max_mutual, rflags};
    Naive N;
    N.cap = cap;
    uint64_t* rows = (uint64_t*)malloc(2 * wp * 8 + 1);
    int64_t* expiry = (int64_t*)malloc(P * 8 + 1);
    memset(rows, 0, 2 * wp * 8);
    for (uint32_t p = 0; p < P; ++p) {
        const uint64_t v = rnd(x) % 7;
        if (v == 0) N.active.insert(p), rows[p / 64] |= 1ull << (p % 64);
        if (v == 1) N.pending.insert(p), rows[wp + p / 64] |= 1ull << (p % 64);
        expiry[p] = rnd(x) % 5 == 0 ? (int64_t)(999 + rnd(x) % 3) : 0;
        if (expiry[p]) N.expiry[p] = expiry[p];
    }
    const uint64_t tail = P % 64 ? ~0ull << (P % 64) : 0;  // past P: never read as a peer, never changed
    if (wp) rows[wp - 1] |= tail & rnd(x), rows[2 * wp - 1] |= tail & rnd(x);
    const uint64_t tail_a = wp ? rows[wp - 1] & tail : 0, tail_p = wp ? rows[2 * wp - 1] & tail : 0;

    n_tr = n_tr < P ? n_tr : P;
    std::set<uint32_t> tp;
    while (tp.size() < n_tr) tp.insert((uint32_t)(rnd(x) % P));
    cn::Transition* tr = (cn::Transition*)malloc(n_tr * sizeof(cn::Transition) + 1);
    uint64_t k = 0;
    for (uint32_t p : tp) tr[k++] = {p, (uint32_t)(rnd(x) % 4)};
    cn::Incoming* in = (cn::Incoming*)malloc(n_in * sizeof(cn::Incoming) + 1);
    uint64_t* neigh = (uint64_t*)malloc(n_in * wp * 8 + 1);
    std::vector<std::vector<uint32_t>> nb(n_in);
    for (k = 0; k < n_in; ++k) {
        in[k] = {(uint32_t)(rnd(x) % P), 0, k % 4 == 3 ? cn::kNoRow : k * wp};
        memset(neigh + k * wp, 0, wp * 8);
        const uint64_t one_in = 1 + rnd(x) % 40;
        for (uint32_t p = 0; p < P; ++p)
            if (rnd(x) % one_in == 0) nb[k].push_back(p), neigh[k * wp + p / 64] |= 1ull << (p % 64);
        neigh[k * wp + wp - 1] |= tail & rnd(x);
    }
    uint32_t* dial = (uint32_t*)malloc(n_dial * 4 + 1);
    for (k = 0; k < n_dial; ++k) dial[k] = (uint32_t)(rnd(x) % P);
    const cn::Torrent T = {P, (uint32_t)(P % 3 == 0 ? cn::kNone : rnd(x) % P), tflags, 0, 0, 0, 0};
    const cn::Lists L = {0, n_tr, 0, n_in, 0, n_dial};
    uint64_t at = 0;
    int wrong = cn::torrent_error(T) != nullptr || cn::lists_error(T, L, tr, in, dial, n_in * wp, &at) != nullptr;

    // the naive round
    std::vector<uint32_t> w_tr, w_in, w_dial;
    uint32_t w_freed = 0;
    for (k = 0; k < n_tr; ++k) {
        const uint32_t p = tr[k].peer, kind = tr[k].kind;
        uint32_t st;
        if (kind == cn::kEstablished) {
            st = N.pending.erase(p) ? (N.active.insert(p), cn::kOk) : cn::kNotPending;
        } else {
            std::set<uint32_t>& held = kind == cn::kClosed ? N.active : N.pending;
            if (held.erase(p)) st = cn::kOk | cn::kFreed, ++N.cap, ++w_freed;
            else st = cn::kNoop;
            if (kind != cn::kFailedIn) st |= N.blacklist(p, R);
        }
        w_tr.push_back(st);
    }
    for (k = 0; k < n_in; ++k) w_in.push_back(N.add_pending(in[k].peer, in[k].neigh_off == cn::kNoRow ? nullptr : &nb[k], max_mutual));
    for (k = 0; k < n_dial; ++k) {
        const uint32_t p = dial[k];
        w_dial.push_back(tflags & cn::kTorrentComplete ? cn::kTorrentIsComplete
                         : p == T.self_peer            ? cn::kSelf
                         : N.blacklisted(p, R.now)     ? cn::kBlacklisted
                                                       : N.add_pending(p, nullptr, 0));
    }

    uint32_t* s_tr = (uint32_t*)malloc(n_tr * 4 + 1);
    uint32_t* s_in = (uint32_t*)malloc(n_in * 4 + 1);
    uint32_t* s_dial = (uint32_t*)malloc(n_dial * 4 + 1);
    uint32_t admitted[2] = {9, 9}, freed = 9, c = cap;
    cn::round_torrent(T, L, R, rows, expiry, &c, tr, in, dial, neigh, s_tr, s_in, s_dial, admitted, &freed);
    for (k = 0; k < n_tr; ++k) wrong += s_tr[k] != w_tr[k];
    for (k = 0; k < n_in; ++k) wrong += s_in[k] != w_in[k];
    for (k = 0; k < n_dial; ++k) wrong += s_dial[k] != w_dial[k];
    uint32_t a_in = 0, a_dial = 0;
    for (uint32_t s : w_in) a_in += s == cn::kOk;
    for (uint32_t s : w_dial) a_dial += s == cn::kOk;
    wrong += admitted[0] != a_in || admitted[1] != a_dial || freed != w_freed || c != N.cap;
    for (uint32_t p = 0; p < P; ++p) {
        wrong += cn::bit(rows, p) != (N.active.count(p) != 0) || cn::bit(rows + wp, p) != (N.pending.count(p) != 0);
        wrong += expiry[p] != (N.expiry.count(p) ? N.expiry[p] : 0);
    }
    if (wp) wrong += (rows[wp - 1] & tail) != tail_a || (rows[2 * wp - 1] & tail) != tail_p;
    free(rows), free(expiry), free(tr), free(in), free(neigh), free(dial), free(s_tr), free(s_in), free(s_dial);
    ++cases;
    return wrong;
}

static int check_sweep(uint32_t P, int& cases) {
    uint64_t x = 77 + P;
    const uint64_t wp = pr::words(P);
    uint64_t* active = (uint64_t*)malloc(wp * 8 + 1);
    uint64_t* close = (uint64_t*)malloc(wp * 8 + 1);
    int64_t* t[3];
    for (auto& a : t) a = (int64_t*)malloc(P * 8 + 1);
    for (uint64_t w = 0; w < wp; ++w) active[w] = rnd(x);  // tail bits included
    for (uint32_t p = 0; p < P; ++p)
        for (auto& a : t) a[p] = (int64_t)(rnd(x) % 1100) - 10;
    memset(close, 0xA5, wp * 8);
    const uint32_t n = cn::preempt_torrent(P, active, t[0], t[1], t[2], 1000, 100, 500, close);
    int wrong = 0;
    uint32_t want_n = 0;
    for (uint32_t p = 0; p < P; ++p) {
        int64_t c = t[0][p] < 0 ? 0 : t[0][p], last = c;
        for (int j = 1; j < 3; ++j) last = t[j][p] > last ? t[j][p] : last;
        const bool want = ((active[p / 64] >> (p % 64)) & 1) && (1000 - last > 100 || 1000 - c > 500);
        wrong += want != (((close[p / 64] >> (p % 64)) & 1) != 0);
        want_n += want;
    }
    if (P % 64) wrong += (close[wp - 1] >> (P % 64)) != 0;
    wrong += n != want_n;
    free(active), free(close);
    for (auto& a : t) free(a);
    ++cases;
    return wrong;
}

static int check_refusals() {
    int wrong = 0;
    const cn::Round ok = {5, 7, 3, cn::kDisableBlacklist};
    wrong += cn::scalars_error(ok) != nullptr;
    cn::Round bad[] = {ok, ok, ok, ok};
    bad[0].now = -1, bad[1].blacklist_duration = -1, bad[2].now = INT64_MAX - 6, bad[3].flags = 2;
    for (auto& b : bad) wrong += cn::scalars_error(b) == nullptr;
    const cn::Round edge = {INT64_MAX - 7, 7, 0, 0};
    wrong += cn::scalars_error(edge) != nullptr;
    wrong += cn::sweep_error(0, 0, 0) != nullptr || !cn::sweep_error(-1, 0, 0) || !cn::sweep_error(0, -1, 0) || !cn::sweep_error(0, 0, -1);
    const cn::Torrent T = {65, 64, cn::kTorrentComplete, 0, 1, 2, 3};
    wrong += cn::torrent_error(T) != nullptr;
    cn::Torrent worse[] = {T, T, T, T, T, T, T, T};
    worse[0].n_peers = 1u << 30, worse[1].self_peer = 65, worse[2].self_peer = cn::kNone - 1, worse[3].flags = 2;
    worse[4].reserved = 1, worse[5].bits_off = 1ull << 48, worse[6].peer_off = 1ull << 48, worse[7].close_off = 1ull << 48;
    for (auto& t : worse) wrong += cn::torrent_error(t) == nullptr;
    bool range = false;
    const cn::Lists L = {0, 2, 0, 1, 0, 2};
    wrong += cn::lists_shape_error(L, &range) != nullptr || range;
    cn::Lists big = L;
    big.n_dial = 1ull << 32;
    wrong += cn::lists_shape_error(big, &range) == nullptr || !range;
    big = L, big.in_off = 1ull << 48;
    wrong += cn::lists_shape_error(big, &range) == nullptr || range;
    cn::Transition tr[2] = {{3, cn::kClosed}, {64, cn::kEstablished}};
    cn::Incoming in[1] = {{64, 0, 5}};
    uint32_t dial[2] = {0, 64};
    uint64_t at = 0;
    wrong += cn::lists_error(T, L, tr, in, dial, 7, &at) != nullptr;
    wrong += cn::lists_error(T, L, tr, in, dial, 6, &at) == nullptr;  // the row ends one word past the array
    tr[1].peer = 3;
    wrong += cn::lists_error(T, L, tr, in, dial, 7, &at) == nullptr || at != 1;
    tr[1] = {65, 0};
    wrong += cn::lists_error(T, L, tr, in, dial, 7, &at) == nullptr;
    tr[1] = {64, 4};
    wrong += cn::lists_error(T, L, tr, in, dial, 7, &at) == nullptr;
    tr[1] = {64, 0}, in[0].peer = 65;
    wrong += cn::lists_error(T, L, tr, in, dial, 7, &at) == nullptr;
    in[0] = {0, 1, cn::kNoRow};
    wrong += cn::lists_error(T, L, tr, in, dial, 0, &at) == nullptr;
    in[0].reserved = 0, dial[1] = 65;
    wrong += cn::lists_error(T, L, tr, in, dial, 0, &at) == nullptr || at != 1;
    wrong += cn::live_bits(65, 0) != ~0ull || cn::live_bits(65, 1) != 1 || cn::live_bits(64, 0) != ~0ull;
    wrong += cn::blacklisted(5, 5) || !cn::blacklisted(6, 5);
    wrong += cn::preempts(900, 0, 0, 1000, 100, 500) || !cn::preempts(899, 0, 0, 1000, 100, 500) ||
             cn::preempts(500, 1000, 0, 1000, 100, 500) || !cn::preempts(499, 0, 1000, 1000, 100, 500);
    return wrong;
}

int main() {
    int mismatches = check_refusals(), cases = 0;
    const uint64_t lens[] = {0, 1, 63, 64, 65, 129};
    const uint32_t caps[] = {0, 1, 5, 40, 64, 65, 300}, limits[] = {0, 2, 10, 50};
    int k = 0;
    for (uint32_t P : {1u, 2u, 63u, 64u, 65u, 127u, 128u, 129u, 300u, 4096u, 4097u})
        for (int a = 0; a < 6; ++a, ++k) {
            mismatches += check_torrent(P, lens[a], lens[(a + 2) % 6], lens[(a + 4) % 6], caps[k % 7],
                                        k % 11 == 10 ? cn::kTorrentComplete : 0, k % 5 == 4 ? cn::kDisableBlacklist : 0,
                                        limits[k % 4], cases);
        }
    for (uint32_t P : {1u, 63u, 64u, 65u, 257u, 4097u}) mismatches += check_sweep(P, cases);
    printf("conn_math: %d cases, %d mismatches\n", cases, mismatches);
    return mismatches != 0;
}
