// announce_math.hpp -- whom an announcing peer talks to (krk_announce_handout,
// krk_announce_round): the tracker's announce (tracker/trackerserver/announce.go:75-115) over a
// torrent's peer store kept as a bit matrix -- a ring of W peer-set windows, (member, complete) a
// window, over the torrent's P known peers.  UpdatePeer (tracker/peerstore/redis.go:126-153) sets
// two bits; GetPeers (:155-196) is up to W k-smallest selections under seeded keys, one a window in
// a seeded order, folded into a set of at most 64 peers; SortPeers
// (tracker/peerhandoutpolicy/peerhandoutpolicy.go:65-99) is a three-class ordering of at most
// 64 + 8 entries.  Bitsets are willf/bitset words (bitfield_math.hpp): peer i = bit i & 63 of word
// i >> 6; tail bits past P are ignored wherever a row is read.  The reference's random choices
// (ShuffleInt64s, SRANDMEMBER, Go map order, the unstable sort.Slice) are the keys below.
// Header-only and free of the runtime, so that tests/native/announce_round_main.cpp builds it
// stand-alone under AddressSanitizer and UndefinedBehaviorSanitizer; announce_round.hip computes
// the same handouts.
#pragma once
#include <stdint.h>

#include "piece_request_math.hpp"

namespace krk {
namespace an {

constexpr uint32_t kMaxWindows = 8;           // KRK_AN_MAX_WINDOWS
constexpr uint32_t kMaxOrigins = 8;           // KRK_AN_MAX_ORIGINS
constexpr uint32_t kMaxLimit = 64;            // KRK_AN_MAX_LIMIT
constexpr uint32_t kDefault = 0;              // KRK_AN_DEFAULT
constexpr uint32_t kCompleteness = 1;         // KRK_AN_COMPLETENESS
constexpr uint32_t kComplete = 1;             // KRK_AN_COMPLETE
constexpr uint32_t kNone = 0xFFFFFFFFu;       // KRK_AN_NONE
constexpr uint32_t kOrigin = 0x80000000u;     // KRK_AN_ORIGIN
constexpr uint32_t kCompleteBit = 0x40000000u;  // KRK_AN_COMPLETE_BIT
constexpr uint64_t kMaxPeers = 1ull << 30;    // P is below it: a peer's index leaves bits 30 and 31 free
constexpr uint32_t kMaxEntries = kMaxLimit + kMaxOrigins;

struct Torrent {  // krk_announce_torrent
    uint64_t n_peers;
    uint32_t n_windows, cur_row, n_origins, reserved;
    uint64_t bits_off;
};
struct Announce {  // krk_announce
    uint32_t torrent, peer, flags, source;
    uint64_t seed;
};

KRK_PR_HD inline uint32_t wkey(uint64_t seed, uint32_t w) {
    return (uint32_t)(pr::splitmix64(seed ^ ((uint64_t)(w + 1) << 32 | 0xFFFFFFFFu)) >> 32);
}
KRK_PR_HD inline uint32_t pkey(uint64_t seed, uint32_t w, uint32_t i) {
    return (uint32_t)(pr::splitmix64(seed ^ ((uint64_t)(w + 1) << 32 | i)) >> 32);
}
KRK_PR_HD inline uint32_t okey(uint64_t seed, uint32_t c) { return (uint32_t)(pr::splitmix64(seed ^ c) >> 32); }
// completenessAssignmentPolicy.assignPriority (completeness_policy.go:28-36) / the default's 0.
KRK_PR_HD inline uint32_t priority(uint32_t policy, bool origin, bool complete) {
    return policy != kCompleteness ? 0u : origin ? 1u : complete ? 0u : 2u;
}
// The bits of word w that are peers of a torrent of n.
KRK_PR_HD inline uint64_t live_bits(uint64_t n, uint64_t w) {
    return n - w * 64 >= 64 ? ~0ull : (1ull << (n - w * 64)) - 1;
}
// First word of ring row `row`'s member row; its complete row follows at + words(P).
KRK_PR_HD inline uint64_t row_off(uint64_t wp, uint32_t row) { return 2 * (uint64_t)row * wp; }
KRK_PR_HD inline uint32_t ring_row(uint32_t cur_row, uint32_t w, uint32_t n_windows) { return (cur_row + w) % n_windows; }

// What is wrong with a torrent / an announce / the round's scalars, or nullptr.
inline const char* torrent_error(const Torrent& t) {
    if (t.n_peers >= kMaxPeers) return "2^30 peers or more";
    if (t.n_windows < 1 || t.n_windows > kMaxWindows) return "a window count outside [1, 8]";
    if (t.cur_row >= t.n_windows) return "cur_row is no ring row";
    if (t.n_origins > kMaxOrigins) return "more than 8 origins";
    if (t.reserved) return "reserved is not 0";
    if (t.bits_off >= (1ull << 48)) return "an offset of 2^48 or more";
    return nullptr;
}
inline const char* announce_error(const Announce& a, const Torrent* torrents, uint64_t n_torrents) {
    if (a.torrent >= n_torrents) return "a torrent past the last";
    if (a.peer >= torrents[a.torrent].n_peers) return "a peer past the torrent's last";
    if (a.source >= torrents[a.torrent].n_peers && a.source != kNone)
        return "a source that is neither one of the torrent's peers nor 0xFFFFFFFF";
    if (a.flags & ~kComplete) return "an unknown flag bit";
    return nullptr;
}
inline const char* scalars_error(uint32_t limit, uint32_t policy) {
    if (limit < 1 || limit > kMaxLimit) return "a limit outside [1, 64]";
    if (policy > kCompleteness) return "an unknown policy";
    return nullptr;
}

// UpdatePeer: rows = the torrent's first word.
inline void update(uint64_t* rows, const Torrent& t, const Announce& a) {
    const uint64_t wp = pr::words(t.n_peers);
    uint64_t* member = rows + row_off(wp, ring_row(t.cur_row, 0, t.n_windows));
    const uint64_t b = 1ull << (a.peer & 63);
    member[a.peer >> 6] |= b;
    if (a.flags & kComplete) member[wp + (a.peer >> 6)] |= b;
}

// The min(k, |member|) peers of one window row with the smallest (pkey(w, i), i), ascending in that
// pair, into out (k <= kMaxLimit entries); returns how many.
inline uint32_t sample(const uint64_t* member, uint64_t n, uint32_t k, uint64_t seed, uint32_t w, uint32_t* out) {
    uint64_t best[kMaxLimit];
    uint32_t m = 0;
    if (!k || k > kMaxLimit) return 0;
    for (uint64_t x = 0; x * 64 < n; ++x)
        for (uint64_t c = member[x] & live_bits(n, x); c; c &= c - 1) {
            const uint32_t i = (uint32_t)(x * 64 + (uint64_t)__builtin_ctzll(c));
            const uint64_t pk = (uint64_t)pkey(seed, w, i) << 32 | i;
            if (m == k) {
                if (pk > best[m - 1]) continue;
                --m;  // the largest leaves
            }
            uint32_t j = m;
            for (; j && best[j - 1] > pk; --j) best[j] = best[j - 1];
            best[j] = pk;
            ++m;
        }
    for (uint32_t j = 0; j < m; ++j) out[j] = (uint32_t)best[j];
    return m;
}

// One announce's handout over the torrent's rows: out has limit + kMaxOrigins entries, every one
// stored; labels has three.  Returns n_out.  The announce and the torrent are valid.
inline uint32_t handout(const uint64_t* rows, const Torrent& t, const Announce& a, uint32_t limit, uint32_t policy,
                        uint32_t* out, uint32_t* labels) {
    const uint32_t cap = limit + kMaxOrigins;
    labels[0] = labels[1] = labels[2] = 0;
    for (uint32_t j = 0; j < cap; ++j) out[j] = kNone;
    if (a.flags & kComplete) return 0;
    const uint64_t wp = pr::words(t.n_peers);
    uint32_t order[kMaxWindows];  // the windows in ascending (wkey(w), w)
    for (uint32_t w = 0; w < t.n_windows; ++w) {
        const uint64_t k = (uint64_t)wkey(a.seed, w) << 32 | w;
        uint32_t j = w;
        for (; j && ((uint64_t)wkey(a.seed, order[j - 1]) << 32 | order[j - 1]) > k; --j) order[j] = order[j - 1];
        order[j] = w;
    }
    uint32_t sel[kMaxLimit], n_sel = 0;
    bool complete[kMaxLimit];
    for (uint32_t v = 0; v < t.n_windows && n_sel < limit; ++v) {
        const uint32_t w = order[v];
        const uint64_t* member = rows + row_off(wp, ring_row(t.cur_row, w, t.n_windows));
        uint32_t got[kMaxLimit];
        const uint32_t m = sample(member, t.n_peers, limit - n_sel, a.seed, w, got);
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t i = got[j];
            const bool c = (member[wp + (i >> 6)] >> (i & 63)) & 1;
            uint32_t s = 0;
            while (s < n_sel && sel[s] != i) ++s;
            if (s == n_sel) {
                sel[n_sel] = i;
                complete[n_sel++] = c;
            } else if (c) {
                complete[s] = true;
            }
        }
    }
    // (priority << 32 | okey, c) ascending: an insertion sort of at most 72 entries
    uint64_t key[kMaxEntries];
    uint32_t val[kMaxEntries], n = 0;
    auto put = [&](uint32_t c, bool origin, bool comp) {
        const uint32_t p = priority(policy, origin, comp);
        const uint64_t k = (uint64_t)p << 32 | okey(a.seed, c);
        uint32_t j = n;
        for (; j && (key[j - 1] > k || (key[j - 1] == k && (val[j - 1] & ~kCompleteBit) > c)); --j)
            key[j] = key[j - 1], val[j] = val[j - 1];
        key[j] = k;
        val[j] = c | (comp && !origin ? kCompleteBit : 0);
        ++n;
        ++labels[p];
    };
    for (uint32_t s = 0; s < n_sel; ++s)
        if (sel[s] != a.source) put(sel[s], false, complete[s]);
    for (uint32_t o = 0; o < t.n_origins; ++o) put(kOrigin | o, true, true);
    for (uint32_t j = 0; j < n; ++j) out[j] = val[j];
    return n;
}

}  // namespace an
}  // namespace krk
