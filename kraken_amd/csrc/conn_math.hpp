// conn_math.hpp -- which connections a torrent opens, admits, frees and closes (krk_conn_round,
// krk_conn_preempt): connstate.State (lib/torrent/scheduler/connstate/state.go) and the scheduler
// events that drive it (lib/torrent/scheduler/events.go:125-285, :369-392) over bit rows.  The
// reference keeps `active`, `pending` and the blacklist as maps keyed by (peer, torrent); here a
// torrent's P known peers are indices, `active` and `pending` are two rows of words(P) words
// (bitfield_math.hpp's layout: peer i = bit i & 63 of word i >> 6), the blacklist is one expiry a
// peer (0: never blacklisted) and numMutualConns is popcount(neighbours & (active | pending)).
// Tail bits past P are ignored wherever a row is read and never set.
//
// One round runs three phases in a fixed order: the transitions (established, failed incoming,
// failed outgoing, closed), then the incoming handshakes in list order (AddPending with the
// remote's neighbours), then the dials in handout order (announceResultEvent.apply).
// Two deliberate differences from the reference.  Its event loop applies events in arrival
// order; a round applies frees first, then incoming, then dials -- a caller who needs another
// interleaving makes several calls, and a round with one non-empty list is exactly that event
// type.  Its dial loop breaks at ErrTorrentAtCapacity; here every remaining entry gets its
// status, and the resulting state is identical because capacity == 0 is AddPending's first check.
// Header-only and free of the runtime, so that tests/native/conn_round_main.cpp builds it
// stand-alone under AddressSanitizer and UndefinedBehaviorSanitizer; conn_round.hip computes the
// same rows, expiries, capacities and statuses.
#pragma once
#include <stdint.h>

#include "piece_request_math.hpp"

namespace krk {
namespace cn {

constexpr uint32_t kNone = 0xFFFFFFFFu;     // KRK_CN_NONE
constexpr uint64_t kNoRow = ~0ull;          // KRK_CN_NO_ROW
constexpr uint32_t kTorrentComplete = 1;    // KRK_CN_TORRENT_COMPLETE (a torrent's flags)
constexpr uint32_t kDisableBlacklist = 1;   // KRK_CN_DISABLE_BLACKLIST (a round's flags)
constexpr uint64_t kMaxPeers = 1ull << 30;  // P is below it
constexpr uint64_t kMaxOff = 1ull << 48;    // an offset is below it, so no sum of offsets overflows
constexpr uint32_t kMaxCapacity = 1u << 31;  // a capacity is below it, so capacity + frees does not wrap

// transition kinds
constexpr uint32_t kEstablished = 0, kFailedIn = 1, kFailedOut = 2, kClosed = 3;

// status bits
constexpr uint32_t kOk = 0x001, kFreed = 0x002, kNoop = 0x004, kNotPending = 0x008, kBlacklistedNow = 0x010,
                   kStillBlacklisted = 0x020, kAtCapacity = 0x040, kAlreadyPending = 0x080, kAlreadyActive = 0x100,
                   kTooManyMutual = 0x200, kSelf = 0x400, kBlacklisted = 0x800, kTorrentIsComplete = 0x1000;

struct Torrent {  // krk_conn_torrent
    uint32_t n_peers, self_peer, flags, reserved;
    uint64_t bits_off, peer_off, close_off;
};
struct Lists {  // krk_conn_lists
    uint64_t trans_off, n_trans, in_off, n_in, dial_off, n_dial;
};
struct Transition {  // krk_conn_transition
    uint32_t peer, kind;
};
struct Incoming {  // krk_conn_incoming
    uint32_t peer, reserved;
    uint64_t neigh_off;
};
struct Round {  // the scalars of a round
    int64_t now, blacklist_duration;
    uint32_t max_mutual, flags;
};

// The bits of word w that are peers of a torrent of n.
KRK_PR_HD inline uint64_t live_bits(uint64_t n, uint64_t w) { return n - w * 64 >= 64 ? ~0ull : (1ull << (n - w * 64)) - 1; }
// blacklistEntry.Blacklisted (state.go:46-52): time remains.
KRK_PR_HD inline bool blacklisted(int64_t expiry, int64_t now) { return expiry > now; }
// State.Blacklist (state.go:122-139) on one entry: the status bits it adds.
KRK_PR_HD inline uint32_t blacklist(int64_t* expiry, const Round& r) {
    if (r.flags & kDisableBlacklist) return 0;
    if (blacklisted(*expiry, r.now)) return kStillBlacklisted;
    *expiry = r.now + r.blacklist_duration;
    return kBlacklistedNow;
}
// The row a transition clears when its bit is set there: pending (false) or active (true).
KRK_PR_HD inline bool clears_active(uint32_t kind) { return kind == kClosed; }
// What a transition whose bit was set / was not set in the row it looks at reports, the blacklist aside.
KRK_PR_HD inline uint32_t transition_status(uint32_t kind, bool was_set) {
    if (kind == kEstablished) return was_set ? kOk : kNotPending;
    return was_set ? kOk | kFreed : kNoop;
}
KRK_PR_HD inline bool blacklists(uint32_t kind) { return kind == kFailedOut || kind == kClosed; }
// AddPending's checks after the mutual count (state.go:165-176), in its order; 0 admits.
KRK_PR_HD inline uint32_t add_pending_status(uint32_t cap, bool pending, bool active, uint64_t mutual, uint32_t max_mutual) {
    return cap == 0 ? kAtCapacity : pending ? kAlreadyPending : active ? kAlreadyActive : mutual > max_mutual ? kTooManyMutual : 0;
}
// preemptionTickEvent on one conn (events.go:378-391): idle or expired.  A negative time counts as 0 (never).
KRK_PR_HD inline bool preempts(int64_t created, int64_t received, int64_t sent, int64_t now, int64_t tti, int64_t ttl) {
    const int64_t c = created < 0 ? 0 : created, r = received < 0 ? 0 : received, s = sent < 0 ? 0 : sent;
    const int64_t last = c > r ? (c > s ? c : s) : (r > s ? r : s);
    return now - last > tti || now - c > ttl;
}

// What is wrong with a round's scalars / a torrent / a torrent's lists, or nullptr.
inline const char* scalars_error(const Round& r) {
    if (r.now < 0 || r.blacklist_duration < 0) return "a negative now or blacklist_duration";
    if (r.now > INT64_MAX - r.blacklist_duration) return "now + blacklist_duration past INT64_MAX";
    if (r.flags & ~kDisableBlacklist) return "an unknown round flag bit";
    return nullptr;
}
inline const char* sweep_error(int64_t now, int64_t tti, int64_t ttl) {
    if (now < 0 || tti < 0 || ttl < 0) return "a negative now, conn_tti or conn_ttl";
    return nullptr;
}
inline const char* torrent_error(const Torrent& t) {
    if (t.n_peers >= kMaxPeers) return "2^30 peers or more";
    if (t.self_peer >= t.n_peers && t.self_peer != kNone) return "a self_peer that is neither one of the torrent's peers nor 0xFFFFFFFF";
    if (t.flags & ~kTorrentComplete) return "an unknown torrent flag bit";
    if (t.reserved) return "reserved is not 0";
    if (t.bits_off >= kMaxOff || t.peer_off >= kMaxOff || t.close_off >= kMaxOff) return "an offset of 2^48 or more";
    return nullptr;
}
// *range: the list is 2^32 entries or more (KRK_ERANGE, not KRK_EINVAL).
inline const char* lists_shape_error(const Lists& l, bool* range) {
    *range = false;
    if (l.trans_off >= kMaxOff || l.in_off >= kMaxOff || l.dial_off >= kMaxOff) return "an offset of 2^48 or more";
    if (l.n_trans >= (1ull << 32) || l.n_in >= (1ull << 32) || l.n_dial >= (1ull << 32)) {
        *range = true;
        return "a list of 2^32 entries or more";
    }
    return nullptr;
}
inline const char* lists_error(const Torrent& t, const Lists& l, const Transition* tr, const Incoming* in, const uint32_t* dial,
                               uint64_t n_neighbor_words, uint64_t* at) {
    const uint64_t wp = pr::words(t.n_peers);
    for (uint64_t k = 0; k < l.n_trans; ++k) {
        *at = k;
        const Transition& e = tr[l.trans_off + k];
        if (e.peer >= t.n_peers) return "a transition of a peer past the torrent's last";
        if (e.kind > kClosed) return "an unknown transition kind";
        if (k && e.peer <= tr[l.trans_off + k - 1].peer) return "transitions that do not ascend strictly by peer";
    }
    for (uint64_t k = 0; k < l.n_in; ++k) {
        *at = k;
        const Incoming& e = in[l.in_off + k];
        if (e.peer >= t.n_peers) return "an incoming handshake of a peer past the torrent's last";
        if (e.reserved) return "an incoming handshake whose reserved is not 0";
        if (e.neigh_off != kNoRow && (e.neigh_off >= kMaxOff || e.neigh_off + wp > n_neighbor_words))
            return "a neighbour row past the end of neighbors";
    }
    for (uint64_t k = 0; k < l.n_dial; ++k) {
        *at = k;
        if (dial[l.dial_off + k] >= t.n_peers) return "a dial of a peer past the torrent's last";
    }
    return nullptr;
}

KRK_PR_HD inline bool bit(const uint64_t* row, uint32_t p) { return (row[p >> 6] >> (p & 63)) & 1; }

// One torrent's round.  rows: active then pending, words(P) words each; expiry: the torrent's P
// entries; *cap its remaining capacity (< 2^31); tr / in / dial and tr_st / in_st / dial_st: the
// torrent's own entries and their statuses.  The lists are valid (lists_error).  Every status is
// stored; admitted[0] the incoming handshakes admitted, admitted[1] the dials, *freed the
// capacity phase 1 gave back.
inline void round_torrent(const Torrent& t, const Lists& l, const Round& r, uint64_t* rows, int64_t* expiry, uint32_t* cap,
                          const Transition* tr, const Incoming* in, const uint32_t* dial, const uint64_t* neighbors,
                          uint32_t* tr_st, uint32_t* in_st, uint32_t* dial_st, uint32_t admitted[2], uint32_t* freed) {
    const uint64_t wp = pr::words(t.n_peers);
    uint64_t *active = rows, *pending = rows + wp;
    uint32_t c = *cap;
    *freed = 0;
    for (uint64_t k = 0; k < l.n_trans; ++k) {
        const uint32_t p = tr[k].peer, kind = tr[k].kind;
        const uint64_t b = 1ull << (p & 63);
        uint64_t* row = clears_active(kind) ? active : pending;
        const bool was = (row[p >> 6] & b) != 0;
        if (was) row[p >> 6] &= ~b;
        if (was && kind == kEstablished) active[p >> 6] |= b;
        uint32_t st = transition_status(kind, was);
        if (st & kFreed) ++c, ++*freed;
        if (blacklists(kind)) st |= blacklist(expiry + p, r);
        tr_st[k] = st;
    }
    admitted[0] = 0;
    for (uint64_t k = 0; k < l.n_in; ++k) {
        const uint32_t p = in[k].peer;
        uint64_t mutual = 0;
        if (in[k].neigh_off != kNoRow)
            for (uint64_t w = 0; w < wp; ++w)
                mutual += (uint64_t)__builtin_popcountll(neighbors[in[k].neigh_off + w] & (active[w] | pending[w]) &
                                                         live_bits(t.n_peers, w));
        const uint32_t st = add_pending_status(c, bit(pending, p), bit(active, p), mutual, r.max_mutual);
        if (!st) {
            pending[p >> 6] |= 1ull << (p & 63);
            --c;
            ++admitted[0];
        }
        in_st[k] = st ? st : kOk;
    }
    admitted[1] = 0;
    for (uint64_t k = 0; k < l.n_dial; ++k) {
        const uint32_t p = dial[k];
        uint32_t st;
        if (t.flags & kTorrentComplete) st = kTorrentIsComplete;
        else if (p == t.self_peer) st = kSelf;
        else if (blacklisted(expiry[p], r.now)) st = kBlacklisted;
        else st = add_pending_status(c, bit(pending, p), bit(active, p), 0, 0);
        if (!st) {
            pending[p >> 6] |= 1ull << (p & 63);
            --c;
            ++admitted[1];
            st = kOk;
        }
        dial_st[k] = st;
    }
    *cap = c;
}

// One torrent's preemption sweep: close[w] for every word of the row, the count returned.
inline uint32_t preempt_torrent(uint64_t n_peers, const uint64_t* active, const int64_t* created, const int64_t* received,
                                const int64_t* sent, int64_t now, int64_t tti, int64_t ttl, uint64_t* close) {
    uint32_t n = 0;
    for (uint64_t w = 0; w < pr::words(n_peers); ++w) {
        uint64_t out = 0;
        for (uint64_t p = w * 64; p < n_peers && p < w * 64 + 64; ++p)
            if (((active[w] >> (p & 63)) & 1) && preempts(created[p], received[p], sent[p], now, tti, ttl)) out |= 1ull << (p & 63);
        close[w] = out;
        n += (uint32_t)__builtin_popcountll(out);
    }
    return n;
}

}  // namespace cn
}  // namespace krk
