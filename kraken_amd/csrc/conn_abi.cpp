// conn_abi.cpp -- connection rounds: connstate.State (lib/torrent/scheduler/connstate/state.go)
// and the scheduler events that drive it (lib/torrent/scheduler/events.go:125-285, :369-392) for a
// batch of torrents over bit rows.  The host forms (krk_conn_round, krk_conn_preempt:
// conn_math.hpp on the calling thread, no device) and the device forms (krk_conn_round_dev,
// krk_conn_preempt_dev: conn_round.hip computing the same state and outputs).
#include "conn_math.hpp"
#include "runtime.hpp"

using namespace krk;

static_assert(cn::kNone == KRK_CN_NONE && cn::kNoRow == KRK_CN_NO_ROW && cn::kTorrentComplete == KRK_CN_TORRENT_COMPLETE &&
                  cn::kDisableBlacklist == KRK_CN_DISABLE_BLACKLIST && cn::kEstablished == KRK_CN_ESTABLISHED &&
                  cn::kFailedIn == KRK_CN_FAILED_IN && cn::kFailedOut == KRK_CN_FAILED_OUT && cn::kClosed == KRK_CN_CLOSED &&
                  cn::kOk == KRK_CN_OK && cn::kFreed == KRK_CN_FREED && cn::kNoop == KRK_CN_NOOP &&
                  cn::kNotPending == KRK_CN_NOT_PENDING && cn::kBlacklistedNow == KRK_CN_BLACKLISTED_NOW &&
                  cn::kStillBlacklisted == KRK_CN_STILL_BLACKLISTED && cn::kAtCapacity == KRK_CN_AT_CAPACITY &&
                  cn::kAlreadyPending == KRK_CN_ALREADY_PENDING && cn::kAlreadyActive == KRK_CN_ALREADY_ACTIVE &&
                  cn::kTooManyMutual == KRK_CN_TOO_MANY_MUTUAL && cn::kSelf == KRK_CN_SELF &&
                  cn::kBlacklisted == KRK_CN_BLACKLISTED && cn::kTorrentIsComplete == KRK_CN_TORRENT_IS_COMPLETE,
              "conn_math.hpp and kraken_hip.h name the same values");
static_assert(sizeof(cn::Torrent) == sizeof(krk_conn_torrent) && offsetof(cn::Torrent, close_off) == offsetof(krk_conn_torrent, close_off) &&
                  sizeof(cn::Lists) == sizeof(krk_conn_lists) && offsetof(cn::Lists, n_dial) == offsetof(krk_conn_lists, n_dial) &&
                  sizeof(cn::Transition) == sizeof(krk_conn_transition) && sizeof(cn::Incoming) == sizeof(krk_conn_incoming) &&
                  offsetof(cn::Incoming, neigh_off) == offsetof(krk_conn_incoming, neigh_off),
              "the cn:: structs are the krk_conn_ structs: the same fields in the same order");

namespace {

// What a call touches of each array, in elements; 0 when nothing is.
struct Extent {
    uint64_t bits = 0, peers = 0, close = 0, trans = 0, in = 0, dial = 0;
    uint64_t n_trans = 0, n_in = 0, n_dial = 0;  // the lists' lengths added up
    bool rows = false;                           // some incoming entry names a neighbour row
};

const cn::Torrent* tors(const krk_conn_torrent* t) { return reinterpret_cast<const cn::Torrent*>(t); }
const cn::Lists* lsts(const krk_conn_lists* l) { return reinterpret_cast<const cn::Lists*>(l); }
const cn::Transition* trs(const krk_conn_transition* t) { return reinterpret_cast<const cn::Transition*>(t); }
const cn::Incoming* ins(const krk_conn_incoming* i) { return reinterpret_cast<const cn::Incoming*>(i); }

int check_torrents(const char* who, const krk_conn_torrent* t, uint64_t n, bool sweep, Extent* x) {
    KRK_CHECK(!n || t, KRK_EINVAL, "%s: torrents is NULL", who);
    for (uint64_t k = 0; k < n; ++k) {
        const char* why = cn::torrent_error(tors(t)[k]);
        KRK_CHECK(!why, KRK_EINVAL, "%s: torrent %llu: %s", who, (unsigned long long)k, why);
        const uint64_t wp = pr::words(t[k].n_peers);
        if (wp) x->bits = std::max(x->bits, t[k].bits_off + (sweep ? 1 : 2) * wp);
        if (wp) x->close = std::max(x->close, t[k].close_off + wp);
        if (t[k].n_peers) x->peers = std::max(x->peers, t[k].peer_off + t[k].n_peers);
    }
    return KRK_OK;
}

// The checks both forms of a round share, the lists included; *x the batch's extents.
int check_round(const char* who, const krk_conn_torrent* t, const krk_conn_lists* l, uint64_t n,
                const krk_conn_transition* tr, const krk_conn_incoming* in, const uint32_t* dial, const uint64_t* neighbors,
                uint64_t n_neighbor_words, const cn::Round& R, Extent* x) {
    const char* why = cn::scalars_error(R);
    KRK_CHECK(!why, KRK_EINVAL, "%s: %s", who, why);
    int r = check_torrents(who, t, n, false, x);
    if (r) return r;
    KRK_CHECK(!n || l, KRK_EINVAL, "%s: lists is NULL", who);
    for (uint64_t k = 0; k < n; ++k) {
        bool range = false;
        why = cn::lists_shape_error(lsts(l)[k], &range);
        KRK_CHECK(!why, range ? KRK_ERANGE : KRK_EINVAL, "%s: torrent %llu: %s", who, (unsigned long long)k, why);
        if (l[k].n_trans) x->trans = std::max(x->trans, l[k].trans_off + l[k].n_trans);
        if (l[k].n_in) x->in = std::max(x->in, l[k].in_off + l[k].n_in);
        if (l[k].n_dial) x->dial = std::max(x->dial, l[k].dial_off + l[k].n_dial);
        x->n_trans += l[k].n_trans, x->n_in += l[k].n_in, x->n_dial += l[k].n_dial;
    }
    KRK_CHECK((tr || !x->trans) && (in || !x->in) && (dial || !x->dial), KRK_EINVAL, "%s: a list is NULL", who);
    for (uint64_t k = 0; k < n; ++k) {
        uint64_t at = 0;
        why = cn::lists_error(tors(t)[k], lsts(l)[k], trs(tr), ins(in), dial, n_neighbor_words, &at);
        KRK_CHECK(!why, KRK_EINVAL, "%s: torrent %llu, entry %llu: %s", who, (unsigned long long)k, (unsigned long long)at, why);
        for (uint64_t j = 0; j < l[k].n_in && !x->rows; ++j)
            x->rows = in[l[k].in_off + j].neigh_off != cn::kNoRow && t[k].n_peers != 0;
    }
    KRK_CHECK(neighbors || !x->rows, KRK_EINVAL, "%s: neighbors is NULL", who);
    return KRK_OK;
}

}  // namespace

extern "C" {

int krk_conn_round(const krk_conn_torrent* torrents, const krk_conn_lists* lists, uint64_t n_torrents, uint64_t* bits,
                   int64_t* expiry, uint32_t* capacity, const krk_conn_transition* transitions,
                   const krk_conn_incoming* incoming, const uint32_t* dials, const uint64_t* neighbors,
                   uint64_t n_neighbor_words, int64_t now, int64_t blacklist_duration, uint32_t max_mutual, uint32_t flags,
                   uint32_t* trans_status_out, uint32_t* in_status_out, uint32_t* dial_status_out, uint32_t* n_admitted_out,
                   uint32_t* n_freed_out) {
    const cn::Round R = {now, blacklist_duration, max_mutual, flags};
    Extent x;
    int r = check_round("conn_round", torrents, lists, n_torrents, transitions, incoming, dials, neighbors, n_neighbor_words,
                        R, &x);
    if (r) return r;
    if (!n_torrents) return KRK_OK;
    KRK_CHECK((bits || !x.bits) && (expiry || !x.peers) && capacity && (trans_status_out || !x.trans) &&
                  (in_status_out || !x.in) && (dial_status_out || !x.dial) && n_admitted_out && n_freed_out,
              KRK_EINVAL, "conn_round: null argument");
    for (uint64_t k = 0; k < n_torrents; ++k)
        KRK_CHECK(capacity[k] < cn::kMaxCapacity, KRK_EINVAL, "conn_round: torrent %llu: a capacity of 2^31 or more",
                  (unsigned long long)k);
    for (uint64_t k = 0; k < n_torrents; ++k) {
        const cn::Torrent& T = tors(torrents)[k];
        const cn::Lists& L = lsts(lists)[k];
        cn::round_torrent(T, L, R, x.bits ? bits + T.bits_off : nullptr, x.peers ? expiry + T.peer_off : nullptr, capacity + k,
                          L.n_trans ? trs(transitions) + L.trans_off : nullptr, L.n_in ? ins(incoming) + L.in_off : nullptr,
                          L.n_dial ? dials + L.dial_off : nullptr, neighbors,
                          L.n_trans ? trans_status_out + L.trans_off : nullptr, L.n_in ? in_status_out + L.in_off : nullptr,
                          L.n_dial ? dial_status_out + L.dial_off : nullptr, n_admitted_out + 2 * k, n_freed_out + k);
    }
    return KRK_OK;
}

int krk_conn_round_dev(const krk_conn_torrent* torrents_host, const krk_conn_lists* lists_host, uint64_t n_torrents,
                       uint64_t* bits_dev, int64_t* expiry_dev, uint32_t* capacity_dev,
                       const krk_conn_transition* transitions_host, const krk_conn_incoming* incoming_host,
                       const uint32_t* dials_host, const uint64_t* neighbors_dev, uint64_t n_neighbor_words, int64_t now,
                       int64_t blacklist_duration, uint32_t max_mutual, uint32_t flags, uint32_t* trans_status_out,
                       uint32_t* in_status_out, uint32_t* dial_status_out, uint32_t* n_admitted_out, uint32_t* n_freed_out,
                       void* stream) {
    const cn::Round R = {now, blacklist_duration, max_mutual, flags};
    Extent x;
    int r = check_round("conn_round_dev", torrents_host, lists_host, n_torrents, transitions_host, incoming_host, dials_host,
                        neighbors_dev, n_neighbor_words, R, &x);
    if (r) return r;
    if (!n_torrents) return KRK_OK;
    KRK_CHECK((bits_dev || !x.bits) && (expiry_dev || !x.peers) && capacity_dev && (trans_status_out || !x.trans) &&
                  (in_status_out || !x.in) && (dial_status_out || !x.dial) && n_admitted_out && n_freed_out,
              KRK_EINVAL, "conn_round_dev: null argument");
    KRK_CHECK(n_torrents <= 0x7FFFFFFFull, KRK_ERANGE, "conn_round_dev: %llu torrents in one call",
              (unsigned long long)n_torrents);
    KRK_DEVICE(D);
    KRK_CHECK(!((uintptr_t)bits_dev & 7) && !((uintptr_t)expiry_dev & 7) && !((uintptr_t)neighbors_dev & 7) &&
                  !((uintptr_t)capacity_dev & 3) && !((uintptr_t)trans_status_out & 3) && !((uintptr_t)in_status_out & 3) &&
                  !((uintptr_t)dial_status_out & 3) && !((uintptr_t)n_admitted_out & 3) && !((uintptr_t)n_freed_out & 3),
              KRK_EINVAL,
              "conn_round_dev: bits_dev, expiry_dev and neighbors_dev must be 8-byte, capacity_dev and the outputs 4-byte "
              "aligned");
    KRK_CHECK((!x.bits || device_writable(bits_dev, 8 * x.bits)) && (!x.peers || device_writable(expiry_dev, 8 * x.peers)) &&
                  device_writable(capacity_dev, 4 * n_torrents) &&
                  (!x.rows || device_writable(neighbors_dev, 8 * n_neighbor_words)) &&
                  (!x.trans || device_writable(trans_status_out, 4 * x.trans)) &&
                  (!x.in || device_writable(in_status_out, 4 * x.in)) &&
                  (!x.dial || device_writable(dial_status_out, 4 * x.dial)) &&
                  device_writable(n_admitted_out, 8 * n_torrents) && device_writable(n_freed_out, 4 * n_torrents),
              KRK_EINVAL,
              "conn_round_dev: bits_dev, expiry_dev, capacity_dev, neighbors_dev and the outputs must be device memory or "
              "page-locked host memory");
    hipStream_t s = pick(D, stream);
    // One staged block: the torrents, then the lists packed torrent after torrent -- the incoming
    // handshakes (16 bytes an entry), the transitions (8), the dials (4).
    const size_t in_at = n_torrents * sizeof(CnTorrent), tr_at = in_at + x.n_in * sizeof(cn::Incoming),
                 dial_at = tr_at + x.n_trans * sizeof(cn::Transition);
    std::vector<uint8_t> stage(dial_at + x.n_dial * sizeof(uint32_t));
    CnTorrent* ct = reinterpret_cast<CnTorrent*>(stage.data());
    cn::Incoming* s_in = reinterpret_cast<cn::Incoming*>(stage.data() + in_at);
    cn::Transition* s_tr = reinterpret_cast<cn::Transition*>(stage.data() + tr_at);
    uint32_t* s_dial = reinterpret_cast<uint32_t*>(stage.data() + dial_at);
    uint64_t a_in = 0, a_tr = 0, a_dial = 0;
    for (uint64_t k = 0; k < n_torrents; ++k) {
        const krk_conn_torrent& T = torrents_host[k];
        const krk_conn_lists& L = lists_host[k];
        ct[k] = {T.bits_off, T.peer_off, a_tr, L.trans_off, L.n_trans, a_in, L.in_off, L.n_in, a_dial, L.dial_off, L.n_dial,
                 T.n_peers,  T.self_peer, T.flags, 0, 0};
        if (L.n_trans) memcpy(s_tr + a_tr, transitions_host + L.trans_off, L.n_trans * sizeof(cn::Transition));
        if (L.n_in) memcpy(s_in + a_in, incoming_host + L.in_off, L.n_in * sizeof(cn::Incoming));
        if (L.n_dial) memcpy(s_dial + a_dial, dials_host + L.dial_off, L.n_dial * sizeof(uint32_t));
        a_tr += L.n_trans, a_in += L.n_in, a_dial += L.n_dial;
    }
    void* d_stage = nullptr;  // copied into the library's pinned staging before this returns
    r = upload(D, stage.data(), stage.size(), &d_stage, s);
    if (r) return r;
    const uint8_t* base = static_cast<const uint8_t*>(d_stage);
    const hipError_t e = timed(K_CONNROUND, s, [&] {
        return launch_conn_round(static_cast<const CnTorrent*>(d_stage), n_torrents,
                                 reinterpret_cast<const cn::Transition*>(base + tr_at),
                                 reinterpret_cast<const cn::Incoming*>(base + in_at),
                                 reinterpret_cast<const uint32_t*>(base + dial_at), neighbors_dev, bits_dev, expiry_dev,
                                 capacity_dev, R, trans_status_out, in_status_out, dial_status_out, n_admitted_out,
                                 n_freed_out, s);
    });
    scratch_free(D, d_stage, s);
    KRK_CHECK(e == hipSuccess, KRK_EHIP, "conn_round launch: %s", launch_error_text(e));
    return KRK_OK;
}

int krk_conn_preempt(const krk_conn_torrent* torrents, uint64_t n_torrents, const uint64_t* bits, const int64_t* created,
                     const int64_t* received, const int64_t* sent, int64_t now, int64_t conn_tti, int64_t conn_ttl,
                     uint64_t* close_out, uint32_t* n_close_out) {
    const char* why = cn::sweep_error(now, conn_tti, conn_ttl);
    KRK_CHECK(!why, KRK_EINVAL, "conn_preempt: %s", why);
    Extent x;
    int r = check_torrents("conn_preempt", torrents, n_torrents, true, &x);
    if (r) return r;
    if (!n_torrents) return KRK_OK;
    KRK_CHECK(((bits && close_out) || !x.bits) && ((created && received && sent) || !x.peers) && n_close_out, KRK_EINVAL,
              "conn_preempt: null argument");
    for (uint64_t k = 0; k < n_torrents; ++k) {
        const krk_conn_torrent& T = torrents[k];
        n_close_out[k] = T.n_peers ? cn::preempt_torrent(T.n_peers, bits + T.bits_off, created + T.peer_off,
                                                         received + T.peer_off, sent + T.peer_off, now, conn_tti, conn_ttl,
                                                         close_out + T.close_off)
                                   : 0;
    }
    return KRK_OK;
}

int krk_conn_preempt_dev(const krk_conn_torrent* torrents_host, uint64_t n_torrents, const uint64_t* bits_dev,
                         const int64_t* created_dev, const int64_t* received_dev, const int64_t* sent_dev, int64_t now,
                         int64_t conn_tti, int64_t conn_ttl, uint64_t* close_out, uint32_t* n_close_out, void* stream) {
    const char* why = cn::sweep_error(now, conn_tti, conn_ttl);
    KRK_CHECK(!why, KRK_EINVAL, "conn_preempt_dev: %s", why);
    Extent x;
    int r = check_torrents("conn_preempt_dev", torrents_host, n_torrents, true, &x);
    if (r) return r;
    if (!n_torrents) return KRK_OK;
    KRK_CHECK(((bits_dev && close_out) || !x.bits) && ((created_dev && received_dev && sent_dev) || !x.peers) && n_close_out,
              KRK_EINVAL, "conn_preempt_dev: null argument");
    KRK_CHECK(n_torrents <= 0x7FFFFFFFull, KRK_ERANGE, "conn_preempt_dev: %llu torrents in one call",
              (unsigned long long)n_torrents);
    KRK_DEVICE(D);
    KRK_CHECK(!((uintptr_t)bits_dev & 7) && !((uintptr_t)created_dev & 7) && !((uintptr_t)received_dev & 7) &&
                  !((uintptr_t)sent_dev & 7) && !((uintptr_t)close_out & 7) && !((uintptr_t)n_close_out & 3),
              KRK_EINVAL, "conn_preempt_dev: the 64-bit arrays must be 8-byte, n_close_out 4-byte aligned");
    KRK_CHECK((!x.bits || (device_writable(bits_dev, 8 * x.bits) && device_writable(close_out, 8 * x.close))) &&
                  (!x.peers || (device_writable(created_dev, 8 * x.peers) && device_writable(received_dev, 8 * x.peers) &&
                                device_writable(sent_dev, 8 * x.peers))) &&
                  device_writable(n_close_out, 4 * n_torrents),
              KRK_EINVAL, "conn_preempt_dev: the arrays must be device memory or page-locked host memory");
    hipStream_t s = pick(D, stream);
    std::vector<CnSweep> stage(n_torrents);
    for (uint64_t k = 0; k < n_torrents; ++k)
        stage[k] = {torrents_host[k].bits_off, torrents_host[k].peer_off, torrents_host[k].close_off, torrents_host[k].n_peers, 0};
    void* d_stage = nullptr;  // copied into the library's pinned staging before this returns
    r = upload(D, stage.data(), stage.size() * sizeof(CnSweep), &d_stage, s);
    if (r) return r;
    const hipError_t e = timed(K_CONNPREEMPT, s, [&] {
        return launch_conn_preempt(static_cast<const CnSweep*>(d_stage), n_torrents, bits_dev, created_dev, received_dev,
                                   sent_dev, now, conn_tti, conn_ttl, close_out, n_close_out, s);
    });
    scratch_free(D, d_stage, s);
    KRK_CHECK(e == hipSuccess, KRK_EHIP, "conn_preempt launch: %s", launch_error_text(e));
    return KRK_OK;
}

}  // extern "C"
