// request_table_abi.cpp -- request table rounds: the piece request tables of a batch of torrents
// (piecerequest.Manager's requests / requestsByPeer, piecerequest/manager.go) maintained beside
// the rows of a request round.  The host form (krk_request_table_round: request_table_math.hpp on
// the calling thread, no device) and the device form (krk_request_table_round_dev,
// request_table.hip computing the same state and outputs).
#include "request_table_math.hpp"
#include "runtime.hpp"

using namespace krk;

static_assert(rt::kMaxEntries == KRK_RT_MAX_ENTRIES && kRtMaxEntries == KRK_RT_MAX_ENTRIES,
              "request_table_math.hpp, kernels.hpp and kraken_hip.h name the same value");
static_assert(sizeof(rt::Entry) == sizeof(krk_request_entry) && sizeof(rt::Entry) == 24 &&
                  offsetof(rt::Entry, piece) == offsetof(krk_request_entry, piece) &&
                  offsetof(rt::Entry, peer) == offsetof(krk_request_entry, peer) &&
                  offsetof(rt::Entry, status) == offsetof(krk_request_entry, status) &&
                  offsetof(rt::Entry, sent_at) == offsetof(krk_request_entry, sent_at),
              "rt::Entry is krk_request_entry");
static_assert(sizeof(rt::Pair) == sizeof(krk_request_pair) && offsetof(rt::Pair, peer) == offsetof(krk_request_pair, peer),
              "rt::Pair is krk_request_pair");
static_assert(sizeof(rs::Failed) == sizeof(krk_failed_request), "rs::Failed is krk_failed_request");

namespace {

constexpr uint64_t kMaxOff = 1ull << 48;  // an offset past it is an error, and no sum below overflows

// What a round touches of each array, in elements (0 when nothing is), and the lists' lengths added up.
struct Extent {
    uint64_t bits = 0, peers = 0, entries = 0;
    uint64_t arrived = 0, gone = 0, marks = 0, holds = 0, records = 0;          // extents of the callers' arrays
    uint64_t n_arrived = 0, n_gone = 0, n_marks = 0, n_holds = 0, n_records = 0;  // sums
};

rt::Lists lists_of(const krk_table_torrent& B, const uint32_t* arrived, const uint32_t* gone,
                   const krk_failed_request* marks, const krk_request_pair* holds, const krk_request_pair* records) {
    return {B.n_arrived ? arrived + B.arrived_off : nullptr,
            B.n_gone ? gone + B.gone_off : nullptr,
            B.n_marks ? reinterpret_cast<const rs::Failed*>(marks) + B.mark_off : nullptr,
            B.n_holds ? reinterpret_cast<const rt::Pair*>(holds) + B.hold_off : nullptr,
            B.n_records ? reinterpret_cast<const rt::Pair*>(records) + B.record_off : nullptr,
            (uint32_t)B.n_arrived, (uint32_t)B.n_gone, (uint32_t)B.n_marks, (uint32_t)B.n_holds, (uint32_t)B.n_records};
}

// The checks both forms share, the lists included; *x the batch's extents.
int check_round(const char* who, const krk_request_torrent* t, const krk_table_torrent* b, uint64_t n,
                const uint32_t* arrived, const uint32_t* gone, const krk_failed_request* marks,
                const krk_request_pair* holds, const krk_request_pair* records, const rt::Round& round, Extent* x) {
    const char* why = rt::round_error(round);
    KRK_CHECK(!why, KRK_EINVAL, "%s: %s", who, why);
    KRK_CHECK(!n || (t && b), KRK_EINVAL, "%s: torrents or tables is NULL", who);
    for (uint64_t k = 0; k < n; ++k) {
        const unsigned long long kk = k;
        KRK_CHECK(t[k].n_pieces < (1ull << 32), KRK_EINVAL, "%s: torrent %llu has %llu pieces (2^32 or more)", who, kk,
                  (unsigned long long)t[k].n_pieces);
        KRK_CHECK(rs::flags_ok(t[k].flags), KRK_EINVAL, "%s: torrent %llu: unknown flag bit: %#x", who, kk, t[k].flags);
        KRK_CHECK(b[k].cap <= rt::kMaxEntries, KRK_EINVAL, "%s: torrent %llu: a table of %u entries (more than %u)", who, kk,
                  b[k].cap, rt::kMaxEntries);
        KRK_CHECK(!b[k].reserved, KRK_EINVAL, "%s: torrent %llu: a non-zero reserved field", who, kk);
        KRK_CHECK(t[k].bits_off < kMaxOff && t[k].peer_off < kMaxOff && b[k].entry_off < kMaxOff &&
                      b[k].arrived_off < kMaxOff && b[k].gone_off < kMaxOff && b[k].mark_off < kMaxOff &&
                      b[k].hold_off < kMaxOff && b[k].record_off < kMaxOff,
                  KRK_EINVAL, "%s: torrent %llu: an offset of 2^48 or more", who, kk);
        KRK_CHECK((b[k].n_arrived | b[k].n_gone | b[k].n_marks | b[k].n_holds | b[k].n_records) < (1ull << 32), KRK_EINVAL,
                  "%s: torrent %llu: a list of 2^32 entries or more", who, kk);
        const uint64_t W = pr::words(t[k].n_pieces);
        if (W) x->bits = std::max(x->bits, t[k].bits_off + (1 + 2 * (uint64_t)t[k].n_peers) * W);
        if (t[k].n_peers) x->peers = std::max(x->peers, t[k].peer_off + t[k].n_peers);
        if (b[k].cap) x->entries = std::max(x->entries, b[k].entry_off + b[k].cap);
        if (b[k].n_arrived) x->arrived = std::max(x->arrived, b[k].arrived_off + b[k].n_arrived);
        if (b[k].n_gone) x->gone = std::max(x->gone, b[k].gone_off + b[k].n_gone);
        if (b[k].n_marks) x->marks = std::max(x->marks, b[k].mark_off + b[k].n_marks);
        if (b[k].n_holds) x->holds = std::max(x->holds, b[k].hold_off + b[k].n_holds);
        if (b[k].n_records) x->records = std::max(x->records, b[k].record_off + b[k].n_records);
        x->n_arrived += b[k].n_arrived, x->n_gone += b[k].n_gone, x->n_marks += b[k].n_marks;
        x->n_holds += b[k].n_holds, x->n_records += b[k].n_records;
    }
    KRK_CHECK((arrived || !x->arrived) && (gone || !x->gone) && (marks || !x->marks) && (holds || !x->holds) &&
                  (records || !x->records),
              KRK_EINVAL, "%s: a list is NULL", who);
    for (uint64_t k = 0; k < n; ++k) {
        uint64_t at = 0;
        why = rt::lists_error(lists_of(b[k], arrived, gone, marks, holds, records), t[k].n_pieces, t[k].n_peers, &at);
        KRK_CHECK(!why, KRK_EINVAL, "%s: torrent %llu, element %llu: %s", who, (unsigned long long)k, (unsigned long long)at,
                  why);
    }
    return KRK_OK;
}

// The NULL rules of the arrays both forms share.
bool nulls_ok(const Extent& x, uint64_t n, const void* bits, const void* entries, const void* n_entries, const void* picks,
              const void* n_picked, const void* quota, const void* failed, const void* n_failed, const void* n_dropped) {
    return (bits || !x.bits) && (entries || !x.entries) && (!n || (n_entries && n_dropped)) && (quota || !x.peers) &&
           !picks == !n_picked && !failed == !n_failed;
}

}  // namespace

extern "C" {

int krk_request_table_round(const krk_request_torrent* torrents, const krk_table_torrent* tables, uint64_t n_torrents,
                            uint64_t* bits, krk_request_entry* entries, uint32_t* n_entries, const uint32_t* arrived,
                            const uint32_t* gone, const krk_failed_request* marks, const krk_request_pair* holds,
                            const krk_request_pair* records, const uint32_t* picks, const uint32_t* n_picked,
                            int64_t now, int64_t timeout, uint32_t limit, int32_t* quota_out,
                            krk_failed_request* failed_out, uint32_t* n_failed_out, uint32_t* n_dropped_out) {
    const rt::Round round{now, timeout, limit};
    Extent x;
    int r = check_round("request_table_round", torrents, tables, n_torrents, arrived, gone, marks, holds, records, round, &x);
    if (r) return r;
    KRK_CHECK(nulls_ok(x, n_torrents, bits, entries, n_entries, picks, n_picked, quota_out, failed_out, n_failed_out,
                       n_dropped_out),
              KRK_EINVAL, "request_table_round: null argument");
    for (uint64_t k = 0; k < n_torrents; ++k)
        KRK_CHECK(n_entries[k] <= tables[k].cap, KRK_EINVAL, "request_table_round: torrent %llu: %u entries in a table of %u",
                  (unsigned long long)k, n_entries[k], tables[k].cap);
    std::vector<uint64_t> keys(rt::kMaxEntries);
    for (uint64_t k = 0; k < n_torrents; ++k) {
        const krk_request_torrent& T = torrents[k];
        const krk_table_torrent& B = tables[k];
        rt::round_torrent(x.bits ? bits + T.bits_off : nullptr, T.n_pieces, T.n_peers, T.flags,
                          reinterpret_cast<rt::Entry*>(entries) + B.entry_off, n_entries + k, B.cap,
                          lists_of(B, arrived, gone, marks, holds, records), picks ? picks + T.peer_off * limit : nullptr,
                          picks ? n_picked + T.peer_off : nullptr, round, keys.data(),
                          T.n_peers ? quota_out + T.peer_off : nullptr,
                          failed_out ? reinterpret_cast<rs::Failed*>(failed_out) + B.entry_off : nullptr,
                          failed_out ? n_failed_out + k : nullptr, n_dropped_out + k);
    }
    return KRK_OK;
}

int krk_request_table_round_dev(const krk_request_torrent* torrents_host, const krk_table_torrent* tables_host,
                                uint64_t n_torrents, uint64_t* bits_dev, krk_request_entry* entries_dev,
                                uint32_t* n_entries_dev, const uint32_t* arrived_host, const uint32_t* gone_host,
                                const krk_failed_request* marks_host, const krk_request_pair* holds_host,
                                const krk_request_pair* records_host, const uint32_t* picks_dev,
                                const uint32_t* n_picked_dev, int64_t now, int64_t timeout, uint32_t limit,
                                int32_t* quota_out, krk_failed_request* failed_out, uint32_t* n_failed_out,
                                uint32_t* n_dropped_out, void* stream) {
    const rt::Round round{now, timeout, limit};
    Extent x;
    int r = check_round("request_table_round_dev", torrents_host, tables_host, n_torrents, arrived_host, gone_host,
                        marks_host, holds_host, records_host, round, &x);
    if (r) return r;
    KRK_CHECK(nulls_ok(x, n_torrents, bits_dev, entries_dev, n_entries_dev, picks_dev, n_picked_dev, quota_out, failed_out,
                       n_failed_out, n_dropped_out),
              KRK_EINVAL, "request_table_round_dev: null argument");
    KRK_CHECK(n_torrents <= 0x7FFFFFFFull, KRK_ERANGE, "request_table_round_dev: %llu torrents in one call",
              (unsigned long long)n_torrents);
    if (!n_torrents) return KRK_OK;
    KRK_DEVICE(D);
    KRK_CHECK(!(((uintptr_t)bits_dev | (uintptr_t)entries_dev) & 7) &&
                  !(((uintptr_t)n_entries_dev | (uintptr_t)picks_dev | (uintptr_t)n_picked_dev | (uintptr_t)quota_out |
                     (uintptr_t)failed_out | (uintptr_t)n_failed_out | (uintptr_t)n_dropped_out) &
                    3),
              KRK_EINVAL, "request_table_round_dev: bits_dev and entries_dev must be 8-byte, the other arrays 4-byte aligned");
    KRK_CHECK((!x.bits || device_writable(bits_dev, 8 * x.bits)) &&
                  (!x.entries || (device_writable(entries_dev, sizeof(rt::Entry) * x.entries) &&
                                  (!failed_out || device_writable(failed_out, sizeof(rs::Failed) * x.entries)))) &&
                  (!x.peers || (device_writable(quota_out, 4 * x.peers) &&
                                (!picks_dev || (device_writable(picks_dev, 4 * x.peers * limit) &&
                                                device_writable(n_picked_dev, 4 * x.peers))))) &&
                  device_writable(n_entries_dev, 4 * n_torrents) && device_writable(n_dropped_out, 4 * n_torrents) &&
                  (!n_failed_out || device_writable(n_failed_out, 4 * n_torrents)),
              KRK_EINVAL,
              "request_table_round_dev: bits_dev, entries_dev, n_entries_dev, picks_dev, n_picked_dev and the outputs must "
              "be device memory or page-locked host memory");
    hipStream_t s = pick(D, stream);
    // One staged block: the torrents, then the five lists, each packed torrent after torrent.
    const size_t arrived_at = n_torrents * sizeof(RtTorrent), gone_at = arrived_at + 4 * x.n_arrived;
    const size_t mark_at = (gone_at + 4 * x.n_gone + 7) & ~size_t(7), hold_at = mark_at + sizeof(rs::Failed) * x.n_marks;
    const size_t record_at = (hold_at + sizeof(rt::Pair) * x.n_holds + 7) & ~size_t(7);
    std::vector<uint8_t> stage(record_at + sizeof(rt::Pair) * x.n_records);
    RtTorrent* tors = reinterpret_cast<RtTorrent*>(stage.data());
    uint64_t a = 0, g = 0, m = 0, h = 0, c = 0;
    for (uint64_t k = 0; k < n_torrents; ++k) {
        const krk_request_torrent& T = torrents_host[k];
        const krk_table_torrent& B = tables_host[k];
        tors[k] = {T.n_pieces, T.bits_off, T.peer_off, B.entry_off, a, g, m, h, c, (uint32_t)B.n_arrived, (uint32_t)B.n_gone,
                   (uint32_t)B.n_marks, (uint32_t)B.n_holds, (uint32_t)B.n_records, T.n_peers, T.flags, B.cap, 0};
        if (B.n_arrived) memcpy(stage.data() + arrived_at + 4 * a, arrived_host + B.arrived_off, 4 * B.n_arrived);
        if (B.n_gone) memcpy(stage.data() + gone_at + 4 * g, gone_host + B.gone_off, 4 * B.n_gone);
        if (B.n_marks) memcpy(stage.data() + mark_at + sizeof(rs::Failed) * m, marks_host + B.mark_off, sizeof(rs::Failed) * B.n_marks);
        if (B.n_holds) memcpy(stage.data() + hold_at + sizeof(rt::Pair) * h, holds_host + B.hold_off, sizeof(rt::Pair) * B.n_holds);
        if (B.n_records)
            memcpy(stage.data() + record_at + sizeof(rt::Pair) * c, records_host + B.record_off, sizeof(rt::Pair) * B.n_records);
        a += B.n_arrived, g += B.n_gone, m += B.n_marks, h += B.n_holds, c += B.n_records;
    }
    void* d_stage = nullptr;  // copied into the library's pinned staging before this returns
    r = upload(D, stage.data(), stage.size(), &d_stage, s);
    if (r) return r;
    const uint8_t* ds = static_cast<const uint8_t*>(d_stage);
    const hipError_t e = timed(K_REQTABLE, s, [&] {
        return launch_request_table(reinterpret_cast<const RtTorrent*>(ds), n_torrents,
                                    reinterpret_cast<const uint32_t*>(ds + arrived_at),
                                    reinterpret_cast<const uint32_t*>(ds + gone_at),
                                    reinterpret_cast<const rs::Failed*>(ds + mark_at),
                                    reinterpret_cast<const rt::Pair*>(ds + hold_at),
                                    reinterpret_cast<const rt::Pair*>(ds + record_at), picks_dev, n_picked_dev, round, bits_dev,
                                    reinterpret_cast<rt::Entry*>(entries_dev), n_entries_dev, quota_out,
                                    reinterpret_cast<rs::Failed*>(failed_out), n_failed_out, n_dropped_out, s);
    });
    scratch_free(D, d_stage, s);
    KRK_CHECK(e == hipSuccess, KRK_EHIP, "request_table launch: %s", launch_error_text(e));
    return KRK_OK;
}

int krk_request_table_geometry(uint64_t* chunk, uint64_t* tile) {
    KRK_CHECK(chunk && tile, KRK_EINVAL, "request_table_geometry: null argument");
    *chunk = kRtChunk;
    *tile = kRtTile;
    return KRK_OK;
}

}  // extern "C"
