// peer_round_abi.cpp -- peer rounds: AddPeer from the handshake's wire bytes, handleComplete and
// the progress derived from the rows of a request round, for a batch of torrents.  The host form
// (krk_peer_round: peer_round_math.hpp on the calling thread, no device) and the device form
// (krk_peer_round_dev, peer_round.hip computing the same state and outputs).
#include "peer_round_math.hpp"
#include "runtime.hpp"

using namespace krk;

static_assert(sizeof(pe::Join) == sizeof(krk_peer_join) && sizeof(pe::Join) == 24 &&
                  offsetof(pe::Join, peer) == offsetof(krk_peer_join, peer) &&
                  offsetof(pe::Join, reserved) == offsetof(krk_peer_join, reserved) &&
                  offsetof(pe::Join, wire_off) == offsetof(krk_peer_join, wire_off) &&
                  offsetof(pe::Join, wire_len) == offsetof(krk_peer_join, wire_len),
              "pe::Join is krk_peer_join");
static_assert(sizeof(krk_peer_torrent) == 40, "krk_peer_torrent layout");
static_assert(pe::kDisableEndgame == KRK_PE_DISABLE_ENDGAME && pe::kTorrentComplete == KRK_PE_TORRENT_COMPLETE &&
                  pe::kEndgame == KRK_PE_ENDGAME && pe::kJoined == KRK_PE_JOINED && pe::kBadBitfield == KRK_PE_BAD_BITFIELD &&
                  pe::kSetFull == KRK_PE_SET_FULL && pe::kPeerComplete == KRK_PE_PEER_COMPLETE &&
                  pe::kClose == KRK_PE_CLOSE && pe::kNotify == KRK_PE_NOTIFY,
              "peer_round_math.hpp and kraken_hip.h name the same values");

namespace {

constexpr uint64_t kMaxOff = 1ull << 48;  // an offset past it is an error, and no sum below overflows

// What a round touches of each array, in elements (0 when nothing is), and the lists' lengths added up.
struct Extent {
    uint64_t bits = 0, peers = 0, live = 0, joins = 0, fulls = 0, wire = 0;  // extents of the callers' arrays
    uint64_t n_live = 0, n_joins = 0, n_fulls = 0, units = 0;                // sums
};

// The checks both forms share, the lists included; *x the batch's extents.
int check_round(const char* who, const krk_request_torrent* t, const krk_peer_torrent* b, uint64_t n, const uint64_t* live,
                const krk_peer_join* joins, const uint32_t* fulls, Extent* x) {
    KRK_CHECK(!n || (t && b), KRK_EINVAL, "%s: torrents or peer_torrents is NULL", who);
    for (uint64_t k = 0; k < n; ++k) {
        const unsigned long long kk = k;
        KRK_CHECK(t[k].n_pieces < (1ull << 32), KRK_EINVAL, "%s: torrent %llu has %llu pieces (2^32 or more)", who, kk,
                  (unsigned long long)t[k].n_pieces);
        KRK_CHECK(!(b[k].flags & ~pe::kDisableEndgame), KRK_EINVAL, "%s: torrent %llu: unknown flag bit: %#x", who, kk,
                  b[k].flags);
        KRK_CHECK(t[k].bits_off < kMaxOff && t[k].peer_off < kMaxOff && b[k].live_off < kMaxOff && b[k].join_off < kMaxOff &&
                      b[k].full_off < kMaxOff,
                  KRK_EINVAL, "%s: torrent %llu: an offset of 2^48 or more", who, kk);
        const uint64_t W = pr::words(t[k].n_pieces), P = t[k].n_peers, L = (P + 63) / 64;
        if (W) x->bits = std::max(x->bits, t[k].bits_off + (1 + 2 * P) * W);
        if (P) x->peers = std::max(x->peers, t[k].peer_off + P), x->live = std::max(x->live, b[k].live_off + L);
        if (b[k].n_joins) x->joins = std::max(x->joins, b[k].join_off + b[k].n_joins);
        if (b[k].n_fulls) x->fulls = std::max(x->fulls, b[k].full_off + b[k].n_fulls);
        x->n_live += L, x->n_joins += b[k].n_joins, x->n_fulls += b[k].n_fulls, x->units += 1 + P;
    }
    KRK_CHECK((live || !x->live) && (joins || !x->joins) && (fulls || !x->fulls), KRK_EINVAL, "%s: live or a list is NULL", who);
    for (uint64_t k = 0; k < n; ++k) {
        uint64_t at = 0;
        const pe::Join* j = b[k].n_joins ? reinterpret_cast<const pe::Join*>(joins) + b[k].join_off : nullptr;
        const char* why = pe::lists_error(j, b[k].n_joins, b[k].n_fulls ? fulls + b[k].full_off : nullptr, b[k].n_fulls,
                                          t[k].n_peers, &at);
        KRK_CHECK(!why, KRK_EINVAL, "%s: torrent %llu, element %llu: %s", who, (unsigned long long)k, (unsigned long long)at,
                  why);
        for (uint32_t e = 0; e < b[k].n_joins; ++e)
            if (j[e].wire_len) x->wire = std::max(x->wire, j[e].wire_off + j[e].wire_len);
    }
    return KRK_OK;
}

// The NULL rules of the arrays both forms share.
bool nulls_ok(const Extent& x, uint64_t n, const void* bits, const void* wire, const void* remaining, const void* tflags,
              const void* held, const void* wanted, const void* status) {
    return (bits || !x.bits) && (wire || !x.wire) && (!n || (remaining && tflags)) && (!x.peers || (held && wanted && status));
}

}  // namespace

extern "C" {

int krk_peer_round(const krk_request_torrent* torrents, const krk_peer_torrent* peer_torrents, uint64_t n_torrents,
                   uint64_t* bits, const uint64_t* live, const krk_peer_join* joins, const uint32_t* fulls,
                   const uint8_t* wire, uint32_t* remaining_out, uint32_t* torrent_flags_out, uint32_t* held_out,
                   uint32_t* wanted_out, uint32_t* status_out) {
    Extent x;
    int r = check_round("peer_round", torrents, peer_torrents, n_torrents, live, joins, fulls, &x);
    if (r) return r;
    KRK_CHECK(nulls_ok(x, n_torrents, bits, wire, remaining_out, torrent_flags_out, held_out, wanted_out, status_out),
              KRK_EINVAL, "peer_round: null argument");
    for (uint64_t k = 0; k < n_torrents; ++k) {
        const krk_request_torrent& T = torrents[k];
        const krk_peer_torrent& B = peer_torrents[k];
        const uint64_t P = T.n_peers;
        pe::round_torrent(x.bits ? bits + T.bits_off : nullptr, T.n_pieces, T.n_peers, P ? live + B.live_off : nullptr,
                          B.n_joins ? reinterpret_cast<const pe::Join*>(joins) + B.join_off : nullptr, B.n_joins,
                          B.n_fulls ? fulls + B.full_off : nullptr, B.n_fulls, wire, B.endgame_threshold, B.flags,
                          remaining_out + k, torrent_flags_out + k, P ? held_out + T.peer_off : nullptr,
                          P ? wanted_out + T.peer_off : nullptr, P ? status_out + T.peer_off : nullptr);
    }
    return KRK_OK;
}

int krk_peer_round_dev(const krk_request_torrent* torrents_host, const krk_peer_torrent* peer_torrents_host,
                       uint64_t n_torrents, uint64_t* bits_dev, const uint64_t* live_host,
                       const krk_peer_join* joins_host, const uint32_t* fulls_host, const uint8_t* wire_dev,
                       uint32_t* remaining_out, uint32_t* torrent_flags_out, uint32_t* held_out, uint32_t* wanted_out,
                       uint32_t* status_out, void* stream) {
    Extent x;
    int r = check_round("peer_round_dev", torrents_host, peer_torrents_host, n_torrents, live_host, joins_host, fulls_host, &x);
    if (r) return r;
    KRK_CHECK(nulls_ok(x, n_torrents, bits_dev, wire_dev, remaining_out, torrent_flags_out, held_out, wanted_out, status_out),
              KRK_EINVAL, "peer_round_dev: null argument");
    KRK_CHECK(n_torrents <= 0x7FFFFFFFull, KRK_ERANGE, "peer_round_dev: %llu torrents in one call",
              (unsigned long long)n_torrents);
    if (!n_torrents) return KRK_OK;
    KRK_DEVICE(D);
    KRK_CHECK(!((uintptr_t)bits_dev & 7) && !(((uintptr_t)remaining_out | (uintptr_t)torrent_flags_out | (uintptr_t)held_out |
                                                (uintptr_t)wanted_out | (uintptr_t)status_out) &
                                               3),
              KRK_EINVAL, "peer_round_dev: bits_dev must be 8-byte, the outputs 4-byte aligned");
    KRK_CHECK((!x.bits || device_writable(bits_dev, 8 * x.bits)) && (!x.wire || device_writable(wire_dev, x.wire)) &&
                  (!x.peers || (device_writable(held_out, 4 * x.peers) && device_writable(wanted_out, 4 * x.peers) &&
                                device_writable(status_out, 4 * x.peers))) &&
                  device_writable(remaining_out, 4 * n_torrents) && device_writable(torrent_flags_out, 4 * n_torrents),
              KRK_EINVAL,
              "peer_round_dev: bits_dev, wire_dev (every span of it) and the outputs must be device memory or page-locked "
              "host memory");
    hipStream_t s = pick(D, stream);
    // One staged block: the torrents, the live words, the joins, the fulls, each packed torrent after torrent.
    const size_t live_at = n_torrents * sizeof(PeTorrent), join_at = live_at + 8 * x.n_live;
    const size_t full_at = join_at + sizeof(pe::Join) * x.n_joins;
    std::vector<uint8_t> stage(full_at + 4 * x.n_fulls);
    PeTorrent* tors = reinterpret_cast<PeTorrent*>(stage.data());
    uint64_t u = 0, l = 0, j = 0, f = 0;
    for (uint64_t k = 0; k < n_torrents; ++k) {
        const krk_request_torrent& T = torrents_host[k];
        const krk_peer_torrent& B = peer_torrents_host[k];
        const uint64_t L = ((uint64_t)T.n_peers + 63) / 64;
        tors[k] = {u, T.n_pieces, T.bits_off, T.peer_off, l, j, f, T.n_peers, B.n_joins, B.n_fulls, B.endgame_threshold, B.flags, 0};
        if (L) memcpy(stage.data() + live_at + 8 * l, live_host + B.live_off, 8 * L);
        if (B.n_joins) memcpy(stage.data() + join_at + sizeof(pe::Join) * j, joins_host + B.join_off, sizeof(pe::Join) * B.n_joins);
        if (B.n_fulls) memcpy(stage.data() + full_at + 4 * f, fulls_host + B.full_off, 4 * (size_t)B.n_fulls);
        u += 1 + (uint64_t)T.n_peers, l += L, j += B.n_joins, f += B.n_fulls;
    }
    void* d_stage = nullptr;  // copied into the library's pinned staging before this returns
    r = upload(D, stage.data(), stage.size(), &d_stage, s);
    if (r) return r;
    const uint8_t* ds = static_cast<const uint8_t*>(d_stage);
    const hipError_t e = timed(K_PEERROUND, s, [&] {
        return launch_peer_round(reinterpret_cast<const PeTorrent*>(ds), n_torrents, x.units,
                                 reinterpret_cast<const uint64_t*>(ds + live_at), reinterpret_cast<const pe::Join*>(ds + join_at),
                                 reinterpret_cast<const uint32_t*>(ds + full_at), wire_dev, bits_dev, remaining_out,
                                 torrent_flags_out, held_out, wanted_out, status_out, s);
    });
    scratch_free(D, d_stage, s);
    KRK_CHECK(e == hipSuccess, KRK_EHIP, "peer_round launch: %s", launch_error_text(e));
    return KRK_OK;
}

int krk_peer_round_geometry(uint64_t* unit_cap, uint64_t* lane_words) {
    KRK_CHECK(unit_cap && lane_words, KRK_EINVAL, "peer_round_geometry: null argument");
    *unit_cap = kPeUnitCap;
    *lane_words = kPeLaneWords;
    return KRK_OK;
}

}  // extern "C"
