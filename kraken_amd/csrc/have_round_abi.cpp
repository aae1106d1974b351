// have_round_abi.cpp -- have rounds: the torrent's own row restored from the piece status sidecar,
// merged with a verify result and emitted as sidecar bytes, wire bitfield and missing list, for a
// batch of torrents.  The host form (krk_have_round: have_round_math.hpp on the calling thread, no
// device) and the device form (krk_have_round_dev, have_round.hip computing the same state and
// outputs).
#include "have_round_math.hpp"
#include "runtime.hpp"

using namespace krk;

static_assert(sizeof(krk_have_torrent) == 96, "krk_have_torrent layout");
static_assert(hv::kRestore == KRK_HV_RESTORE && hv::kInCache == KRK_HV_IN_CACHE && hv::kMergeOr == KRK_HV_MERGE_OR &&
                  hv::kMergeAnd == KRK_HV_MERGE_AND && hv::kEmitStatus == KRK_HV_EMIT_STATUS &&
                  hv::kEmitWire == KRK_HV_EMIT_WIRE && hv::kEmitMissing == KRK_HV_EMIT_MISSING &&
                  hv::kBadStatus == KRK_HV_BAD_STATUS,
              "have_round_math.hpp and kraken_hip.h name the same values");

namespace {

constexpr uint64_t kMaxOff = 1ull << 48;  // an offset past it is an error, and no sum of two overflows

// What a round touches of each array, in elements (0 when nothing is).
struct Extent {
    uint64_t bits = 0, sidecar = 0, ok = 0, changed = 0, missing = 0, status_out = 0, wire_out = 0;
};

// The checks both forms share; *x the batch's extents.
int check_round(const char* who, const krk_request_torrent* t, const krk_have_torrent* h, uint64_t n, Extent* x) {
    KRK_CHECK(!n || (t && h), KRK_EINVAL, "%s: torrents or haves is NULL", who);
    for (uint64_t k = 0; k < n; ++k) {
        const unsigned long long kk = k;
        const krk_have_torrent& H = h[k];
        KRK_CHECK(t[k].n_pieces < (1ull << 32), KRK_EINVAL, "%s: torrent %llu has %llu pieces (2^32 or more)", who, kk,
                  (unsigned long long)t[k].n_pieces);
        const char* why = hv::flags_error(H.flags);
        KRK_CHECK(!why, KRK_EINVAL, "%s: torrent %llu: %s: %#x", who, kk, why, H.flags);
        KRK_CHECK(!H.reserved, KRK_EINVAL, "%s: torrent %llu: a non-zero reserved field", who, kk);
        KRK_CHECK(H.piece_length >= 0 && H.length >= 0, KRK_EINVAL, "%s: torrent %llu: a negative piece_length or length", who,
                  kk);
        KRK_CHECK(t[k].bits_off < kMaxOff && H.status_off < kMaxOff && H.ok_off < kMaxOff && H.changed_off < kMaxOff &&
                      H.missing_off < kMaxOff && H.status_out_off < kMaxOff && H.wire_out_off < kMaxOff,
                  KRK_EINVAL, "%s: torrent %llu: an offset of 2^48 or more", who, kk);
        KRK_CHECK(H.status_off + H.status_len >= H.status_off && H.changed_off + H.changed_cap >= H.changed_off &&
                      H.missing_off + H.missing_cap >= H.missing_off,
                  KRK_EINVAL, "%s: torrent %llu: an offset plus its length or cap overflows", who, kk);
        const uint64_t N = t[k].n_pieces, W = pr::words(N);
        if (W) x->bits = std::max(x->bits, t[k].bits_off + W);
        if ((H.flags & hv::kRestore) && H.status_len == N && N) x->sidecar = std::max(x->sidecar, H.status_off + N);
        if ((H.flags & (hv::kMergeOr | hv::kMergeAnd)) && W) {
            x->ok = std::max(x->ok, H.ok_off + W);
            if (H.changed_cap) x->changed = std::max(x->changed, H.changed_off + std::min(H.changed_cap, N));
        }
        if ((H.flags & hv::kEmitMissing) && N && H.missing_cap)
            x->missing = std::max(x->missing, H.missing_off + std::min(H.missing_cap, N));
        if ((H.flags & hv::kEmitStatus) && N) x->status_out = std::max(x->status_out, H.status_out_off + N);
        if (H.flags & hv::kEmitWire) x->wire_out = std::max(x->wire_out, H.wire_out_off + 8 + 8 * W);
    }
    return KRK_OK;
}

}  // namespace

extern "C" {

int krk_have_round(const krk_request_torrent* torrents, const krk_have_torrent* haves, uint64_t n_torrents, uint64_t* bits,
                   const uint8_t* sidecar, const uint64_t* ok_bits, uint32_t* flags_out, uint32_t* n_unexpected_out,
                   uint32_t* n_changed_out, uint32_t* changed_out, uint32_t* n_complete_out, uint64_t* bytes_out,
                   uint8_t* status_out, uint8_t* wire_out, uint32_t* missing_out) {
    Extent x;
    const int r = check_round("have_round", torrents, haves, n_torrents, &x);
    if (r) return r;
    KRK_CHECK((bits || !x.bits) && (sidecar || !x.sidecar) && (ok_bits || !x.ok) && (changed_out || !x.changed) &&
                  (missing_out || !x.missing) && (status_out || !x.status_out) && (wire_out || !x.wire_out) &&
                  (!n_torrents || (flags_out && n_unexpected_out && n_changed_out && n_complete_out && bytes_out)),
              KRK_EINVAL, "have_round: null argument");
    for (uint64_t k = 0; k < n_torrents; ++k) {
        const krk_have_torrent& H = haves[k];
        const hv::Torrent T = {H.flags,
                               H.piece_length,
                               H.length,
                               sidecar ? sidecar + H.status_off : nullptr,
                               H.status_len,
                               ok_bits && (H.flags & (hv::kMergeOr | hv::kMergeAnd)) ? ok_bits + H.ok_off : nullptr,
                               changed_out ? changed_out + H.changed_off : nullptr,
                               changed_out ? H.changed_cap : 0,
                               missing_out ? missing_out + H.missing_off : nullptr,
                               missing_out ? H.missing_cap : 0,
                               status_out ? status_out + H.status_out_off : nullptr,
                               wire_out ? wire_out + H.wire_out_off : nullptr};
        const hv::Out o = hv::round_torrent(bits ? bits + torrents[k].bits_off : nullptr, torrents[k].n_pieces, T);
        flags_out[k] = o.flags, n_unexpected_out[k] = o.n_unexpected, n_changed_out[k] = o.n_changed;
        n_complete_out[k] = o.n_complete, bytes_out[k] = o.bytes;
    }
    return KRK_OK;
}

int krk_have_round_dev(const krk_request_torrent* torrents_host, const krk_have_torrent* haves_host, uint64_t n_torrents,
                       uint64_t* bits_dev, const uint8_t* sidecar_dev, const uint64_t* ok_bits_dev, uint32_t* flags_out,
                       uint32_t* n_unexpected_out, uint32_t* n_changed_out, uint32_t* changed_out, uint32_t* n_complete_out,
                       uint64_t* bytes_out, uint8_t* status_out, uint8_t* wire_out, uint32_t* missing_out, void* stream) {
    Extent x;
    int r = check_round("have_round_dev", torrents_host, haves_host, n_torrents, &x);
    if (r) return r;
    KRK_CHECK((bits_dev || !x.bits) && (sidecar_dev || !x.sidecar) && (ok_bits_dev || !x.ok) && (changed_out || !x.changed) &&
                  (missing_out || !x.missing) && (status_out || !x.status_out) && (wire_out || !x.wire_out) &&
                  (!n_torrents || (flags_out && n_unexpected_out && n_changed_out && n_complete_out && bytes_out)),
              KRK_EINVAL, "have_round_dev: null argument");
    KRK_CHECK(n_torrents <= 0x7FFFFFFFull, KRK_ERANGE, "have_round_dev: %llu torrents in one call",
              (unsigned long long)n_torrents);
    if (!n_torrents) return KRK_OK;
    KRK_DEVICE(D);
    KRK_CHECK(!(((uintptr_t)bits_dev | (uintptr_t)ok_bits_dev | (uintptr_t)bytes_out) & 7) &&
                  !(((uintptr_t)flags_out | (uintptr_t)n_unexpected_out | (uintptr_t)n_changed_out | (uintptr_t)changed_out |
                     (uintptr_t)n_complete_out | (uintptr_t)missing_out) &
                    3),
              KRK_EINVAL, "have_round_dev: bits_dev, ok_bits_dev and bytes_out must be 8-byte, the uint32 outputs 4-byte aligned");
    KRK_CHECK((!x.bits || device_writable(bits_dev, 8 * x.bits)) && (!x.sidecar || device_writable(sidecar_dev, x.sidecar)) &&
                  (!x.ok || device_writable(ok_bits_dev, 8 * x.ok)) && (!x.changed || device_writable(changed_out, 4 * x.changed)) &&
                  (!x.missing || device_writable(missing_out, 4 * x.missing)) &&
                  (!x.status_out || device_writable(status_out, x.status_out)) &&
                  (!x.wire_out || device_writable(wire_out, x.wire_out)) && device_writable(flags_out, 4 * n_torrents) &&
                  device_writable(n_unexpected_out, 4 * n_torrents) && device_writable(n_changed_out, 4 * n_torrents) &&
                  device_writable(n_complete_out, 4 * n_torrents) && device_writable(bytes_out, 8 * n_torrents),
              KRK_EINVAL,
              "have_round_dev: bits_dev, sidecar_dev, ok_bits_dev and the outputs (every span of them) must be device memory "
              "or page-locked host memory");
    hipStream_t s = pick(D, stream);
    std::vector<HvTorrent> stage(n_torrents);  // the torrents and their haves, one block
    for (uint64_t k = 0; k < n_torrents; ++k) {
        const krk_request_torrent& T = torrents_host[k];
        const krk_have_torrent& H = haves_host[k];
        stage[k] = {T.n_pieces,    T.bits_off,    H.piece_length, H.length,         H.status_off,   H.status_len, H.ok_off, H.changed_off,
                    H.changed_cap, H.missing_off, H.missing_cap,  H.status_out_off, H.wire_out_off, H.flags,      0};
    }
    void* d_stage = nullptr;  // copied into the library's pinned staging before this returns
    r = upload(D, stage.data(), stage.size() * sizeof(HvTorrent), &d_stage, s);
    if (r) return r;
    const HvArrays A = {bits_dev,       sidecar_dev, ok_bits_dev, flags_out, n_unexpected_out, n_changed_out, changed_out,
                        n_complete_out, bytes_out,   status_out,  wire_out,  missing_out};
    const hipError_t e = timed(K_HAVEROUND, s, [&] { return launch_have_round(static_cast<const HvTorrent*>(d_stage), n_torrents, A, s); });
    scratch_free(D, d_stage, s);
    KRK_CHECK(e == hipSuccess, KRK_EHIP, "have_round launch: %s", launch_error_text(e));
    return KRK_OK;
}

int krk_have_round_geometry(uint64_t* unit_cap, uint64_t* pass_words) {
    KRK_CHECK(unit_cap && pass_words, KRK_EINVAL, "have_round_geometry: null argument");
    *unit_cap = kHvUnitCap;
    *pass_words = kHvPassWords;
    return KRK_OK;
}

}  // extern "C"
