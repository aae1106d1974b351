// kernels.hpp -- device work descriptors and kernel launchers (implemented in *.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

namespace krk {

// What the last launcher on this thread launched, for the kernel timeline
// (krk_kernel_timeline): SHA-256 plan id (KRK_SHA_PLAN_*) and work units (streams for
// SHA-256, work items + runs for CRC).  Written by the launchers, read by timed().
inline thread_local int t_launch_plan = 0;
inline thread_local uint64_t t_launch_units = 0;

// Before a launch: an error already pending on this thread belongs to an earlier HIP call
// that nobody checked (the caller's own, or one outside the library).  It is reported, not
// cleared away: the launcher returns it without launching, and launch_error_text() says
// where it came from, so the entry point's message names it.  hipErrorNotReady is an event
// query's answer, not an error.
inline thread_local bool t_launch_pending = false;
inline hipError_t launch_precheck() {
    t_launch_pending = false;
    const hipError_t p = hipPeekAtLastError();
    if (p == hipSuccess) return hipSuccess;
    (void)hipGetLastError();
    if (p == hipErrorNotReady) return hipSuccess;
    t_launch_pending = true;
    return p;
}
inline const char* launch_error_text(hipError_t e) {
    static thread_local char buf[256];
    if (!t_launch_pending) return hipGetErrorString(e);
    snprintf(buf, sizeof buf, "HIP error pending from an earlier call on this thread: %s", hipGetErrorString(e));
    return buf;
}

// ---------------------------------------------------------------- CRC pieces
// One work item = a contiguous byte run inside ONE piece, processed by one wave.
// Its raw CRC is shifted to the piece end (mul = x^(8*(piece_end - item_end))) and
// XOR-ed into sums[out]; the piece's first item also carries the init/xorout term
// xr = shift(~0, piece_len) ^ ~0.  XOR is order-free, so items of one piece may run
// on any wave, XCD or launch.
struct alignas(16) CrcItem {
    uint64_t ptr;   // device address of the run
    uint32_t len;   // bytes, 1 .. kItemBytes
    uint32_t out;   // index into sums[]
    uint32_t mul;
    uint32_t xr;
    uint32_t pad[2];
};
static_assert(sizeof(CrcItem) == 32, "CrcItem layout");

constexpr uint32_t kSeg = 64;                // bytes per lane per wave step
constexpr uint32_t kStep = 64 * kSeg;        // bytes per wave step (4 KiB)
constexpr uint32_t kGap = kStep - kSeg;      // zero-gap between a lane's segments
constexpr uint32_t kItemBytes = 256 * 1024;  // max bytes per work item

// Global constant table layout (uint32 words).
constexpr int kTabT = 0;        // T0..T3 slicing tables, 1024 words
constexpr int kTabG = 1024;     // G0..G3 shift-by-kGap tables, 1024 words
constexpr int kTabLaneMul = 2048;  // 64 words: x^(8*(63-l)*kSeg)
constexpr int kTabX8Pow = 2112;    // 64 words: x^(8*2^k)
// Coalesced layout (variants 2, 3): wave step = 4 KiB loaded as four fully coalesced
// 1 KiB wave-instructions; lane l owns chain k = bytes [1024k + 16l, +16) of every
// step, so a chain's segments are kGapC = 4080 zero bytes apart.
constexpr uint32_t kGapC = kStep - 16;
constexpr int kTabGC = 2176;       // G0..G3 shift-by-kGapC tables, 1024 words
constexpr int kTabLaneMulC = 3200; // 256 words [k*64 + l]: x^(8*(kGapC - 1024k - 16l))
constexpr int kTabWords = 3456;

// A run of consecutive WHOLE pieces of one blob, expanded into work items on the
// device: a whole piece's items and their constants depend only on the piece
// length, so the host writes one run per blob range instead of one item per
// 256 KiB (C4: 81,920 items -> 1 run).  consts[cpat + j] is item j's piece-end
// shift, consts[cpat + ipp] the piece's init/xor-out term.
struct alignas(16) CrcRun {
    uint64_t ptr;        // device address of the run's first piece
    uint64_t plen;       // piece length
    uint32_t n_pieces;
    uint32_t out;        // sums index of the first piece
    uint32_t item_base;  // index of the run's first item in the launch
    uint32_t ipp;        // items per piece = ceil(plen / kItemBytes)
    uint32_t cpat;
    uint32_t pad[3];
};
static_assert(sizeof(CrcRun) == 48, "CrcRun layout");

// One CRC launch: items [0, run_items) come from the runs, [run_items,
// run_items + n_items) from the explicit item array.
struct CrcWork {
    const CrcRun* runs;
    const CrcItem* items;
    const uint32_t* consts;
    uint32_t n_runs;
    uint32_t run_items;
    uint32_t n_items;
    uint32_t pad;
    uint32_t* next;  // work-queue head (zeroed per launch): waves claim items by atomicAdd
};

struct CrcLaunchCfg {
    int cus;           // compute units
    int variant;       // crc32_pieces.hip launch_crc_items; default 16 (byte-addressable tables, work queue)
};

bool crc_variant_valid(int variant);
hipError_t launch_crc_items(const CrcWork& w, const uint32_t* tabs, uint32_t* sums, const CrcLaunchCfg& cfg,
                            hipStream_t s);

// Piece verification: ok[i] = (sums[i] == expected[i]).
hipError_t launch_crc_verify(const uint32_t* sums, const uint32_t* expected, uint8_t* ok,
                             uint32_t n, hipStream_t s);

// ---------------------------------------------------------------- SHA-256
// One job = one Merkle-Damgard stream, run by one lane.  Processes len bytes
// starting from midstate h (or from out_state + 8*out when kShaFromState); if
// kShaFinal, pads with total = prefix + len bytes and writes the big-endian digest
// to out_digest + 32*out, else writes the midstate (len must then be a multiple of
// 64) to out_state + 8*out.
constexpr uint32_t kShaFinal = 1;
constexpr uint32_t kShaFromState = 2;
struct alignas(16) ShaJob {
    uint64_t ptr;
    uint64_t len;
    uint64_t prefix;   // bytes absorbed before this job (for the length field)
    uint32_t out;
    uint32_t flags;
    uint32_t h[8];
};
static_assert(sizeof(ShaJob) == 64, "ShaJob layout");

// Digests computed elsewhere (host offload) into digests[32 * idx]: n records of a
// little-endian uint32 idx + 32 digest bytes.
hipError_t launch_digest_scatter(const uint8_t* rec, uint32_t n, uint8_t* digests, hipStream_t s);
hipError_t launch_sha256(const ShaJob* jobs, uint32_t n_jobs, uint8_t* out_digest,
                         uint32_t* out_state, hipStream_t s);
// Lanes per stream launch_sha256 uses for a batch of n_jobs streams (1, 2 or 8).
int sha_lanes_for(uint32_t n_jobs);
int sha_plan_for(uint32_t n_jobs);  // KRK_SHA_PLAN_* the next launch of n_jobs streams uses
// One launch on a given plan whatever the process-wide setting (planner calibration).
hipError_t launch_sha256_plan(int plan, const ShaJob* jobs, uint32_t n_jobs, uint8_t* out_digest,
                              uint32_t* out_state, hipStream_t s);
// Process-wide launch plan (KRK_SHA_PLAN_* of kraken_hip.h; diagnostic plans >= 100
// only in the KRK_DIAG build).
bool sha_plan_valid(int plan);
void set_sha_plan(int plan);

// ---------------------------------------------------------------- InfoHash
// One job = one blob's info.Hash() (info_hash.hip), run by one wave: SHA-1 over the bencoded
// info{length, names[name_off, +name_len), piece_length, sums[first_sum, +n_sums)}, the 20
// digest bytes to out20 + 20 * out.
struct alignas(16) InfoHashJob {
    int64_t piece_length;
    int64_t length;
    uint64_t first_sum;
    uint64_t n_sums;
    uint64_t name_off;
    uint64_t name_len;
    uint64_t out;
    uint64_t pad;
};
static_assert(sizeof(InfoHashJob) == 64, "InfoHashJob layout");
hipError_t launch_info_hash(const InfoHashJob* jobs, uint32_t n_jobs, const uint32_t* sums, const uint8_t* names,
                            uint8_t* out20, hipStream_t s);

// ---------------------------------------------------------------- piece bitfield
// One blob of a verify batch (piece_bitfield.hip): its sums are sums[first_sum, +n_pieces) and
// it is checked against expected[first_sum, +n_pieces); its bitfield is the ceil(n_pieces / 64)
// words from bits[first_word].  first_word ascends with the blob index (blob i's words follow
// blob i-1's) and blobs[0].first_word == 0.
struct alignas(16) BitfieldBlob {
    uint64_t first_sum;
    uint64_t n_pieces;  // < 2^32
    uint64_t first_word;
    uint64_t pad;
};
static_assert(sizeof(BitfieldBlob) == 32, "BitfieldBlob layout");
// bits[w] bit l = (piece 64 (w - first_word) + l of w's blob matches), n_bad[b] = blob b's
// mismatching pieces: every one of the n_words words and n_blobs counts is stored.
hipError_t launch_piece_bitfield(const BitfieldBlob* blobs, uint64_t n_blobs, uint64_t n_words, const uint32_t* sums,
                                 const uint32_t* expected, uint64_t* bits, uint32_t* n_bad, hipStream_t s);
// ok[i] = (digests[32 i, +32) == expected[32 i, +32)); both 16-byte aligned.
hipError_t launch_digest_equal(const uint8_t* digests, const uint8_t* expected, uint64_t n, uint8_t* ok,
                               hipStream_t s);

// ---------------------------------------------------------------- re-piece
// One blob of a re-piece batch (piece_repiece.hip): its stored sums are sums[first_old,
// + ceil(length / po)), its new sums, for pieces of po k bytes, out[first_new, + ceil(length /
// (po k))).  first_unit ascends with the blob index (blob i's units follow blob i-1's,
// rp::units of repiece_math.hpp) and blobs[0].first_unit == 0.
struct alignas(16) RepieceBlob {
    uint64_t first_old;
    uint64_t first_new;
    uint64_t length;
    uint64_t po;  // the stored piece length
    uint64_t k;   // new piece length / po, >= 1
    uint64_t first_unit;
};
static_assert(sizeof(RepieceBlob) == 48, "RepieceBlob layout");
// Every new sum of the n_units units is stored; x8pow is the x^(8 * 2^b) table (kTabX8Pow).
hipError_t launch_piece_repiece(const RepieceBlob* blobs, uint64_t n_blobs, uint64_t n_units, const uint32_t* x8pow,
                                const uint32_t* sums, uint32_t* out, hipStream_t s);

// ---------------------------------------------------------------- _torrentmeta JSON
// One blob of a serialise batch (metainfo_json.hip): its sums are sums[first_sum, + n_sums), its
// document goes to out + out_off.  first_unit ascends with the blob index (blob i's
// mj::ser_units(n_sums) units follow blob i-1's) and blobs[0].first_unit == 0.
struct alignas(16) MjSerBlob {
    uint64_t first_sum;
    uint64_t n_sums;
    uint64_t out_off;
    uint64_t first_unit;
    int64_t piece_length;
    int64_t length;
    uint32_t sums_null;  // PieceSums is `null` (then n_sums == 0)
    uint32_t pad[3];
    uint8_t name[64];
};
static_assert(sizeof(MjSerBlob) == 128, "MjSerBlob layout");
// The launch geometry of metainfo_json.hip (krk_metainfo_json_scan_geometry reports it).  In mj:
// piece_bitfield.hip and piece_repiece.hip have a kMaxBlocks of their own.
namespace mj {
constexpr uint32_t kMaxBlocks = 1u << 18;  // workgroups a launch has at the most; beyond, the waves stride
constexpr uint32_t kScanBlock = 256;       // threads of the scan's one workgroup
constexpr uint32_t kScanPer = 8;           // consecutive counts a thread of the scan takes a pass
}  // namespace mj
// scratch: mj_ser_scratch_bytes(n_units) of device memory, 8-byte aligned.  Every byte of every
// document and every out_len[i] is stored.
inline uint64_t mj_ser_scratch_bytes(uint64_t n_units) { return 8 * (n_units + 1) + 4 * n_units; }
hipError_t launch_metainfo_serialize(const MjSerBlob* blobs, uint64_t n_blobs, uint64_t n_units, const uint32_t* sums,
                                     uint8_t* out, uint64_t* out_len, void* scratch, hipStream_t s);
// One blob of a parse batch: the span between its document's brackets is text[text_off,
// + text_len), its expect_n sums go to sums_out[first_sum, + expect_n).  first_unit as above
// (mj::parse_units(text_len) units a blob).
struct alignas(16) MjParseBlob {
    uint64_t text_off;
    uint64_t text_len;
    uint64_t first_sum;
    uint64_t expect_n;
    uint64_t first_unit;
    uint64_t pad;
};
static_assert(sizeof(MjParseBlob) == 48, "MjParseBlob layout");
inline uint64_t mj_parse_scratch_bytes(uint64_t n_units) { return 8 * (n_units + 1) + 8 * n_units; }
hipError_t launch_metainfo_parse_sums(const MjParseBlob* blobs, uint64_t n_blobs, uint64_t n_units,
                                      const uint8_t* text, uint32_t* sums_out, uint32_t* status, void* scratch,
                                      hipStream_t s);

// ---------------------------------------------------------------- host gather
// One tile of a host -> device gather (gather.hip): n <= kGatherTile bytes from src (a
// device-visible address of page-locked host memory: a hipHostMalloc'd or registered
// mapping; any alignment) to dst (device, 16-B aligned, room for n rounded up to 16).
constexpr uint64_t kGatherTile = 64 << 10;
struct alignas(32) GatherTile {
    uint64_t src;
    uint64_t dst;
    uint64_t n;
    uint64_t pad;
};
static_assert(sizeof(GatherTile) == 32, "GatherTile layout");
hipError_t launch_gather(const GatherTile* tiles, uint32_t n_tiles, int cus, hipStream_t s);

// ---------------------------------------------------------------- HRW
// Scores for (key, node) pairs and the per-key descending order.
struct HrwArgs {
    const uint8_t* keys;      // decoded key bytes
    const uint64_t* key_off;  // n_keys + 1
    uint64_t n_keys;
    const uint8_t* labels;
    const uint64_t* label_off;  // n_nodes + 1
    const int64_t* weights;
    uint32_t n_nodes;
    uint32_t n_out;
    const uint8_t* key_bad;   // n_keys flags: invalid hex -> NaN scores
    int32_t* order;           // n_keys * n_out
    double* scores;           // nullable: n_keys * n_nodes
};
hipError_t launch_hrw_order(const HrwArgs& a, hipStream_t s);
// hrw.UInt64ToFloat64 of n Sum values (as uint64) on the device.
hipError_t launch_u64_to_f64(const uint64_t* vals, uint64_t n, int rehash, double* out, hipStream_t s);

// Locations filter over full orders (n_out == n_nodes rows).
hipError_t launch_ring_filter(const int32_t* order, uint64_t n_rows, uint32_t n_nodes,
                              const uint8_t* healthy, int32_t max_replica, uint32_t row_out,
                              int32_t* locs, uint8_t* counts, hipStream_t s);
// Per-digest gather from the 65,536-row shard table.
hipError_t launch_shard_gather(const uint8_t* digests32, uint64_t n, const int32_t* table_locs,
                               const uint8_t* table_counts, uint32_t row_out, int32_t* locs,
                               uint8_t* counts, hipStream_t s);
hipError_t launch_shard_gather_u8(const uint8_t* digests32, uint64_t n, const int32_t* table_locs,
                                  const uint8_t* table_counts, uint32_t row_out, uint8_t* locs,
                                  uint8_t* counts, hipStream_t s);
// The owner table of a ring of <= 255 nodes with rows of <= 3 owners packed one word a
// ShardID (owner bytes 0-2, 0xFF padded; the count in byte 3), and the gather over it:
// wave-contiguous digest loads, one word load a row, rows regrouped through LDS so owner
// lists and counts go out as whole words.
// Needs digests32 2-byte aligned and locs / counts 4-byte aligned (the caller checks).
hipError_t launch_pack_owner_rows(const int32_t* table_locs, const uint8_t* table_counts, uint32_t row_out,
                                  uint32_t* packed, hipStream_t s);
hipError_t launch_shard_gather_packed(const uint8_t* digests32, uint64_t n, const uint32_t* packed,
                                      uint32_t row_out, uint8_t* locs, uint8_t* counts, hipStream_t s);

// ---------------------------------------------------------------- ring select
// A 65,536-bit shard predicate applied to n digests (ring_select.hip): bits[i >> 6] bit i & 63 =
// (mask[ShardID(d_i)] ^ invert) | or_bits[i] (or_bits nullable; tail bits 0, every word stored),
// *count_out = the selected digests (stored for n == 0 too), idx (nullable with idx_cap == 0) the
// first min(count, idx_cap) selected i in ascending order.  mask: 2,048 words in device memory.
// A workgroup takes kSelectW digests; the workgroup counts are scanned in tiles of kSelectT.
constexpr uint32_t kSelectW = 1024;
constexpr uint32_t kSelectT = 256;
inline uint64_t ring_select_workgroups(uint64_t n) { return n / kSelectW + (n % kSelectW != 0); }
inline uint64_t ring_select_tiles(uint64_t n) {
    const uint64_t g = ring_select_workgroups(n);
    return g / kSelectT + (g % kSelectT != 0);
}
// scratch: ring_select_scratch_bytes(n) of device memory, 8-byte aligned.
inline uint64_t ring_select_scratch_bytes(uint64_t n) {
    return 12 * ring_select_tiles(n) + 4 * ring_select_workgroups(n) + 8;
}
hipError_t launch_ring_select(const uint8_t* digests32, uint64_t n, const uint32_t* mask, int invert,
                              const uint64_t* or_bits, uint64_t* bits, uint64_t* idx, uint64_t idx_cap,
                              uint64_t* count_out, void* scratch, hipStream_t s);
// The scratch of a selection over n digests: [tile_base u64 x tiles][workgroup counts, then
// offsets, u32 x workgroups][tile_sum u32 x tiles].
struct SelectScratch {
    uint64_t* tile_base;
    uint32_t* wg_count;
    uint32_t* tile_sum;
};
inline SelectScratch select_scratch(void* scratch, uint64_t n) {
    uint64_t* tile_base = static_cast<uint64_t*>(scratch);
    uint32_t* wg_count = reinterpret_cast<uint32_t*>(tile_base + ring_select_tiles(n));
    return {tile_base, wg_count, wg_count + ring_select_workgroups(n)};
}
// Phases 2 and 3 of a selection whose phase 1 has stored the bitset's words and the workgroup
// counts (wg_count[b] = the set bits of words [kSelectW / 64 b, + kSelectW / 64)): the scan,
// *count_out, and the index list.  launch_ring_select's own tail, and launch_cleanup_plan's.
hipError_t launch_select_scan_scatter(uint64_t n, const uint64_t* bits, uint64_t* idx, uint64_t idx_cap,
                                      uint64_t* count_out, void* scratch, hipStream_t s);

// ---------------------------------------------------------------- digest hex, cleanup plan
// A cache listing's text (digest_hex.hip, digest_hex_math.hpp): name i is names[off[i], off[i + 1]),
// 64 hex digits when valid.  parse: digests32[32 i, + 32) (zero for an invalid name; any
// alignment), status[i] (nullable) and valid (nullable, the bitset of "status 0", tail bits 0),
// every documented byte stored.  format: hex[64 i, + 64) lowercase, any alignment both sides.
// A workgroup takes kDhexW names.
constexpr uint32_t kDhexW = 1024;
hipError_t launch_digest_parse_hex(const uint8_t* names, const uint64_t* off, uint64_t n, uint8_t* digests32,
                                   uint32_t* status, uint64_t* valid, hipStream_t s);
hipError_t launch_digest_format_hex(const uint8_t* digests32, uint64_t n, uint8_t* hex, hipStream_t s);
// sel(i) = valid(i) & ((mask[ShardID(d_i)] ^ invert) | expired(now, mtime[i], ttl)) (mtime
// nullable: no expiry term) over the listing's text: bits, idx, idx_cap, count_out, mask and
// scratch as launch_ring_select, valid (nullable) as launch_digest_parse_hex.
hipError_t launch_cleanup_plan(const uint8_t* names, const uint64_t* off, uint64_t n, const int64_t* mtime, int64_t now,
                               int64_t ttl, const uint32_t* mask, int invert, uint64_t* bits, uint64_t* valid,
                               uint64_t* idx, uint64_t idx_cap, uint64_t* count_out, void* scratch, hipStream_t s);

// ---------------------------------------------------------------- piece requests
// One torrent of a request round (piece_request.hip, piece_request_math.hpp): its rows are
// bits[bits_off, + (1 + 2 n_peers) W), W = ceil(n_pieces / 64): have, then (bits_p, blocked_p) a
// peer; its peers are quota / n_picked [peer_off, + n_peers) and picks rows of `limit` from
// peer_off * limit; its counts are counts[piece_off, + n_pieces), its taken row the W words from
// taken[taken_off].  first_unit ascends with the torrent index (torrent t's
// ceil(n_pieces / kPrG) count units follow torrent t-1's) and tors[0].first_unit == 0.
struct alignas(16) PrTorrent {
    uint64_t n_pieces;  // < 2^32
    uint64_t bits_off;
    uint64_t peer_off;
    uint64_t piece_off;
    uint64_t seed;
    uint64_t taken_off;
    uint64_t first_unit;
    uint32_t n_peers;
    uint32_t flags;  // pr::kRarestFirst / pr::kSample | pr::kAllowDuplicates
};
static_assert(sizeof(PrTorrent) == 64, "PrTorrent layout");
constexpr uint32_t kPrG = 256;      // a count unit, and the thread stride of both kernels: one piece a thread
constexpr uint32_t kPrPass = 4096;  // the pieces one step of the selection scan covers: 16 strides
constexpr uint32_t kPrMaxBlocks = 1u << 10;  // count units beyond: the workgroups stride
// counts (nullable: no count launch; then no torrent may be rarest-first): every
// counts[piece_off + i] stored.  Then one workgroup a torrent runs its peers in order: every
// n_picked and picks entry stored; a quota above `limit` is read as `limit`.
hipError_t launch_piece_request(const PrTorrent* tors, uint64_t n_tors, uint64_t n_units, const uint64_t* bits,
                                const int32_t* quota, uint32_t limit, uint32_t* counts, uint64_t* taken,
                                uint32_t* picks, uint32_t* n_picked, hipStream_t s);

// One torrent of a resend round (piece_resend.hip, piece_resend_math.hpp): its rows as a request
// round's, its quotas quota[peer_off, + n_peers), its quota left left[left_off, + n_peers), its
// marks mark[mark_off, + n_peers) (scratch; touched from peer kRsS on, and only with
// allow-duplicates), its n_failed entries failed[list_off ..] with their targets at
// target[failed_off ..].  n_resent is indexed by the torrent.
namespace rs {
struct Failed;
}
struct alignas(16) RsTorrent {
    uint64_t n_pieces;  // < 2^32
    uint64_t bits_off;
    uint64_t peer_off;
    uint64_t left_off;
    uint64_t mark_off;
    uint64_t list_off;
    uint64_t failed_off;
    uint64_t n_failed;
    uint32_t n_peers;
    uint32_t flags;  // pr::kAllowDuplicates is read
    uint64_t pad;
};
static_assert(sizeof(RsTorrent) == 80, "RsTorrent layout");
constexpr uint32_t kRsS = 256;  // the peers one pass over a failed entry's peers covers: one peer a thread
// One workgroup a torrent runs its failed entries in order: every target, left and n_resent
// entry stored.  The lists are valid (rs::list_error).
hipError_t launch_piece_resend(const RsTorrent* tors, uint64_t n_tors, const uint64_t* bits, const int32_t* quota,
                               const rs::Failed* failed, int32_t* left, uint32_t* mark, uint32_t* target,
                               uint32_t* n_resent, hipStream_t s);

// ---------------------------------------------------------------- announce rounds
// One announce round (announce_round.hip, announce_math.hpp): the update launch sets every
// announcer's bits in window 0 of its torrent (atomic or), the handout launch -- one wave an
// announce -- stores every handout[a * (limit + 8) + j], n_out[a] and labels[3 a + k].  The
// torrents and announces are valid (an::torrent_error, an::announce_error), limit in [1, 64].
namespace an {
struct Torrent;
struct Announce;
}
hipError_t launch_announce_round(const an::Torrent* tors, const an::Announce* anns, uint64_t n_anns, uint64_t* bits,
                                 uint32_t limit, uint32_t policy, uint32_t* handout, uint32_t* n_out, uint32_t* labels,
                                 hipStream_t s);

// ---------------------------------------------------------------- connection rounds
// One torrent of a connection round (conn_round.hip, conn_math.hpp): its active and pending rows
// at bits[bits_off ..], its expiries at expiry[peer_off ..], its capacity at capacity[t]; its three
// lists in the staged arrays from tr_at / in_at / dial_at, their statuses from trans_off / in_off /
// dial_off of the three status outputs.
namespace cn {
struct Transition;
struct Incoming;
struct Round;
}
struct alignas(16) CnTorrent {
    uint64_t bits_off, peer_off;
    uint64_t tr_at, trans_off, n_trans;
    uint64_t in_at, in_off, n_in;
    uint64_t dial_at, dial_off, n_dial;
    uint32_t n_peers, self_peer, flags, pad;
    uint64_t pad2;
};
static_assert(sizeof(CnTorrent) == 112, "CnTorrent layout");
// One wave64 a torrent runs the three phases in order: every status, n_admitted[2t], [2t + 1],
// n_freed[t] and capacity[t] stored.  The lists are valid (cn::lists_error).
hipError_t launch_conn_round(const CnTorrent* tors, uint64_t n_tors, const cn::Transition* tr, const cn::Incoming* in,
                             const uint32_t* dial, const uint64_t* neighbors, uint64_t* bits, int64_t* expiry,
                             uint32_t* capacity, const cn::Round& round, uint32_t* tr_st, uint32_t* in_st, uint32_t* dial_st,
                             uint32_t* n_admitted, uint32_t* n_freed, hipStream_t s);
// One torrent of a preemption sweep: its active row, its three time arrays from peer_off, its
// close row at close[close_off ..].
struct alignas(16) CnSweep {
    uint64_t bits_off, peer_off, close_off;
    uint32_t n_peers, pad;
};
static_assert(sizeof(CnSweep) == 32, "CnSweep layout");
// One workgroup a torrent: every word of its close row and n_close[t] stored.
hipError_t launch_conn_preempt(const CnSweep* tors, uint64_t n_tors, const uint64_t* bits, const int64_t* created,
                               const int64_t* received, const int64_t* sent, int64_t now, int64_t tti, int64_t ttl,
                               uint64_t* close, uint32_t* n_close, hipStream_t s);

// ---------------------------------------------------------------- synthetic data
// One synthetic chunk: bytes [offset, offset + n) of the blob whose stream seed is `seed`.
struct SynthChunk {
    uint8_t* dst;
    uint64_t seed;
    uint64_t offset;
    uint64_t n;
};
hipError_t launch_synth_fill_chunks(const SynthChunk* chunks, uint32_t n_chunks, int variant, hipStream_t s);
// Shader clock probe: out[0] = shader cycles, out[1] = 100 MHz ticks of one spin.
hipError_t launch_clock_probe(uint32_t spins, uint64_t* out, hipStream_t s);
hipError_t launch_synth_fill(uint8_t* dst, uint64_t seed, uint64_t offset, uint64_t n,
                             int variant, hipStream_t s);

}  // namespace krk
