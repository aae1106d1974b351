/*
 * kraken_hip.h -- C ABI of the MI355X-native blob-metainfo hot path.
 *
 * The drop-in boundary.  Plain pointers and sizes only (no torch types); all
 * entry points are re-entrant and return KRK_OK (0) or a negative KRK_E*
 * code, with a thread-local message from krk_last_error().  The Go wrappers
 *  bind these through cgo and re-create the reference's exact
 * error strings.  Each entry point names the reference interface it replaces.
 *
 * Device work runs on the calling thread's current device (krk_set_device);
 * "stream" arguments are hipStream_t passed as void* (NULL = the library's
 * own per-device stream).  *_dev entry points take device pointers and do no
 * host<->device copies of bulk data; the host entry points stage through
 * library-owned hipHostMalloc buffers with double-buffered hipMemcpyAsync.
 */
#ifndef KRAKEN_HIP_H
#define KRAKEN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KRK_OK 0
#define KRK_EINVAL (-1)    /* bad argument; e.g. "piece length must be positive" */
#define KRK_EHIP (-2)      /* HIP runtime error (message has the hip error string) */
#define KRK_ENOMEM (-3)    /* host or device allocation failed */
#define KRK_ENODEV (-4)    /* no MI355X (gfx950) device visible */
#define KRK_ERANGE (-5)    /* output capacity too small */
#define KRK_EHEX (-6)      /* invalid hex key (hrw.Score returns NaN, rendezvous.go:154-157) */
#define KRK_EIO (-7)       /* file open/read failed (message has the path and errno text) */
#define KRK_EFORMAT (-8)   /* a _torrentmeta document outside the canonical form (message says where) */

/* ---------------------------------------------------------------- runtime */
const char* krk_version(void);
const char* krk_last_error(void);            /* thread-local, never NULL */
int krk_device_count(int* n);                /* gfx950 devices visible */
int krk_set_device(int dev);                 /* per calling thread */
/* Eager context creation (streams, CRC tables) for the devices in dev_mask (bit i =
 * device i; 0 = the calling thread's current device), so the first request on a
 * device does not pay it; otherwise contexts are created on first use.  KRK_ENODEV
 * if a masked device is absent or not gfx950.  (SURVEY.md 8(b) krk_init.) */
int krk_init(uint64_t dev_mask);
/* Free every device context: streams, tables, scratch, pinned upload slots and the
 * staging windows kept across host-path calls (up to 2 x 1 GiB pinned per device).
 * The caller guarantees no library call is in flight and every krk_digester /
 * krk_piece_stream / krk_stream handle is freed.  Later calls re-create contexts
 * lazily. */
int krk_shutdown(void);
int krk_synchronize(void);                   /* drain the library's streams on the current device */

/* ------------------------------------------------- CRC-32/IEEE piece sums
 * Replaces core.calcPieceSums (core/metainfo.go:158-179), the loop inside
 * core.NewMetaInfo (core/metainfo.go:55-79); PieceHash() = crc32.NewIEEE()
 * (core/piece_hash.go:22-24).  Pieces are [i*P, min((i+1)*P, L)), ceil(L/P)
 * sums, none for L == 0, no empty trailing piece. */

typedef struct krk_blob {
    const uint8_t* data;     /* device pointer (any alignment; 16 B is the fast path) */
    uint64_t length;         /* bytes */
    int64_t piece_length;    /* > 0, else KRK_EINVAL "piece length must be positive" */
    uint64_t sums_offset;    /* index of this blob's first sum in the sums array */
} krk_blob;

/* Number of piece sums for a blob: ceil(length / piece_length). */
uint64_t krk_num_pieces(uint64_t length, int64_t piece_length);

/* Device-resident batch: sums_dev (device, uint32) receives every blob's sums
 * at blobs[i].sums_offset.  Asynchronous on `stream`.
 * A call owns the span of sums_dev from its lowest sums_offset to its highest end
 * (sums_offset + krk_num_pieces): the span is zeroed before the sums are XOR-ed in, so words
 * in a gap between two blobs' ranges come back zero; words outside the span are not touched.
 * Give each call its own span. */
int krk_piece_sums_dev(const krk_blob* blobs, uint64_t n_blobs, uint32_t* sums_dev, void* stream);

/* Host forms (sums_host: krk_piece_sums_host, krk_piece_sums_files, krk_metainfo_digest_host,
 * krk_metainfo_digest_files): the same span, and the same advice -- give each call its own.
 * Every blob's own words are written, words outside the span are never touched, and a batch
 * with no piece at all writes nothing (sums_host may then be NULL).  A word in a GAP inside
 * the span belongs to the call and comes back either zero or as the caller left it,
 * depending on where the sums were computed:
 *   krk_metainfo_digest_host, krk_metainfo_digest_files   zero (the device span is copied back;
 *                                                         the host offload's blobs are then
 *                                                         written over their own words)
 *   krk_piece_sums_files, CRC placement GPU               zero (the same copy)
 *   krk_piece_sums_files, CRC placement HOST              untouched (threads write their pieces)
 *   krk_piece_sums_host                                   untouched, whatever its GPU share
 * Do not keep anything in a gap.  tests/test_gpu_window_matrix.py and
 * tests/test_window_matrix_cpu.py pin each row but the third. */

/* Host batch (end-to-end): blobs[i].data are HOST pointers; sums_host receives
 * the sums.  Streams bytes through pinned staging, overlapping H2D with the
 * kernel.  Synchronous.  This is the batch form of Generator.Generate's
 * NewMetaInfo call (lib/metainfogen/generator.go:41-58). */
int krk_piece_sums_host(const krk_blob* blobs, uint64_t n_blobs, uint32_t* sums_host);
/* krk_piece_sums_host and krk_verify_pieces_host split a batch, whole pieces at a time,
 * between host PCLMUL threads (the reference's own placement: one hash.Hash32 per piece,
 * lib/torrent/storage/agentstorage/torrent.go:182-193) and the GPU pass.  Pinned caller
 * bytes (krk_host_alloc) are DMA'd straight into the device windows and the GPU takes a
 * share learned from the previous calls' measured rates of both sides (first call: the
 * planner rates' model, at most 10 %) -- or none, when host-only calls measured faster
 * than split ones (after two split calls -- the first sets up the staging windows -- one
 * runs host-only to find out; every 16th call re-measures the other choice).  Pageable
 * bytes stay on the host (a staging copy per byte costs more than the GPU saves).
 * KRK_CRC_GPU_FRACTION forces the share. */

/* Piece sums of cache FILES: the batch form of Generator.Generate reading the
 * CAS cache file itself (lib/metainfogen/generator.go:41-58: GetCacheFileReader
 * -> NewMetaInfo).  Placement as krk_crc32_update (krk_set_crc_placement; AUTO =
 * the measured crossover, HOST without a device): HOST reads each file once in
 * 512 KiB preads on the host pool and CRCs each chunk in cache; GPU reads the
 * bytes (pread on a pool of host threads, or O_DIRECT when KRK_FILE_DIRECT=1 and
 * the filesystem allows it) straight into the pinned staging windows -- no
 * pageable copy -- and the windows feed the CRC kernel as in krk_piece_sums_host.
 * The call's bytes on each side are reported by
 * krk_crc_host_split (kraken_hip_internal.h).  length is the size
 * the caller stat-ed (Generate picks the piece length from it); a file shorter
 * than that is KRK_EIO "read blob: <path>: unexpected EOF".  Synchronous. */
typedef struct krk_file_blob {
    const char* path;
    uint64_t length;
    int64_t piece_length;    /* > 0 */
    uint64_t sums_offset;
} krk_file_blob;
int krk_piece_sums_files(const krk_file_blob* files, uint64_t n_files, uint32_t* sums_host);

/* Streaming form for NewMetaInfo(d, io.Reader, P): the cgo shim copies each Read() chunk in
 * with _update; _end returns the io.CopyN-loop results (core/metainfo.go:157-179).
 * Placement (KRK_PLACE_* below), fixed at _begin:
 *   KRK_PLACE_HOST  the caller's thread runs PCLMUL CRC-32 over each chunk in place (~17 GB/s
 *                   a core, the reference's own placement) -- no copy, no PCIe;
 *   KRK_PLACE_GPU   bytes go through the device's submission engine (pooled pinned slots;
 *                   the CRC requests of all concurrent streams and crc32_update calls share
 *                   launches); each slot's piece portions are hashed as independent
 *                   messages and folded into the piece sums on the host with the GF(2)
 *                   combine, so state crosses slot and piece boundaries;
 *   KRK_PLACE_AUTO  (krk_piece_stream_begin) the process setting (krk_set_crc_placement,
 *                   KRK_CRC_PLACEMENT), by default the crossover: HOST unless the host's CRC
 *                   capacity (the CPUs this process may use x one thread's measured PCLMUL
 *                   rate) is below what the host link could carry to the GPU (0.85 x the
 *                   measured pinned H2D rate) -- on MI355X hosts the host side carries
 *                   60-80 GB/s for one stream and > 100 GB/s for several against ~20 GB/s
 *                   through the engine; HOST when no gfx950 device is present.
 * HOST placement needs no device; GPU placement without one is KRK_ENODEV. */
typedef struct krk_piece_stream krk_piece_stream;
int krk_piece_stream_begin(int64_t piece_length, krk_piece_stream** out);
int krk_piece_stream_begin_on(int placement, int64_t piece_length, krk_piece_stream** out);
int krk_piece_stream_placement(const krk_piece_stream* s, int* placement);
int krk_piece_stream_update(krk_piece_stream* s, const uint8_t* host_buf, uint64_t n);
int krk_piece_stream_end(krk_piece_stream* s, uint32_t* sums_out, uint64_t cap,
                         uint64_t* n_sums, uint64_t* length);
void krk_piece_stream_free(krk_piece_stream* s);

/* crc32.Update(crc, IEEETable, p) for one buffer (hash.Hash32 Write path used by
 * agentstorage.Torrent.writePiece, lib/torrent/storage/agentstorage/torrent.go:175-199).
 * data is a HOST pointer.  AUTO (krk_crc32_update): calls of at most 64 KiB
 * (KRK_CRC_HOST_MAX) and every call while the crossover of krk_piece_stream_begin says HOST
 * run on the caller's thread (large ones shared with idle host-pool threads); the rest go
 * through the device's CRC queue, coalesced with the other pending requests of the device
 * into one launch.  krk_crc32_update_on forces a placement. */
int krk_crc32_update(uint32_t crc, const uint8_t* data, uint64_t n, uint32_t* out);
int krk_crc32_update_on(int placement, uint32_t crc, const uint8_t* data, uint64_t n, uint32_t* out);
/* What KRK_PLACE_AUTO means for new piece streams and crc32_update calls, process-wide:
 * KRK_PLACE_AUTO (default: the crossover), KRK_PLACE_HOST or KRK_PLACE_GPU. */
int krk_set_crc_placement(int placement);

/* Batch piece verification (the same kernel in verify mode): ok_out[i] = 1 iff
 * piece i of the blob matches expected[i].  data is a device pointer. */
int krk_verify_pieces_dev(const krk_blob* blob, const uint32_t* expected_host,
                          uint8_t* ok_out_host, void* stream);

/* Batched agent piece verification over HOST buffers: ok_out[i] = 1 iff
 * crc32(data[i][0:lengths[i]]) == expected[i] -- the h.Sum32() != GetPieceSum(pi)
 * check of agentstorage.Torrent.writePiece (lib/torrent/storage/agentstorage/
 * torrent.go:174-199, error "invalid piece sum"), for many received pieces (any
 * torrents, any lengths) in one pinned, pipelined GPU pass instead of one
 * hash.Hash32 per piece.  Synchronous. */
int krk_verify_pieces_host(const uint8_t* const* data, const uint64_t* lengths, const uint32_t* expected,
                           uint64_t n, uint8_t* ok_out);

/* ------------------------------------------- verify against stored MetaInfo
 * Which pieces of a blob still match the MetaInfo stored for it, answered as the reference
 * answers it: Torrent.Bitfield() (lib/torrent/storage/agentstorage/torrent.go:130-140), a
 * willf/bitset -- []uint64, piece i is bit (i & 63) of word (i >> 6), 1 = complete; the tail
 * bits of a blob's last word are 0.  This is the "recheck" of a download file against its
 * metainfo (the agent keeps complete[] only from what writePiece saw, torrent.go:174-220) and
 * the read-only scrub of a CAS cache against its _torrentmeta sidecars -- what
 * Generator.Generate (lib/metainfogen/generator.go:41-58) would compute, compared instead of
 * written.  For the origin the blob's SHA-256 (core.Digester, core/digester.go:28-72) is also
 * compared with its name (uploader.verify, origin/blobserver/uploader.go:74-94): the only check
 * that catches a sidecar regenerated over rotten bytes.
 *
 * Bitfield layout of a batch: blob i's krk_bitfield_words(num_pieces) words follow blob i-1's;
 * blob i's first word index is the running sum of krk_bitfield_words over the earlier blobs (a
 * blob without pieces owns no word).  n_bad[i] = blob i's mismatching pieces.  Every output
 * word, count and flag is written by the call; the caller pre-zeroes nothing. */
uint64_t krk_bitfield_words(uint64_t n_pieces);              /* ceil(n_pieces / 64) */
/* One blob's bitfield from sums already on the host (the bitset the agent's Bitfield() returns
 * for them): pure host code, no device; bit-identical to the device kernel.  n_bad_out may be
 * NULL. */
int krk_piece_bitfield(const uint32_t* sums, const uint32_t* expected, uint64_t n_pieces,
                       uint64_t* bits_out, uint32_t* n_bad_out);
/* Device-resident batch (the batch form of krk_verify_pieces_dev; with digests, of
 * uploader.verify + Generate compared): blobs[i].data are device pointers; expected_host is
 * indexed by blobs[i].sums_offset; expected_digests_host is n_blobs*32 bytes, or NULL for the
 * piece-sum pass alone.  With digests the SHA-256 and CRC kernels run as in
 * krk_metainfo_digest_dev (two streams joined into `stream`, the host offload as set).  One
 * wave ballots 64 consecutive pieces of one blob into one word.  bits_out, n_bad_out (n_blobs)
 * and digest_ok_out (n_blobs bytes, 1 = equal; non-NULL exactly when digests are given) are
 * device memory or page-locked host memory (krk_host_alloc): any other pointer is KRK_EINVAL
 * before anything is launched.  Asynchronous on `stream`: every host array is copied into the
 * library's staging before the call returns; the sums and digests stay in device scratch.
 * n_blobs == 0 is KRK_OK; KRK_ENODEV without a gfx950 device. */
int krk_verify_batch_dev(const krk_blob* blobs, uint64_t n_blobs, const uint32_t* expected_host,
                         const uint8_t* expected_digests_host, uint64_t* bits_out, uint32_t* n_bad_out,
                         uint8_t* digest_ok_out, void* stream);
/* The same over cache or download FILES, all arrays on the host.  Synchronous.  Without
 * digests it is krk_piece_sums_files underneath (the same CRC placement rule; HOST placement
 * needs no device; krk_crc_host_split reports the call's split); with digests it is
 * krk_metainfo_digest_files (one read a byte feeds both).  Errors are the underlying call's:
 * KRK_EIO "read blob: <path>: unexpected EOF", "open <path>: <errno text>". */
int krk_verify_files(const krk_file_blob* files, uint64_t n_files, const uint32_t* expected,
                     const uint8_t* expected_digests, uint64_t* bits_host, uint32_t* n_bad_host,
                     uint8_t* digest_ok_host);

/* ------------------------------------------- piece request rounds
 * What to ask the peers for next: the availability counts numPeersByPiece
 * (lib/torrent/scheduler/dispatch/dispatcher.go:257-284, :495) and
 * piecerequest.Manager.ReservePieces (piecerequest/manager.go:101-137) as bit-matrix work over
 * the bitset layout above.  One torrent of N pieces (N < 2^32), W = krk_bitfield_words(N), P peers
 * in a fixed order, a pipeline limit L (1 <= L <= KRK_PR_MAX_LIMIT):
 *   counts[i] = the peers whose bitfield has bit i set (the column sum of the peers' rows).
 *   For p = 0 .. P-1:  q = max(quota_p, 0);
 *     cand   = bits_p & ~have & ~blocked_p & ~taken;
 *     picks_p = the min(q, |cand|) candidates with the smallest (key(i), i), ascending in that pair;
 *     taken |= picks_p, unless KRK_PR_ALLOW_DUPLICATES (then taken stays empty).
 *   key(i) = counts[i]                                          KRK_PR_RAREST_FIRST
 *            splitmix64(seed ^ ((uint64)p << 32 | i)) >> 32     KRK_PR_SAMPLE
 * with splitmix64(x): z = x + 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 * z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31.  KRK_PR_SAMPLE is the reference's default
 * policy (default_policy.go:33-66, a uniform sample of `limit` valid candidates) made
 * reproducible from a seed.  blocked_p is validRequest (manager.go:224-236) as a bitset: outside
 * endgame the pieces with a pending, unexpired request to any peer, in endgame those pending to
 * p itself.  A round with one positive quota is ReservePieces for that peer; with several it is
 * ReservePieces called peer after peer at one clock instant (`taken` is the pending set growing).
 * The one deliberate difference is tie order: equal keys go to the LOWER PIECE INDEX, where the
 * reference's heap (rarest_first_policy.go:38-44) leaves them to container/heap's sift order; the
 * sequence of counts popped is the same.  Tail bits past N of any row are ignored: never counted,
 * never picked.
 *
 * Every output element is stored by the call, the caller pre-zeroes nothing: n_picked[p],
 * picks[p * limit + j] (0xFFFFFFFF for j >= n_picked[p]), and counts when asked for.
 * KRK_EINVAL, refused before any output is touched: n_pieces >= 2^32, a quota above the limit
 * (host forms; the device form cannot read quota_dev before the launch and reads such a quota
 * as the limit), a limit outside [1, KRK_PR_MAX_LIMIT], an unknown policy or flag bit, a NULL
 * that is not nullable. */
#define KRK_PR_MAX_LIMIT 16u
#define KRK_PR_RAREST_FIRST 0u
#define KRK_PR_SAMPLE 1u
#define KRK_PR_ALLOW_DUPLICATES 0x100u
#define KRK_PR_NONE 0xFFFFFFFFu
typedef struct {
    uint64_t n_pieces;    /* < 2^32 */
    uint32_t n_peers;
    uint32_t flags;       /* policy | KRK_PR_ALLOW_DUPLICATES */
    uint64_t seed;        /* KRK_PR_SAMPLE only */
    uint64_t bits_off;    /* first word of its rows in `bits`: have, then (bits_p, blocked_p) a peer */
    uint64_t peer_off;    /* first peer in quota / n_picked / picks (picks row = peer * limit) */
    uint64_t piece_off;   /* first piece in counts_out */
} krk_request_torrent;
/* counts_out[i], i < n_pieces, from n_peers rows of krk_bitfield_words(n_pieces) words back to
 * back.  No device. */
int krk_piece_availability(const uint64_t* peer_bits, uint32_t n_peers, uint64_t n_pieces, uint32_t* counts_out);
/* selectPieces with `valid` passed as a bitset: the min(max(q, 0), |cand & ~blocked|) smallest
 * (key(i), i) of one peer (`peer` enters KRK_PR_SAMPLE's key).  picks_out holds max(q, 0)
 * entries, those from *n_out on 0xFFFFFFFF; q > KRK_PR_MAX_LIMIT is KRK_EINVAL.  blocked is
 * nullable, counts is nullable under KRK_PR_SAMPLE.  No device. */
int krk_piece_select(const uint64_t* cand, const uint64_t* blocked, const uint32_t* counts, uint64_t n_pieces,
                     int32_t q, uint32_t flags, uint64_t seed, uint32_t peer, uint32_t* picks_out,
                     uint32_t* n_out);
/* The whole round of n_torrents torrents on the host.  counts_out is nullable.  The regions the
 * torrents name in one array must not overlap. */
int krk_piece_request_round(const krk_request_torrent* torrents, uint64_t n_torrents, const uint64_t* bits,
                            const int32_t* quota, uint32_t limit, uint32_t* counts_out, uint32_t* picks_out,
                            uint32_t* n_picked_out);
/* The same on the device (piece_request.hip), bit for bit; asynchronous on `stream`: one launch
 * for the counts and one for the rounds, one workgroup a torrent.  bits_dev, quota_dev and the
 * outputs are device memory or page-locked host memory (krk_host_alloc), bits_dev 8-byte and the
 * others 4-byte aligned: anything else is KRK_EINVAL before anything is launched.  torrents_host
 * is copied into the library's staging before the call returns.  n_torrents == 0 is KRK_OK;
 * KRK_ENODEV without a gfx950 device: there is no fall-back to the host form. */
int krk_piece_request_round_dev(const krk_request_torrent* torrents_host, uint64_t n_torrents,
                                const uint64_t* bits_dev, const int32_t* quota_dev, uint32_t limit,
                                uint32_t* counts_out, uint32_t* picks_out, uint32_t* n_picked_out, void* stream);

/* ------------------------------------------- resend rounds
 * Where the failed piece requests go next: Dispatcher.resendFailedPieceRequests
 * (lib/torrent/scheduler/dispatch/dispatcher.go:401-434) for every torrent of a batch, over the
 * rows of a request round.  A torrent is its krk_request_torrent, unchanged (piece_off, the seed
 * and the policy bits of flags are not read -- one candidate needs no choice --
 * KRK_PR_ALLOW_DUPLICATES is), and a list of F failed requests that ascends by piece, the
 * entries of one piece adjacent and in the caller's order:
 *   left_p = max(quota_p, 0)
 *   for f = 0 .. F-1, i = piece_f:
 *     target_f = KRK_PR_NONE
 *     for p = 0 .. P-1:                      the first eligible peer wins
 *       skip if status_f is EXPIRED or INVALID and p == peer_f      (dispatcher.go:412-416)
 *       skip unless bit i of bits_p and not bit i of have           (:418-420)
 *       skip if left_p == 0                                         (requestQuota, manager.go:110-113)
 *       skip if bit i of blocked_p                                  (validRequest, :224-236)
 *       skip if an earlier entry of this call with the same piece was resent
 *            to p (KRK_PR_ALLOW_DUPLICATES) / to any peer (otherwise)
 *       target_f = p; left_p -= 1; break
 * The last skip is the pending set growing inside the call: after ReservePieces(p, {i}) the new
 * request blocks p itself and, outside endgame, everybody.  quota_p is requestQuota(p), any int32.
 * Two deliberate differences from the reference.  It walks the failed requests in Go map order
 * and the peers in sync.Map order, both random; here the list order is the caller's (ascending
 * piece) and the peers go in index order.  Its `sent` counter is shadowed and never incremented
 * (:408, :422); n_resent_out is the count it meant to keep.
 *
 * Every output element is stored by the call, the caller pre-zeroes nothing:
 * target_out[failed_off + f] (the peer's index or KRK_PR_NONE), quota_left_out[peer_off + p]
 * (left_p after the torrent's list; nullable) and n_resent_out[t].  KRK_EINVAL, refused before
 * any output is touched: n_pieces >= 2^32, a piece >= n_pieces, a peer that is neither < n_peers
 * nor KRK_PR_NONE, a status outside 1..3, a list that does not ascend by piece, an unknown flag
 * bit, a NULL that is not nullable.  KRK_ERANGE: a list of 2^32 entries or more.  The regions the
 * torrents name in one array must not overlap. */
#define KRK_PR_EXPIRED 1u /* piecerequest.StatusExpired / StatusUnsent / StatusInvalid */
#define KRK_PR_UNSENT 2u
#define KRK_PR_INVALID 3u
typedef struct {
    uint32_t piece;
    uint32_t peer;   /* index among the torrent's peers, or KRK_PR_NONE: the peer has left (ClearPeer
                        ejects only the first entry a piece, manager.go:188-196, so such entries survive) */
    uint32_t status; /* KRK_PR_EXPIRED, KRK_PR_UNSENT, KRK_PR_INVALID */
} krk_failed_request;
typedef struct {
    uint64_t failed_off; /* first entry in `failed` and in target_out */
    uint64_t n_failed;
} krk_resend_torrent;    /* parallel to torrents[] */
/* The whole round of n_torrents torrents on the host.  No device. */
int krk_piece_resend_round(const krk_request_torrent* torrents, const krk_resend_torrent* resends,
                           uint64_t n_torrents, const uint64_t* bits, const int32_t* quota,
                           const krk_failed_request* failed, uint32_t* target_out, int32_t* quota_left_out,
                           uint32_t* n_resent_out);
/* The same on the device (piece_resend.hip), bit for bit; asynchronous on `stream`: one launch,
 * one workgroup a torrent.  bits_dev, quota_dev and the outputs are device memory or page-locked
 * host memory (krk_host_alloc), bits_dev 8-byte and the others 4-byte aligned: anything else is
 * KRK_EINVAL before anything is launched.  torrents_host, resends_host and failed_host are host
 * memory: the lists are checked as above, and all three are copied into the library's staging,
 * before the call returns.  n_torrents == 0 is KRK_OK; KRK_ENODEV without a gfx950 device: there
 * is no fall-back to the host form. */
int krk_piece_resend_round_dev(const krk_request_torrent* torrents_host, const krk_resend_torrent* resends_host,
                               uint64_t n_torrents, const uint64_t* bits_dev, const int32_t* quota_dev,
                               const krk_failed_request* failed_host, uint32_t* target_out,
                               int32_t* quota_left_out, uint32_t* n_resent_out, void* stream);

/* ------------------------------------------- announce rounds
 * Whom an announcing peer talks to: the tracker's announce (tracker/trackerserver/announce.go:75-115)
 * for a batch of announces at one clock instant -- peerstore UpdatePeer and GetPeers
 * (tracker/peerstore/redis.go:126-196), the blob's origins appended, PriorityPolicy.SortPeers
 * (tracker/peerhandoutpolicy/peerhandoutpolicy.go:65-99) -- as bit-matrix work.  A torrent's peer
 * store is a bit matrix over its P known peers (P < 2^30; the identities stay with the caller, who
 * maps them to indices): a ring of W windows, each two rows of WP = krk_bitfield_words(P) words,
 * member_w then complete_w.  Window w (0 = the current one) is ring row (cur_row + w) % W, at words
 * bits_off + 2 * row * WP.  With splitmix64 as KRK_PR_SAMPLE defines it above:
 *   wkey(w)    = splitmix64(seed ^ ((uint64)(w + 1) << 32 | 0xFFFFFFFF)) >> 32    window order
 *   pkey(w, i) = splitmix64(seed ^ ((uint64)(w + 1) << 32 | i)) >> 32             SRANDMEMBER in window w
 *   okey(c)    = splitmix64(seed ^ c) >> 32     final order; c = i for peer i, KRK_AN_ORIGIN | o for origin o
 * A round of A announces has two phases:
 *   update (UpdatePeer)    for every announce: set bit `peer` of member_0, and of complete_0 under
 *                          KRK_AN_COMPLETE.  `bits` is read and written.
 *   handout (getPeerHandout, GetPeers, SortPeers)   each announce on its own, over the updated rows:
 *     under KRK_AN_COMPLETE: n_out = 0 and the label counts 0 (announce.go:96-100); otherwise
 *     selected = {};  for the windows in ascending (wkey(w), w), while |selected| < limit:
 *       need   = limit - |selected|
 *       sample = the min(need, |member_w|) members of window w with the smallest (pkey(w, i), i)
 *       selected |= sample;  complete |= sample & complete_w
 *     (a sample may repeat peers already selected, so |selected| may grow by fewer than `need`:
 *     redis.go:172-188 does the same);
 *     append the torrent's O origins; drop `source`;
 *     priority under KRK_AN_COMPLETENESS: complete peer (seeder) 0, origin 1, incomplete peer 2;
 *              under KRK_AN_DEFAULT: 0 for all;
 *     order by ascending (priority, okey(c), c).
 * Tail bits past P of any row are ignored: never sampled, and the update never sets one.
 *
 * Three deliberate differences from the reference.  Its random choices -- ShuffleInt64s over the
 * windows, SRANDMEMBER, the Go map order of `selected` and sort.Slice, which is not stable -- are
 * the seeded keys above: reproducible, and the same on host and device.  All updates of a round
 * land before any handout of the round, where the server interleaves them announce by announce.
 * And the reference drops the source by POINTER comparison (peerhandoutpolicy.go:69), which never
 * matches the PeerInfos the store has just built, so its server hands an announcer its own entry
 * back; here `source` is an index, which is the intent, and KRK_AN_NONE reproduces the server.
 *
 * Every output element is stored by the call, the caller pre-zeroes nothing: n_out[a];
 * handout_out[a * (limit + KRK_AN_MAX_ORIGINS) + j] = c, with KRK_AN_COMPLETE_BIT set for a complete
 * peer (never for an origin: origins are always complete), KRK_AN_NONE for j >= n_out[a];
 * label_counts_out[a * 3 + priority], the policy's three gauges (peer_seeder, origin,
 * peer_incomplete; under KRK_AN_DEFAULT everything lands in slot 0).  KRK_EINVAL, refused before
 * any output or bit is touched: P >= 2^30, W outside [1, KRK_AN_MAX_WINDOWS], O above
 * KRK_AN_MAX_ORIGINS, a limit outside [1, KRK_AN_MAX_LIMIT], cur_row >= W, torrent >= n_torrents,
 * peer >= P, a source that is neither < P nor KRK_AN_NONE, an unknown policy or flag bit, a
 * non-zero `reserved`, an offset of 2^48 or more, a NULL.  A == 0 is KRK_OK.  The regions the
 * torrents name in `bits` must not overlap. */
#define KRK_AN_MAX_WINDOWS 8u
#define KRK_AN_MAX_ORIGINS 8u
#define KRK_AN_MAX_LIMIT 64u
#define KRK_AN_DEFAULT 0u       /* peerhandoutpolicy "default" */
#define KRK_AN_COMPLETENESS 1u  /* peerhandoutpolicy "completeness" */
#define KRK_AN_COMPLETE 1u      /* krk_announce.flags: the peer announces as complete */
#define KRK_AN_NONE 0xFFFFFFFFu
#define KRK_AN_ORIGIN 0x80000000u
#define KRK_AN_COMPLETE_BIT 0x40000000u
typedef struct {
    uint64_t n_peers;     /* P < 2^30 */
    uint32_t n_windows;   /* W in [1, KRK_AN_MAX_WINDOWS] */
    uint32_t cur_row;     /* window w (0 = current) is ring row (cur_row + w) % W */
    uint32_t n_origins;   /* O in [0, KRK_AN_MAX_ORIGINS] */
    uint32_t reserved;    /* 0 */
    uint64_t bits_off;    /* first word of its 2*W rows in `bits`: (member, complete) a ring row */
} krk_announce_torrent;
typedef struct {
    uint32_t torrent;     /* index into torrents[] */
    uint32_t peer;        /* the announcer's index, < P */
    uint32_t flags;       /* KRK_AN_COMPLETE */
    uint32_t source;      /* index to leave out of the handout, or KRK_AN_NONE */
    uint64_t seed;
} krk_announce;
/* One announce's handout phase over the rows as they are (no update).  handout_out holds
 * limit + KRK_AN_MAX_ORIGINS entries, label_counts_out three.  No device. */
int krk_announce_handout(const krk_announce_torrent* torrents, uint64_t n_torrents, const uint64_t* bits,
                         const krk_announce* announce, uint32_t limit, uint32_t policy, uint32_t* handout_out,
                         uint32_t* n_out, uint32_t* label_counts_out);
/* The whole round on the host: every update, then every handout.  No device. */
int krk_announce_round(const krk_announce_torrent* torrents, uint64_t n_torrents, uint64_t* bits,
                       const krk_announce* announces, uint64_t n_announces, uint32_t limit, uint32_t policy,
                       uint32_t* handout_out, uint32_t* n_out, uint32_t* label_counts_out);
/* The same on the device (announce_round.hip), bit for bit, the updated rows included;
 * asynchronous on `stream`: one launch for the updates (one thread an announce) and one for the
 * handouts (one wave an announce).  bits_dev and the outputs are device memory or page-locked host
 * memory (krk_host_alloc), bits_dev 8-byte and the others 4-byte aligned: anything else is
 * KRK_EINVAL before anything is launched.  torrents_host and announces_host are checked as above
 * and copied into the library's staging before the call returns.  KRK_ERANGE: 2^31 announces or
 * more.  KRK_ENODEV without a gfx950 device: there is no fall-back to the host form. */
int krk_announce_round_dev(const krk_announce_torrent* torrents_host, uint64_t n_torrents, uint64_t* bits_dev,
                           const krk_announce* announces_host, uint64_t n_announces, uint32_t limit,
                           uint32_t policy, uint32_t* handout_out, uint32_t* n_out, uint32_t* label_counts_out,
                           void* stream);

/* ------------------------------------------- connection rounds
 * The step between an announce's handout and a request round's "P connected peers":
 * connstate.State (lib/torrent/scheduler/connstate/state.go) and the scheduler events that drive
 * it (lib/torrent/scheduler/events.go:125-285, :369-392) for every torrent of a batch.  The caller
 * maps a torrent's known peers to indices (the index space of its request rounds), P < 2^30,
 * WP = krk_bitfield_words(P).  A torrent's state:
 *   bits[bits_off ..]          two rows of WP words: active, then pending
 *   expiry[peer_off + p]       the blacklist entry's expiration in the caller's clock units, 0: never
 *   capacity[t]                MaxOpenConnectionsPerTorrent minus the pending and active conns
 *                              (state.go:160-164); the caller initialises it
 * Tail bits past P of any row, neighbour rows included, are ignored and never set.
 *
 * One round, scalars now, blacklist_duration, max_mutual and flags (KRK_CN_DISABLE_BLACKLIST),
 * runs a torrent's three lists in a fixed order.  Blacklisted(p) is expiry_p > now (state.go:46-52).
 * blacklist(p): nothing under KRK_CN_DISABLE_BLACKLIST; else if Blacklisted(p) the status gains
 * KRK_CN_STILL_BLACKLISTED (state.go:128-130) and the entry stays; else
 * expiry_p = now + blacklist_duration and the status gains KRK_CN_BLACKLISTED_NOW.
 *  1. transitions {peer, kind}, strictly ascending by peer (one a connection a round; they commute):
 *       ESTABLISHED (MovePendingToActive)  pending: cleared, active set, OK; else NOT_PENDING.
 *                                          A closed conn is the caller's to filter.
 *       FAILED_IN   (failedIncomingHandshakeEvent)  pending: cleared, capacity + 1, OK | FREED; else NOOP
 *       FAILED_OUT  (failedOutgoingHandshakeEvent)  as FAILED_IN, then blacklist(p) in both cases
 *       CLOSED      (connClosedEvent)      active: cleared, capacity + 1, OK | FREED; else NOOP;
 *                                          then blacklist(p) in both cases, as the reference does
 *  2. incoming handshakes {peer, neigh_off}, in list order; neigh_off is a word offset into
 *     `neighbors` of one WP-word row (the remote's RemoteBitfields() keys as bits), or
 *     KRK_CN_NO_ROW.  AddPending's checks in its order (state.go:158-184):
 *       capacity == 0 -> AT_CAPACITY; pending_p -> ALREADY_PENDING; active_p -> ALREADY_ACTIVE;
 *       popcount(neigh & (active | pending)) > max_mutual -> TOO_MANY_MUTUAL (strictly greater);
 *       else pending_p = 1, capacity - 1 -> OK.
 *     An admission is seen by the entries after it.  The blacklist is not consulted, as in the reference.
 *  3. dials: candidate peer indices, one announce handout in handout order
 *     (announceResultEvent.apply, events.go:257-285).  Under KRK_CN_TORRENT_COMPLETE every entry is
 *     TORRENT_IS_COMPLETE and nothing changes.  Otherwise, in list order:
 *       p == self_peer -> SELF; Blacklisted(p) -> BLACKLISTED (also under DISABLE_BLACKLIST, as the
 *       reference); capacity == 0 -> AT_CAPACITY; pending_p -> ALREADY_PENDING (a duplicate of an
 *       entry admitted earlier lands here); active_p -> ALREADY_ACTIVE;
 *       else pending_p = 1, capacity - 1 -> OK: the caller dials these.
 * Two deliberate differences from the reference.  Its event loop applies events in arrival order;
 * a round applies frees first, then incoming, then dials: a caller who needs another interleaving
 * makes several calls, and a round with one non-empty list is exactly that event type.  Its dial
 * loop breaks at ErrTorrentAtCapacity; here every remaining entry gets its status, and the state is
 * the same because capacity == 0 is AddPending's first check.
 *
 * Every output element is stored by the call, the caller pre-zeroes nothing: one status an entry
 * of each list (at the list's offset), n_admitted_out[2t] (incoming) and [2t + 1] (dials),
 * n_freed_out[t].  bits, expiry and capacity are read and written.  KRK_EINVAL, refused before any
 * output, bit, expiry or capacity is touched: P >= 2^30, a peer >= P in any list, a self_peer that
 * is neither < P nor KRK_CN_NONE, an unknown kind or flag bit, a reserved field that is not 0,
 * transitions that do not ascend strictly, now < 0, blacklist_duration < 0 or their sum past
 * INT64_MAX, a neighbour row that runs past n_neighbor_words, an offset >= 2^48, a NULL that is not
 * nullable (a pointer nothing is read from or stored to may be NULL), and in the host form a
 * capacity >= 2^31.  KRK_ERANGE: a list of 2^32 entries or more.  n_torrents == 0 is KRK_OK.  The
 * regions the torrents name in one array must not overlap. */
#define KRK_CN_NONE 0xFFFFFFFFu                /* self_peer: we are not among the torrent's peers */
#define KRK_CN_NO_ROW 0xFFFFFFFFFFFFFFFFull    /* neigh_off: no neighbours */
#define KRK_CN_TORRENT_COMPLETE 1u             /* krk_conn_torrent.flags: dispatcher.Complete() */
#define KRK_CN_DISABLE_BLACKLIST 1u            /* a round's flags: Config.DisableBlacklist */
#define KRK_CN_ESTABLISHED 0u                  /* krk_conn_transition.kind */
#define KRK_CN_FAILED_IN 1u
#define KRK_CN_FAILED_OUT 2u
#define KRK_CN_CLOSED 3u
#define KRK_CN_OK 0x001u                       /* status bits */
#define KRK_CN_FREED 0x002u
#define KRK_CN_NOOP 0x004u
#define KRK_CN_NOT_PENDING 0x008u              /* ErrInvalidActiveTransition */
#define KRK_CN_BLACKLISTED_NOW 0x010u
#define KRK_CN_STILL_BLACKLISTED 0x020u        /* "conn is already blacklisted" */
#define KRK_CN_AT_CAPACITY 0x040u              /* ErrTorrentAtCapacity */
#define KRK_CN_ALREADY_PENDING 0x080u          /* ErrConnAlreadyPending */
#define KRK_CN_ALREADY_ACTIVE 0x100u           /* ErrConnAlreadyActive */
#define KRK_CN_TOO_MANY_MUTUAL 0x200u          /* ErrTooManyMutualConns */
#define KRK_CN_SELF 0x400u
#define KRK_CN_BLACKLISTED 0x800u
#define KRK_CN_TORRENT_IS_COMPLETE 0x1000u
typedef struct {
    uint32_t n_peers;   /* P */
    uint32_t self_peer; /* our own index among the torrent's peers, or KRK_CN_NONE */
    uint32_t flags;     /* KRK_CN_TORRENT_COMPLETE */
    uint32_t reserved;  /* 0 */
    uint64_t bits_off;  /* first word of the active row in `bits`; the pending row follows */
    uint64_t peer_off;  /* first entry in expiry (a round) / created, received, sent (a sweep) */
    uint64_t close_off; /* first word of the close row in close_out: krk_conn_preempt only */
} krk_conn_torrent;
typedef struct {
    uint64_t trans_off, n_trans; /* first entry in `transitions` and in trans_status_out */
    uint64_t in_off, n_in;       /* ... in `incoming` and in in_status_out */
    uint64_t dial_off, n_dial;   /* ... in `dials` and in dial_status_out */
} krk_conn_lists;                /* parallel to torrents[] */
typedef struct {
    uint32_t peer;
    uint32_t kind; /* KRK_CN_ESTABLISHED .. KRK_CN_CLOSED */
} krk_conn_transition;
typedef struct {
    uint32_t peer;
    uint32_t reserved;  /* 0 */
    uint64_t neigh_off; /* word offset of the WP-word row in `neighbors`, or KRK_CN_NO_ROW */
} krk_conn_incoming;
/* The whole round of n_torrents torrents on the host.  No device. */
int krk_conn_round(const krk_conn_torrent* torrents, const krk_conn_lists* lists, uint64_t n_torrents, uint64_t* bits,
                   int64_t* expiry, uint32_t* capacity, const krk_conn_transition* transitions,
                   const krk_conn_incoming* incoming, const uint32_t* dials, const uint64_t* neighbors,
                   uint64_t n_neighbor_words, int64_t now, int64_t blacklist_duration, uint32_t max_mutual,
                   uint32_t flags, uint32_t* trans_status_out, uint32_t* in_status_out, uint32_t* dial_status_out,
                   uint32_t* n_admitted_out, uint32_t* n_freed_out);
/* The same on the device (conn_round.hip), bit for bit -- rows, expiries, capacities and every
 * output; asynchronous on `stream`: one launch, one wave a torrent.  bits_dev, expiry_dev,
 * capacity_dev, neighbors_dev and the outputs are device memory or page-locked host memory
 * (krk_host_alloc), the 64-bit arrays 8-byte and the others 4-byte aligned: anything else is
 * KRK_EINVAL before anything is launched.  The torrents and the three lists are host memory,
 * checked as above and copied into the library's staging before the call returns.  The capacities
 * cannot be read before the launch and are trusted to be below 2^31.  KRK_ERANGE: 2^31 torrents or
 * more.  KRK_ENODEV without a gfx950 device: there is no fall-back to the host form. */
int krk_conn_round_dev(const krk_conn_torrent* torrents_host, const krk_conn_lists* lists_host, uint64_t n_torrents,
                       uint64_t* bits_dev, int64_t* expiry_dev, uint32_t* capacity_dev,
                       const krk_conn_transition* transitions_host, const krk_conn_incoming* incoming_host,
                       const uint32_t* dials_host, const uint64_t* neighbors_dev, uint64_t n_neighbor_words, int64_t now,
                       int64_t blacklist_duration, uint32_t max_mutual, uint32_t flags, uint32_t* trans_status_out,
                       uint32_t* in_status_out, uint32_t* dial_status_out, uint32_t* n_admitted_out,
                       uint32_t* n_freed_out, void* stream);
/* The preemption tick's connection half (preemptionTickEvent, events.go:370-392), element-wise:
 * peer p of torrent t is closed iff active_p and either
 *   now - max(created_p, received_p, sent_p) > conn_tti   (idle; timeutil.MostRecent is a max)
 *   or now - created_p > conn_ttl                          (expired); both strict, as the reference.
 * The three int64 arrays (CreatedAt, LastGoodPieceReceived, LastPieceSent) are indexed from
 * peer_off; 0 is "never", and a negative time counts as 0.  Only the active row of `bits` is read;
 * self_peer and flags are not.  Stored: close_out[close_off + w] for every word of the row (tail
 * bits 0) and n_close_out[t].  KRK_EINVAL before anything is touched: P >= 2^30, an offset >= 2^48,
 * a non-zero reserved, a negative now, conn_tti or conn_ttl, a NULL that is not nullable.  The
 * torrent-idle half of the tick is one comparison a torrent and stays with the caller. */
int krk_conn_preempt(const krk_conn_torrent* torrents, uint64_t n_torrents, const uint64_t* bits, const int64_t* created,
                     const int64_t* received, const int64_t* sent, int64_t now, int64_t conn_tti, int64_t conn_ttl,
                     uint64_t* close_out, uint32_t* n_close_out);
/* The same on the device (conn_round.hip), bit for bit; asynchronous on `stream`: one launch, one
 * workgroup a torrent, one lane a peer.  The arrays are device or page-locked host memory, the
 * 64-bit ones 8-byte and n_close_out 4-byte aligned; KRK_ENODEV without a gfx950 device. */
int krk_conn_preempt_dev(const krk_conn_torrent* torrents_host, uint64_t n_torrents, const uint64_t* bits_dev,
                         const int64_t* created_dev, const int64_t* received_dev, const int64_t* sent_dev, int64_t now,
                         int64_t conn_tti, int64_t conn_ttl, uint64_t* close_out, uint32_t* n_close_out, void* stream);

/* ------------------------------------------- re-piece stored MetaInfo, no blob read
 * The piece sums of a stored MetaInfo at a COARSER piece length, from the stored sums alone:
 * what a changed piece-length table (lib/metainfogen/config.go:48-80) asks of every
 * _torrentmeta in the cache, and overwriteMetaInfo(d, pieceLength)
 * (origin/blobserver/server.go:344-360) of one.  new_piece_length must be a multiple of
 * piece_length (splitting pieces needs the bytes and stays with Generate).  On finalised IEEE
 * sums crc(A || B) = shift(crc(A), |B|) ^ crc(B), shift(c, n) = c * x^(8n) mod P, so a new
 * piece's sum is the XOR over the old pieces it covers of their sums shifted to its end: bit-exact,
 * O(pieces), zero blob bytes.  The shift is a bijection, so a stored sum that was wrong stays
 * wrong in the coarse sum: re-piecing neither hides nor repairs rot (krk_verify_files is the
 * check).
 *
 * A blob reads krk_num_pieces(length, piece_length) sums at sums_offset and writes
 * krk_num_pieces(length, new_piece_length) sums at out_offset; length == 0 reads and writes
 * nothing; equal piece lengths copy; new_piece_length >= length > 0 gives one sum, the blob's
 * whole CRC-32.  Every output sum is stored by the call; the caller pre-zeroes nothing and words
 * between two blobs' ranges are not touched.  Refused before anything is written or launched:
 * KRK_EINVAL "piece length must be positive", "new piece length %lld is not a multiple of piece
 * length %lld", a negative length; krk_repiece_sums also KRK_EINVAL "%llu piece sums for %llu
 * pieces" and KRK_ERANGE when n_out is too small. */
typedef struct krk_repiece_blob {
    int64_t length, piece_length, new_piece_length;
    uint64_t sums_offset, out_offset;      /* into sums / out, in sums */
} krk_repiece_blob;
/* One blob; pure host code, no device. */
int krk_repiece_sums(const uint32_t* sums, uint64_t n_sums, int64_t length, int64_t piece_length,
                     int64_t new_piece_length, uint32_t* out, uint64_t n_out);
/* A batch on the host; no device. */
int krk_repiece_batch(const krk_repiece_blob* blobs, uint64_t n, const uint32_t* sums, uint32_t* out);
/* The same on the device (piece_repiece.hip, bit-identical to the host forms): sums_dev and
 * out_dev are device memory or page-locked host memory (krk_host_alloc); any other pointer is
 * KRK_EINVAL before anything is launched.  Asynchronous on `stream`: the descriptors are copied
 * into the library's staging before the call returns, so out_dev can feed
 * krk_info_hash_batch_dev on the same stream with no host step between.  n == 0 is KRK_OK;
 * KRK_ENODEV without a gfx950 device. */
int krk_repiece_batch_dev(const krk_repiece_blob* blobs_host, uint64_t n, const uint32_t* sums_dev,
                          uint32_t* out_dev, void* stream);

/* ------------------------------------------------- _torrentmeta JSON (Serialize / Deserialize)
 * MetaInfo.Serialize and DeserializeMetaInfo (core/metainfo.go:125-155): the sidecar's JSON,
 * byte for byte what json.Marshal(&metaInfoJSON{info}) emits --
 *   {"Info":{"PieceLength":I64,"PieceSums":ARR,"Name":"H64","Length":I64}}
 *   I64 = -?(0|[1-9][0-9]{0,18}) in int64 range, never "-0"
 *   ARR = null | [] | [U32(,U32)*]    U32 = 0|[1-9][0-9]{0,9}, <= 4294967295
 *   H64 = 64 hex digits, either case
 * with no whitespace and no trailing bytes: the canonical form.  The parser accepts exactly that
 * form; anything else -- valid JSON that encoding/json would still unmarshal included -- is
 * KRK_EFORMAT "metainfo json: not the canonical form at byte <i> of <n>" and belongs to the
 * caller's general decoder.  `null` (a nil slice) and `[]` (an empty one) stay distinct in both
 * directions.  The host forms need no device. */
/* An upper bound of a document's size that depends on the sum count alone. */
uint64_t krk_metainfo_json_bound(uint64_t n_sums);
/* The document of (piece_length, sums[0, n_sums), name, length) to out[0, *len); sums_null != 0
 * writes PieceSums as null (n_sums must be 0).  *len is the exact size whenever the arguments
 * are valid: cap < *len is KRK_ERANGE with nothing written.  A name that is not 64 hex digits
 * is KRK_EINVAL (its JSON escaping stays with the caller). */
int krk_metainfo_serialize(int64_t piece_length, const uint32_t* sums, uint64_t n_sums, int sums_null,
                           const char* name, uint64_t name_len, int64_t length, uint8_t* out, uint64_t cap,
                           uint64_t* len);
/* The four fields of a canonical document.  sums_cap >= (len + 1) / 2 always suffices; fewer
 * than *n_sums is KRK_ERANGE with *n_sums set.  On KRK_EFORMAT nothing is promised about the
 * outputs.  name_out receives the 64 name bytes as written (no terminator). */
int krk_metainfo_parse(const uint8_t* data, uint64_t len, int64_t* piece_length, uint32_t* sums_out,
                       uint64_t sums_cap, uint64_t* n_sums, int* sums_null, char name_out[64], int64_t* length);
/* The envelope alone, O(1) work a document: the header from the front, the fixed-form trailer
 * (,"Name":"...","Length":...}}) from the back, and [*arr_begin, *arr_end), the bytes strictly
 * between '[' and ']' (empty for [] and for null), which are NOT looked at: they are
 * krk_metainfo_parse_sums_batch_dev's part.  KRK_EFORMAT on any other envelope. */
int krk_metainfo_json_envelope(const uint8_t* data, uint64_t len, int64_t* piece_length, uint64_t* arr_begin,
                               uint64_t* arr_end, int* sums_null, char name_out[64], int64_t* length);
/* The same codec on the device (metainfo_json.hip), asynchronous on `stream`; the descriptors
 * are copied into the library's staging before a call returns.  Every device-side pointer is
 * device memory or page-locked host memory (krk_host_alloc): any other pointer is KRK_EINVAL
 * before anything is launched.  KRK_ENODEV without a gfx950 device; n == 0 is KRK_OK.
 *
 * Serialise: blob i's sums are sums_dev[sums_off, + n_sums); its document is stored at
 * out + out_off, a slot of at least krk_metainfo_json_bound(n_sums) bytes the caller chose, and
 * its exact size in out_len[i] (8-byte aligned).  Every byte of [out_off, out_off + out_len[i])
 * is stored by the call and no byte outside it is touched; nothing is pre-zeroed.  Bytes equal
 * to krk_metainfo_serialize's.  A name that is not 64 hex digits, or sums_null with n_sums != 0,
 * is KRK_EINVAL. */
typedef struct krk_metainfo_json_blob {
    uint64_t sums_off, n_sums;             /* into sums_dev, in sums */
    int64_t piece_length, length;
    uint64_t out_off;                      /* into out, in bytes */
    uint32_t sums_null, reserved;
    char name[64];
} krk_metainfo_json_blob;
int krk_metainfo_serialize_batch_dev(const krk_metainfo_json_blob* blobs_host, uint64_t n, const uint32_t* sums_dev,
                                     uint8_t* out, uint64_t* out_len, void* stream);
/* Parse: span i is text_dev[text_off, + text_len), the bytes krk_metainfo_json_envelope found
 * between the brackets (text_len == 0 for [] and for a null array, which bring no work);
 * expect_n is the number of sums it must hold, krk_num_pieces(length, piece_length) of the
 * envelope.  status[i] == 0 only if the span is canonical (U32(,U32)*, or empty) AND holds
 * exactly expect_n numbers; then sums_out[sums_off, + expect_n) are its values.  With a nonzero
 * status (bit 0: form, bit 1: count) those expect_n sums are unspecified; nothing outside them
 * is written either way, and the caller pre-zeroes nothing. */
typedef struct krk_metainfo_json_span {
    uint64_t text_off, text_len;           /* into text_dev, in bytes */
    uint64_t sums_off, expect_n;           /* into sums_out, in sums */
} krk_metainfo_json_span;
int krk_metainfo_parse_sums_batch_dev(const krk_metainfo_json_span* spans_host, uint64_t n, const uint8_t* text_dev,
                                      uint32_t* sums_out, uint32_t* status, void* stream);

/* ----------------------------------------------------- SHA-256 (Digester)
 * Replaces core.Digester (core/digester.go:28-72): crypto.SHA256 over the whole
 * blob.  One Merkle-Damgard stream per lane, many blobs per launch. */

/* Device-resident batch: data_dev[i] (device pointers, array itself on host),
 * lengths[i]; digests_dev receives n*32 bytes (device). Asynchronous. */
int krk_sha256_dev(const uint8_t* const* data_dev, const uint64_t* lengths, uint64_t n,
                   uint8_t* digests_dev, void* stream);

/* Device-resident batch hashed by host threads (x86 SHA extensions): up to `threads`
 * threads (<= 0: the CPUs this process may use) each read a blob out of device memory
 * through their own pinned double buffers, after the work queued on `stream` up to the
 * call; digests_host n*32 bytes.  Synchronous.  The host lane of a windowed batch
 * (kraken_amd/windowed.py): the longest chains of a larger-than-HBM batch hashed on the
 * host while the GPU windows run the rest. */
int krk_sha256_dev_on_host(const uint8_t* const* data_dev, const uint64_t* lengths, uint64_t n, int threads,
                           void* stream, uint8_t* digests_host);

/* Host batch: HOST data pointers; digests_host n*32 bytes.  Synchronous.  The window
 * schedule of krk_metainfo_digest_host without the piece CRCs (at most the window
 * stream cap of blobs live, admitted longest first; page-locked blobs DMA'd directly),
 * and the planner's blobs hashed in place on host threads under the default AUTO host
 * offload. */
int krk_sha256_host(const uint8_t* const* data_host, const uint64_t* lengths, uint64_t n,
                    uint8_t* digests_host);

/* Streaming Digester (core.NewDigester, digester.go:34): _write may be called any
 * number of times (io.Copy chunks); _sum does not reset (Digester.Digest(),
 * digester.go:41-48) so writing may continue afterwards.  One digester is
 * single-owner (like hash.Hash); different digesters may be used from different
 * threads at once.
 *
 * Placement, fixed at creation:
 *   KRK_PLACE_GPU   bytes go through the device's submission engine: the caller copies
 *                   them into pooled pinned slots (512 KiB) and every
 *                   pending slot of every GPU digester of the device is digested in
 *                   ONE multi-stream sha256_multi launch (a dispatcher thread batches
 *                   them).  A digester's midstate lives in an HBM row of the engine,
 *                   so its requests chain through the device in stream order and the
 *                   next launch is queued behind the running one (up to 8 requests
 *                   of a digester in flight; the kernel reads the pinned slots in
 *                   place).  Creation allocates nothing on the device.
 *   KRK_PLACE_HOST  SHA-NI on the caller's thread (host_meta.cpp): ~2 GB/s per stream
 *                   against ~59 MB/s for one GPU stream.
 *   KRK_PLACE_AUTO  (krk_digester_new) HOST while at most N digesters are live in the
 *                   process, GPU beyond.  N is the crossover computed from the calling
 *                   thread's device's planner rates: the fewest live GPU digesters whose
 *                   aggregate (live streams x the measured per-stream rate of the launch
 *                   plan they get, capped by what the engine's zero-copy slot reads carry:
 *                   0.58 x the measured pinned H2D rate) beats the host's (the process's CPU
 *                   budget x one thread's measured SHA-NI rate); never (all on the host) when
 *                   the host out-hashes that -- the case on MI355X boxes' 16-CPU shares
 *                   (measured: 32.7 GB/s at best on the GPU against 34-37 on the host).  KRK_DIGESTER_HOST_STREAMS or
 *                   krk_set_digester_host_streams pins N (-1 restores the default).
 * HOST placement needs no device; GPU placement without a gfx950 device is KRK_ENODEV and
 * AUTO without one is HOST (the product's own SHA-NI path, not the oracle). */
typedef struct krk_digester krk_digester;
#define KRK_PLACE_AUTO 0
#define KRK_PLACE_HOST 1
#define KRK_PLACE_GPU 2
int krk_digester_new(krk_digester** out);
int krk_digester_new_on(int placement, krk_digester** out);
int krk_digester_placement(const krk_digester* d, int* placement);
int krk_digester_write(krk_digester* d, const uint8_t* host_buf, uint64_t n);
int krk_digester_sum(krk_digester* d, uint8_t out32[32]);
void krk_digester_free(krk_digester* d);
int krk_set_digester_host_streams(int64_t n);

/* The slot pool's HARD cap on pinned staging bytes for the calling thread's device
 * (default KRK_SLOT_POOL_MB = 4096 MiB; at least one 16-slot chunk).  At the cap a
 * writer waits for a slot to come back (backpressure) instead of pinning more: slots
 * are held only by requests in flight, never by an idle digester or piece stream (their
 * partial data stays in their own host buffer).  Lowering the cap frees nothing already
 * pinned.  bytes == 0 only reads: *cap_out = the cap, *waits_out = how many times a
 * writer waited at it (either may be NULL). */
int krk_engine_set_pool_cap(uint64_t bytes, uint64_t* cap_out, uint64_t* waits_out);

/* ----------------------------------------- metainfo + digest (batch)
 * Both products for every blob in one call: the Digester SHA-256 of
 * uploader.verify (origin/blobserver/uploader.go:74-94) and the piece sums of
 * Generate (lib/metainfogen/generator.go:41-58).  The SHA and CRC kernels run
 * concurrently on two internal streams joined back into `stream`.  Device
 * pointers; asynchronous.  As with krk_piece_sums_dev, a call owns the span of sums_dev from
 * its lowest sums_offset to its highest end (gaps inside it come back zero): give each call
 * its own span. */
int krk_metainfo_digest_dev(const krk_blob* blobs, uint64_t n_blobs, uint32_t* sums_dev,
                            uint8_t* digests_dev, void* stream);

/* Chunked (streaming) form on device data: each call advances every listed blob
 * by one chunk -- SHA-256 from the blob's midstate in state_dev (8 words per
 * blob slot, written back), CRC-32 of the chunk's byte range XOR-accumulated
 * into its pieces' sums (sums_dev must be zero before a blob's first chunk).
 * A blob's chunks are submitted in order, one per call; every chunk but the
 * last is a multiple of 64 bytes; the chunk that reaches blob_length writes
 * the digest to digests_dev[32*blob].  This is the multi-blob Digester.Write +
 * calcPieceSums step that end-to-end and larger-than-HBM batches (C3) run
 * window by window.  Asynchronous on `stream`. */
typedef struct krk_chunk {
    const uint8_t* data;     /* device pointer to the chunk's bytes */
    uint64_t offset;         /* chunk's first byte inside its blob */
    uint64_t length;         /* chunk bytes */
    uint64_t blob_length;    /* total blob length */
    int64_t piece_length;    /* > 0 */
    uint64_t sums_offset;    /* blob's first piece-sum slot */
    uint64_t blob;           /* blob slot for state_dev / digests_dev */
} krk_chunk;
int krk_metainfo_digest_chunks_dev(const krk_chunk* chunks, uint64_t n_chunks, uint32_t* state_dev,
                                   uint32_t* sums_dev, uint8_t* digests_dev, void* stream);
/* The same with the SHA-256 launch on `sha_stream` (NULL: the library's own), forked from
 * and joined back into `stream` like the default; with a sha_stream the piece CRCs run on
 * `stream` itself (no barrier of the step on the library's streams).  A caller that runs D2H copies beside
 * the windows (the C3 host lane, kraken_amd/windowed.py) passes a stream of another
 * priority (krk_stream_create_prio): streams of one priority share the device's few
 * hardware queues, and a copy queued behind a window's ~0.6 s SHA-256 launch on a shared
 * queue waits for it. */
int krk_metainfo_digest_chunks_dev_on(const krk_chunk* chunks, uint64_t n_chunks, uint32_t* state_dev,
                                      uint32_t* sums_dev, uint8_t* digests_dev, void* stream, void* sha_stream);

/* End-to-end form: blobs[i].data are HOST pointers (pageable or pinned).  Every
 * byte crosses PCIe once, window by window, and both kernels run on each window
 * (SHA-256 chained from per-blob midstates, CRC by byte range) while the next window
 * goes up.  How a window goes up: page-locked blobs (krk_host_alloc) by one DMA a chunk
 * (few wide chunks) or one gather launch that reads the caller's pages over PCIe, so each
 * byte is read from host memory once, by the GPU; pageable blobs are copied by host threads
 * into the library's pinned windows first (measured faster than registering the caller's
 * 4 KiB pages for the gather, which KRK_HOST_GATHER=1 still does).  Allocate receive buffers
 * with krk_host_alloc to get the one-read path.  sums_host indexed by blobs[i].sums_offset;
 * digests_host n_blobs*32 bytes.  Synchronous. */
int krk_metainfo_digest_host(const krk_blob* blobs, uint64_t n_blobs, uint32_t* sums_host,
                             uint8_t* digests_host);

/* The same from the CAS files themselves: the upload verify of uploader.verify
 * (origin/blobserver/uploader.go:74-94) or the cache-fill digest of CAStore.WriteCacheFile
 * (lib/store/ca_store.go:99-135) fused with the metainfo Generator.Generate computes from the
 * cache file (lib/metainfogen/generator.go:41-58): each file is read ONCE (pread on the host
 * pool into the pinned windows; O_DIRECT for a cold batch, below) and that read feeds both
 * the SHA-256 digest and the piece CRCs -- the reference reads it twice.  files[i].length is
 * the size the caller stat-ed; a shorter file is KRK_EIO "read blob: <path>: unexpected EOF",
 * an unopenable one KRK_EIO "open <path>: <errno text>".  Live blobs per window are also
 * capped by the file descriptors the process may still open (RLIMIT_NOFILE).  With the host
 * offload (KRK_OFFLOAD_AUTO) the planner's files are read, hashed and piece-summed on host
 * threads in one pass each -- unless a sample of the files (mmap + mincore, no reads) finds
 * them mostly outside the page cache: a disk-bound batch stays on the windows and is read
 * O_DIRECT through Linux AIO (one thread queues a window's chunks; KRK_FILE_DIRECT=1/0
 * forces O_DIRECT on/off).  KRK_FILE_READAHEAD_MB=N keeps each file hinted N MiB ahead of
 * its page-cache reads (POSIX_FADV_WILLNEED; off by default).  Synchronous. */
int krk_metainfo_digest_files(const krk_file_blob* files, uint64_t n_files, uint32_t* sums_host,
                              uint8_t* digests_host);

/* ------------------------------------------------------- multi-device
 * One process, several GPUs (the origin is one process,
 * origin/cmd/cmd.go:164).  The device set -- the devices of the last krk_init mask,
 * or krk_set_devices (a device may repeat: several workers on one GPU), default the
 * calling thread's device -- is where the *_multi calls run and where new Digesters
 * and piece streams are placed (round-robin).  A *_multi call splits its batch by
 * bytes (LPT: the longest blob to the least-loaded device), runs the single-device
 * entry point on every device from its own host thread and gathers the results
 * into the caller's arrays (same layout as the single-device call).  No collective:
 * blobs are independent.  Synchronous. */
int krk_set_devices(const int* devs, uint32_t n);
int krk_get_devices(int* devs, uint32_t cap, uint32_t* n);
int krk_metainfo_digest_host_multi(const krk_blob* blobs, uint64_t n_blobs, uint32_t* sums_host,
                                   uint8_t* digests_host);
int krk_piece_sums_host_multi(const krk_blob* blobs, uint64_t n_blobs, uint32_t* sums_host);
int krk_piece_sums_files_multi(const krk_file_blob* files, uint64_t n_files, uint32_t* sums_host);
int krk_metainfo_digest_files_multi(const krk_file_blob* files, uint64_t n_files, uint32_t* sums_host,
                                    uint8_t* digests_host);
int krk_sha256_host_multi(const uint8_t* const* data_host, const uint64_t* lengths, uint64_t n,
                          uint8_t* digests_host);

/* ---------------------------------------------------- InfoHash (host CPU)
 * info.Hash() (core/metainfo.go:37-44): SHA-1 over the bencoded
 * info{PieceLength, PieceSums, Name, Length}.  bencode_out may be NULL. */
int krk_info_hash(int64_t piece_length, const uint32_t* sums, uint64_t n_sums,
                  const char* name, uint64_t name_len, int64_t length, uint8_t out20[20]);
/* Batch form for many blobs (Generator.Generate over a batch, whole-CAS regen):
 * blob i has piece_lengths[i], sums[sums_off[i] .. sums_off[i] + n_sums[i]), name
 * names[name_off[i] .. name_off[i+1]), length lengths[i]; out20 receives 20*n bytes.
 * Spread over host threads.  names may be NULL when every name is empty. */
/* Generator.Generate over device-resident blobs (lib/metainfogen/generator.go:41-58 ->
 * core.NewMetaInfo, core/metainfo.go:53-79): every blob's piece sums (sums_dev, also
 * copied to sums_host at blobs[i].sums_offset) and its InfoHash (info_hash20, 20 B a
 * blob; names/name_off = the blobs' digest hex, the info Name).  The batch runs as up to
 * 8 groups of about equal bytes back to back on `stream`; each group's sums are copied
 * back and hashed on host threads while the later groups' kernels run.  Synchronous.
 * With the InfoHash placed on the device (krk_set_info_hash_placement below) the hashes come
 * from krk_info_hash_batch_dev's kernel instead and no host thread is started. */
int krk_metainfo_batch_dev(const krk_blob* blobs, uint64_t n_blobs, const char* names, const uint64_t* name_off,
                           uint32_t* sums_dev, uint32_t* sums_host, uint8_t* info_hash20, void* stream);
int krk_info_hash_batch(const int64_t* piece_lengths, const uint32_t* sums, const uint64_t* sums_off,
                        const uint64_t* n_sums, const char* names, const uint64_t* name_off,
                        const int64_t* lengths, uint64_t n, uint8_t* out20);
int krk_bencode_info(int64_t piece_length, const uint32_t* sums, uint64_t n_sums,
                     const char* name, uint64_t name_len, int64_t length,
                     uint8_t* out, uint64_t cap, uint64_t* written);
/* krk_info_hash_batch on the device, from piece sums already in device memory: the same
 * arguments and the same 20 bytes a blob, with sums_dev device memory and out20 device memory
 * or page-locked host memory (krk_host_alloc; as krk_ring_locations_dev: any other pointer is
 * KRK_EINVAL).  One wave a blob formats the bencoding into an on-chip ring and hashes it from
 * there; the text never exists in memory.  Asynchronous on `stream`: every host array (names
 * included) is copied into the library's staging before the call returns, so the caller may
 * overwrite them at once; out20 is valid once the stream reaches the call's end.  names may be
 * NULL when every name is empty; n == 0 is KRK_OK; KRK_ENODEV without a gfx950 device. */
int krk_info_hash_batch_dev(const int64_t* piece_lengths, const uint32_t* sums_dev, const uint64_t* sums_off,
                            const uint64_t* n_sums, const char* names, const uint64_t* name_off,
                            const int64_t* lengths, uint64_t n, uint8_t* out20, void* stream);
/* Where krk_metainfo_batch_dev (and nothing else) computes its InfoHashes, process-wide:
 * KRK_PLACE_HOST (each group's sums copied back and hashed on host threads while later
 * groups' kernels run), KRK_PLACE_GPU (krk_info_hash_batch_dev's kernel behind the piece-sum
 * launches on the library's streams; the sums and the hashes copied back once, no host thread
 * started) or KRK_PLACE_AUTO, the default, which for now means KRK_PLACE_HOST.  The
 * environment variable KRK_INFOHASH_PLACEMENT (0/1/2), read once, sets the same; a call wins
 * over it.  Another value is KRK_EINVAL.  krk_info_hash_placement reports the setting. */
int krk_set_info_hash_placement(int placement);
int krk_info_hash_placement(int* placement);

/* pieceLengthConfig.get (lib/metainfogen/config.go:71-80); thresholds ascending. */
int64_t krk_piece_length_for_size(const int64_t* thresholds, const int64_t* lengths,
                                  uint32_t n, int64_t size);

/* -------------------------------------------------------- HRW placement
 * Replaces hrw.RendezvousHash.GetOrderedNodes / RendezvousHashNode.Score
 * (lib/hrw/rendezvous.go:151-217) with murmur3.New64 + UInt64ToFloat64
 * (rendezvous.go:39,99-118), and hashring.ring.Locations (lib/hashring/ring.go:96-118).
 * Keys are hex strings (hex-decoded, then key||label is hashed).  Order is
 * descending score; exact ties go to the lower node index (the reference's
 * tie order is unspecified: Go map order, ring.go:151). */

typedef struct krk_nodes {
    const char* labels;          /* concatenated label bytes */
    const uint64_t* label_off;   /* n_nodes + 1 offsets into labels */
    const int64_t* weights;      /* n_nodes (ring nodes use 100, ring.go:28) */
    uint32_t n_nodes;
} krk_nodes;

/* keys: concatenated hex strings with key_off (n_keys+1).  order_out:
 * n_keys * n_out node indices (-1 padded when n_out > n_nodes); scores_out
 * (nullable): n_keys * n_nodes, in node order -- also with n_out == 0, which asks for
 * scores alone.  Returns KRK_EHEX if any key is not valid hex (its row is then filled
 * from NaN scores: node order).  n_nodes of 0 or above 4096 and n_out above 4096 are
 * KRK_EINVAL, refused before anything is launched or written. */
int krk_hrw_ordered(const char* keys, const uint64_t* key_off, uint64_t n_keys,
                    const krk_nodes* nodes, uint32_t n_out, int32_t* order_out,
                    double* scores_out);

/* hrw.UInt64ToFloat64 (rendezvous.go:99-118) with MaxHashValue = 8 x 0xFF (murmur3's
 * Sum size): sums8 holds n 8-byte big-endian hash Sums; out[i] = low 53 bits / 2^53,
 * where all-zero low bits are re-hashed once with murmur3.New64 when rehash != 0 (the
 * hasher argument; 0 = nil hasher).  Runs the scoring kernel's own device function. */
int krk_hrw_uint64_to_float64(const uint8_t* sums8, uint64_t n, int rehash, double* out);

/* ring.Locations for raw 32-byte sha256 digests (ShardID = first 2 bytes).
 * healthy: n_nodes flags.  locs_out: n * max(1, max_replica) node indices
 * (-1 padded); counts_out: n entries.  Counts are one byte: a ring whose shards can have
 * more than 255 owners, min(max_replica, n_nodes) > 255, is KRK_ERANGE, refused before
 * anything is launched or written (300 nodes with max_replica 255 are served). */
int krk_ring_locations(const uint8_t* digests32, uint64_t n, const krk_nodes* nodes,
                       const uint8_t* healthy, int32_t max_replica,
                       int32_t* locs_out, uint8_t* counts_out);
/* The whole ring in one call: Locations(d) depends on d only through ShardID =
 * hex[:4] (core/digest.go:148-150), so the 65,536 possible owner lists are computed
 * once per membership or health change (ring.Refresh, lib/hashring/ring.go:141-165)
 * and Locations becomes a host lookup: row ((d[0] << 8) | d[1]) of locs_out
 * (65,536 x max(1, max_replica) node indices, -1 padded) with counts_out[row] valid
 * entries.  Same semantics as krk_ring_locations, KRK_ERANGE for
 * min(max_replica, n_nodes) > 255 included. */
int krk_ring_owner_table(const krk_nodes* nodes, const uint8_t* healthy, int32_t max_replica,
                         int32_t* locs_out, uint8_t* counts_out);
/* Device-resident form (digests in device memory).  The owner table of a membership
 * (labels, weights, healthy, max_replica) is built on its first call and kept (8
 * memberships a device, least recently used replaced), as the reference's Ring keeps its
 * hrw until Refresh; later calls only gather.  locs/counts: device memory, or page-locked
 * host memory (krk_host_alloc) that the gather writes over PCIe -- the owner lists are on
 * the host when the stream reaches the call's end, with no copy-back; any other pointer is
 * KRK_EINVAL.  min(max_replica, n_nodes) > 255 is KRK_ERANGE (8-bit counts, as
 * krk_ring_locations), refused before any table is built or output written. */
int krk_ring_locations_dev(const uint8_t* digests32_dev, uint64_t n, const krk_nodes* nodes,
                           const uint8_t* healthy, int32_t max_replica,
                           int32_t* locs_dev, uint8_t* counts_dev, void* stream);
/* Compact form for rings of <= 255 nodes (KRK_ERANGE beyond): owner indices as
 * uint8 (0xFF padded), a quarter of the bytes the caller copies back.  Same
 * ring.Locations semantics (lib/hashring/ring.go:91-118) as krk_ring_locations_dev, its
 * KRK_ERANGE for min(max_replica, n_nodes) > 255 included. */
int krk_ring_locations_u8_dev(const uint8_t* digests32_dev, uint64_t n, const krk_nodes* nodes,
                              const uint8_t* healthy, int32_t max_replica,
                              uint8_t* locs_dev, uint8_t* counts_dev, void* stream);

/* Ring ownership as bitsets: which of these blobs belong on this origin, and which change
 * hands when the ring changes.  forceCleanupHandler -> maybeDelete
 * (origin/blobserver/server.go:686-759) asks owns = stringset.FromSlice(hashRing.Locations(d))
 * .Has(s.addr) of every cache file and deletes on expired || !owns; applyToReplicas
 * (server.go:426-454) asks the same set question a blob.  Locations(d) depends on d only
 * through its ShardID, so every such question is a 65,536-bit shard predicate: a mask of 1,024
 * uint64 words, shard s = bit (s & 63) of word (s >> 6), built on the host from the tables
 * krk_ring_owner_table returns (65,536 rows of `row` indices, counts[s] valid ones) and
 * applied to n digests by krk_ring_select / krk_ring_select_dev: 1/8 byte a digest plus 8
 * bytes a selected one, against the max(1, MaxReplica) + 1 bytes of krk_ring_locations_u8_dev.
 * No device is needed for the masks or for krk_ring_select.
 *
 * krk_ring_mask_owns: mask[s] = node is one of Locations(s) (server.go:686-759 `owns`;
 * "gained" / "lost" of a node between two memberships are owns_B & ~owns_A and its mirror).
 * krk_ring_mask_moved: mask[s] = the owner SETS of s differ between membership A and B (sets,
 * as maybeDelete and applyToReplicas use stringset, server.go:426-454: order is ignored).
 * b_to_a[j] = the index in A of B's node j, -1 for a node A does not have; NULL = the same node
 * list (only health or MaxReplica changed).  A NULL pointer, row == 0, a count above its row or
 * a B owner outside [0, n_nodes_b) is KRK_EINVAL, refused before mask_out is touched. */
int krk_ring_mask_owns(const int32_t* locs, const uint8_t* counts, uint32_t row, int32_t node,
                       uint64_t* mask_out);
int krk_ring_mask_moved(const int32_t* locs_a, const uint8_t* counts_a, uint32_t row_a,
                        const int32_t* locs_b, const uint8_t* counts_b, uint32_t row_b,
                        const int32_t* b_to_a, uint32_t n_nodes_b, uint64_t* mask_out);
/* A mask applied to n raw 32-byte digests (server.go:686-759 over ListCacheFiles(), 426-454
 * over a batch): sel(i) = (mask[ShardID(d_i)] ^ (invert != 0)) | or_bits[i].  or_bits
 * (nullable) is n bits in the bitset layout -- the `expired` half of expired || !owns.
 * bits_out: krk_bitfield_words(n) words, bit (i & 63) of word (i >> 6) = sel(i), the last
 * word's tail bits 0, every word stored.  *count_out = the selected digests, always written
 * (0 for n == 0).  idx_out (nullable; then idx_cap must be 0) receives the first
 * min(count, idx_cap) selected i in ascending order -- the reference's `deleted` list is in
 * listing order -- and nothing past them: count > idx_cap says the list is truncated. */
int krk_ring_select(const uint8_t* digests32, uint64_t n, const uint64_t* mask, int invert,
                    const uint64_t* or_bits, uint64_t* bits_out, uint64_t* idx_out, uint64_t idx_cap,
                    uint64_t* count_out);
/* The same for digests in device memory (any byte alignment), bit for bit (server.go:686-759,
 * 426-454).  or_bits_dev, bits_out, idx_out and count_out are device memory or page-locked
 * host memory (krk_host_alloc; as krk_ring_locations_dev the results are then on the host when
 * the stream reaches the call's end) and 8-byte aligned: any other pointer is KRK_EINVAL before
 * anything is launched.  mask_host is copied into the library's staging before the call
 * returns; the call is asynchronous on `stream`.  KRK_ENODEV without a gfx950 device. */
int krk_ring_select_dev(const uint8_t* digests32_dev, uint64_t n, const uint64_t* mask_host, int invert,
                        const uint64_t* or_bits_dev, uint64_t* bits_out, uint64_t* idx_out,
                        uint64_t idx_cap, uint64_t* count_out, void* stream);

/* ------------------------------------- cleanup plans from a raw cache listing
 * A cache listing is hex names and mtimes, not raw digests and a ready `expired` bitset: the
 * SHA-256 hex codec (core.NewSHA256DigestFromHex / ValidateSHA256 / Digest.Hex(),
 * core/digest.go:57-68,143-161), the expiry comparison of maybeDelete
 * (origin/blobserver/server.go:686-759) and of the store's TTL/TTI rule readyForDeletion
 * (lib/store/cleanup.go:112-155, with its _last_access_time sidecar,
 * lib/store/metadata/last_access_time.go:55-70), and the two fused with the ring selection.
 *
 * Listing layout (the names / name_off convention of krk_metainfo_batch_dev): `names` is bytes
 * back to back, `off` is n + 1 uint64 values, name i is names[off[i], off[i+1]); off[0] need not
 * be 0.  A name's length is the unsigned 64-bit difference off[i+1] - off[i]; any value but 64
 * is a length error and no byte of that name is read.  Then the 32 pairs are decoded in index
 * order, either case accepted; the first byte, in index order, that is not [0-9a-fA-F] is the
 * error (encoding/hex's InvalidByteError).  One status word a name:
 *   0                                        valid
 *   KRK_DHEX_LEN | min(len, 0x3FFFFFFF)      len != 64
 *   KRK_DHEX_BYTE | p << 8 | byte            bad byte at position p (0..63)
 * An invalid name's digest is 32 zero bytes (every output byte is stored) and its bit in the
 * `valid` bitset is 0; the bitset has krk_bitfield_words(n) words in the layout above, tail bits
 * 0, every word stored.  Times are int64 nanoseconds; expired(now, t, d) = sat_sub(now, t) > d,
 * the subtraction saturating at the int64 limits as time.Time.Sub does, the comparison strict. */
#define KRK_DHEX_LEN 0x40000000u
#define KRK_DHEX_BYTE 0x80000000u
#define KRK_NO_TIME INT64_MIN   /* a missing _last_access_time */
/* Host forms; no device.  status_out and valid_out may be NULL. */
int krk_digest_parse_hex(const uint8_t* names, const uint64_t* off, uint64_t n, uint8_t* digests32_out,
                         uint32_t* status_out, uint64_t* valid_out);
/* Digest.Hex(): 64 lowercase characters a digest at stride 64, no terminator. */
int krk_digest_format_hex(const uint8_t* digests32, uint64_t n, uint8_t* hex_out);
/* bit i = (mtime_ns && expired(now, mtime_ns[i], ttl)) ||
 *         (atime_ns && atime_ns[i] != KRK_NO_TIME && expired(now, atime_ns[i], tti));
 * either column may be NULL.  maybeDelete passes mtime only; cleanup.go's scan passes mtime only
 * when ttl > 0, together with the access-time column.  krk_bitfield_words(n) words, tail bits 0. */
int krk_expiry_bits(const int64_t* mtime_ns, const int64_t* atime_ns, uint64_t n, int64_t now_ns,
                    int64_t ttl_ns, int64_t tti_ns, uint64_t* bits_out);
/* maybeDelete over ListCacheFiles() from the listing itself:
 *   sel(i) = valid(i) & ((mask[ShardID(d_i)] ^ (invert != 0)) | expired(now, mtime_ns[i], ttl)).
 * mtime_ns may be NULL: no expiry term (a krk_ring_mask_moved mask then answers "which names of
 * this listing change hands").  An invalid name is never selected.  bits_out, idx_out, idx_cap
 * and count_out as krk_ring_select: ascending listing positions (positions in the listing
 * itself: no compaction, no mapping back), truncation reported by count > idx_cap, the count
 * always stored.  valid_out may be NULL.  A NULL argument that is not nullable, or idx_out NULL
 * with idx_cap != 0, is KRK_EINVAL before any output is touched. */
int krk_cleanup_plan(const uint8_t* names, const uint64_t* off, uint64_t n, const int64_t* mtime_ns,
                     int64_t now_ns, int64_t ttl_ns, const uint64_t* mask, int invert, uint64_t* bits_out,
                     uint64_t* valid_out, uint64_t* idx_out, uint64_t idx_cap, uint64_t* count_out);
/* The same on the device (digest_hex.hip), byte for byte and bit for bit; asynchronous on
 * `stream`.  Every device-side pointer is device memory or page-locked host memory
 * (krk_host_alloc); off, mtime, valid, bits, idx and count 8-byte aligned, status 4-byte aligned;
 * anything else is KRK_EINVAL before anything is launched.  Names start at any byte alignment and
 * no byte outside names[off[0], off[n]) is read; digests32_dev and hex_dev may have any
 * alignment; all offsets are 64-bit.  status_dev, valid_dev, mtime_ns_dev and valid_out may be
 * NULL.  mask_host is copied into the library's staging before the call returns.  KRK_ENODEV
 * without a gfx950 device: there is no fall-back to the host forms. */
int krk_digest_parse_hex_dev(const uint8_t* names_dev, const uint64_t* off_dev, uint64_t n,
                             uint8_t* digests32_dev, uint32_t* status_dev, uint64_t* valid_dev, void* stream);
int krk_digest_format_hex_dev(const uint8_t* digests32_dev, uint64_t n, uint8_t* hex_dev, void* stream);
int krk_cleanup_plan_dev(const uint8_t* names_dev, const uint64_t* off_dev, uint64_t n,
                         const int64_t* mtime_ns_dev, int64_t now_ns, int64_t ttl_ns, const uint64_t* mask_host,
                         int invert, uint64_t* bits_out, uint64_t* valid_out, uint64_t* idx_out,
                         uint64_t idx_cap, uint64_t* count_out, void* stream);

/* ------------------------------------------------ device memory helpers
 * For callers (benchmarks, cgo) that do not own a device allocator. */
int krk_dev_alloc(uint64_t bytes, void** out);
int krk_dev_free(void* p);
/* Pinned (page-locked) host memory: what a cgo caller reads files / receives
 * pieces into so that the host entry points DMA it without a staging copy, and
 * where device results are gathered at full PCIe rate. */
int krk_host_alloc(uint64_t bytes, void** out);
int krk_host_free(void* p);
int krk_memcpy_h2d(void* dst_dev, const void* src_host, uint64_t n);
int krk_memcpy_d2h(void* dst_host, const void* src_dev, uint64_t n);
/* Queued on `stream` (NULL = the library's stream): dst_host should be pinned
 * (krk_host_alloc) for the copy to overlap the host. */
int krk_memcpy_d2h_async(void* dst_host, const void* src_dev, uint64_t n, void* stream);
int krk_stream_create(void** out);
/* A stream of the given priority: -1 high, 0 normal, 1 low (HIP's priority range).
 * Streams of another priority run on hardware queues of their own: a stream that holds
 * long kernels (a C3 window's SHA-256 launch runs ~0.6 s) is kept off the queues the
 * short work shares, which would otherwise wait behind it. */
int krk_stream_create_prio(int priority, void** out);
/* Waits for the stream's work, retires the library's state tied to it (events of upload
 * slots and scratch blocks last used on it), then destroys it.  Streams handed to the
 * library must be destroyed here, not with hipStreamDestroy. */
int krk_stream_destroy(void* s);
int krk_stream_sync(void* s);
/* Events (a window loop waits for ONE earlier window's kernels while the next
 * window's are already queued behind them on the same stream).  No timing; a thread in
 * krk_event_sync sleeps until the event completes rather than spinning a core. */
int krk_event_create(void** out);
int krk_event_record(void* ev, void* stream);
int krk_event_sync(void* ev);
int krk_event_destroy(void* ev);

/* Host offload of the longest SHA-256 chains, process-wide.  krk_sha256_dev and
 * krk_metainfo_digest_dev hand the longest blobs of a batch to host threads (x86 SHA
 * extensions, ~2 GB/s a thread against ~59 MB/s a GPU stream), which read them from device
 * memory through pinned double buffers while the GPU hashes the rest and every blob's piece
 * CRCs; the digests land in digests_dev as before.  How many go to the host minimises
 * max(GPU time, host time) at the planner's measured rates (krk_planner_rates_get) and is 0
 * unless that shortens the batch by 10 %: a single 1 GiB blob (C1) goes to the host.  When
 * whole blobs cannot shorten it -- 1,000 equal 100 MiB blobs (C2) each take the GPU ~1.8 s
 * wherever the others run -- every chain starts on the GPU and host threads take over the
 * tails of the longest ones from the GPU's midstate, each as soon as the GPU has reached its
 * planned split (tail handoff, when the model ends the batch 5 % sooner; KRK_SHA_TAIL=0
 * off): C2 1.42 s a batch against 1.77.  The call then returns after the host part is
 * hashed (the GPU part stays asynchronous on `stream`; with tail handoff, once the SHA-256
 * launch has ended too).  The host-buffer entry points work
 * on their offloaded blobs in place and never upload them: krk_sha256_host hashes them,
 * krk_metainfo_digest_host hashes them AND computes their piece sums (the SHA-256 pass and
 * the CRC pass of a blob are separate host tasks), so the bytes that cross the host link
 * shrink by theirs (the threshold there is 3 %).
 * threads: KRK_OFFLOAD_AUTO (-1, the default) = the process's host CPU budget (the node's
 * CPUs -- affinity capped by the cgroup quota -- divided among the LOCAL_WORLD_SIZE ranks of
 * a node, or KRK_HOST_CPUS) for device-resident batches and a quarter of them for
 * host-resident batches (whose staging windows need the rest as copy threads); 0 = off
 * (every chain on the GPU); n = up to n threads. */
#define KRK_OFFLOAD_AUTO (-1)
int krk_set_sha_host_offload(int threads);
int krk_sha_host_offload(int* threads);      /* the current setting */
/* The rates the planners use (the offload of the batch entry
 * points, the host/GPU split of the CRC-only host entry points), per device:
 * sha_stream_bps = one SHA-256 stream's rate at full residency under each AUTO tier
 * (eight lanes up to 16 x CUs streams, two lanes up to 64 x CUs, one lane beyond),
 * pinned D2H / H2D copy rates, one host thread's SHA-256, CRC-32 and memcpy rates.  Measured on
 * the calling thread's device at first use (~50 ms: each tier's launch plan timed on
 * 16 / 64 / 128 x CUs streams, a 64 MiB pinned copy each way); without a device the
 * nominal MI355X figures (source 0).  (kraken_hip_internal.h: krk_planner_rates_set
 * overrides them for tests, krk_host_offload_plan shows a plan without device work.) */
#define KRK_RATES_NOMINAL 0
#define KRK_RATES_MEASURED 1
#define KRK_RATES_SET 2
typedef struct krk_planner_rates {
    double sha_stream_bps[3];
    double d2h_bps, h2d_bps;
    double host_sha_bps, host_crc_bps, host_copy_bps;
    int32_t cus;
    int32_t source;
} krk_planner_rates;
int krk_planner_rates_get(krk_planner_rates* out);
/* Measure the calling thread's device's rates now (krk_init does it for its devices, so that
 * the measurement runs before the library has work of its own on them; otherwise the first
 * planner use measures).  Re-measure after a change of load the planners should see. */
int krk_planner_calibrate(void);

#ifdef __cplusplus
}
#endif
#endif /* KRAKEN_HIP_H */
