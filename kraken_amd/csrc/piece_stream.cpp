// piece_stream.cpp -- krk_piece_stream_* and krk_crc32_update*: the CRC-only streaming
// calls (NewMetaInfo over an io.Reader, PieceHash) and where they run.
//
// On the GPU placement each request's piece portions are hashed as independent messages
// (engine.cpp) and the owner's piece sums are folded on the completer thread with the GF(2)
// combine crc(A||B) = crc(A) * x^(8|B|) ^ crc(B) (crc_math.hpp), in submission order, so a
// stream's piece end need not be known when its bytes are submitted.  crc32.Update calls of
// at most KRK_CRC_HOST_MAX bytes run on the caller's thread (no PCIe round trip for a small
// write); product code (host_meta.cpp).
#include "engine.hpp"
#include "engine_math.hpp"
#include "offload.hpp"

using namespace krk;

struct krk_piece_stream {
    Owner o;  // o.E null: host placement
    uint64_t P = 0;
    uint64_t submitted = 0;       // stream bytes consumed (host) / handed to the engine (GPU)
    std::vector<uint32_t> sums;   // GPU: folded on the completer thread, in submission order
    // host placement: crc32.Update value of the current piece, bytes of it seen
    uint32_t crc = 0;
    uint64_t in_piece = 0;
    // GPU placement
    std::unique_ptr<uint8_t[]> pend;  // bytes not yet submitted
    size_t fill = 0;
    std::atomic<bool> fold_stop{false};    // completer thread: a request failed or broke the order, stop folding
    std::atomic<bool> fold_broken{false};  // completer thread: a continuation arrived with no start
};

namespace krk {
namespace {

// ------------------------------------------------------- CRC placement
// A piece stream (NewMetaInfo over an io.Reader) and a crc32.Update call (PieceHash) carry
// no state the GPU could keep: every byte crosses the host link once, copied into a pinned
// slot by the caller's thread first.  Measured on MI355X (tests/native/crc_crossover.cpp,
// profiles/r04/crc_crossover.jsonl): the engine's CRC side carries 10 GB/s for one stream
// and ~20 GB/s for 4 to 64 (slot copies and per-slot H2D), where the host placement --
// PCLMUL on the caller's thread, large writes shared with idle host-pool threads -- carries
// 60-80 GB/s for one stream and well over 100 GB/s for several.  So AUTO keeps CRC work on
// the host unless the host's whole CRC capacity (the CPUs this process may use x one thread's
// PCLMUL rate) is below what the host link could carry to the GPU at best (0.85 x the
// measured pinned H2D rate): a box with few or slow cores.
std::atomic<int> g_crc_placement{KRK_PLACE_AUTO};  // krk_set_crc_placement / KRK_CRC_PLACEMENT

int crc_placement_setting() {
    static std::once_flag once;
    std::call_once(once, [] {
        if (const char* e = KRK_OP_ENV("KRK_CRC_PLACEMENT")) {
            const int v = atoi(e);
            if (v >= KRK_PLACE_AUTO && v <= KRK_PLACE_GPU) g_crc_placement.store(v);
        }
    });
    return g_crc_placement.load(std::memory_order_relaxed);
}

// AUTO: true = this stream / call goes to the GPU engine (a device being present).
bool crc_auto_gpu() {
    int drc = KRK_OK;
    Device* D = device(&drc);
    if (!D) return false;
    const Rates R = planner_rates(D);
    return (double)host_threads() * R.host_crc < host_link(R);
}

}  // namespace

// The placement a new piece stream / crc32_update call runs on (runtime.hpp: the file and
// host-buffer CRC calls resolve theirs the same way): HOST or GPU.  `placement`
// KRK_PLACE_AUTO follows the process setting, then the crossover; GPU needs a gfx950
// device (KRK_ENODEV), AUTO without one is HOST.
int resolve_crc_placement(int placement, int* rc) {
    *rc = KRK_OK;
    const bool asked_auto = placement == KRK_PLACE_AUTO;
    if (asked_auto) placement = crc_placement_setting();
    const bool forced = placement != KRK_PLACE_AUTO;  // explicit, or the process setting
    if (placement == KRK_PLACE_AUTO) placement = crc_auto_gpu() ? KRK_PLACE_GPU : KRK_PLACE_HOST;
    if (placement == KRK_PLACE_GPU) {
        int drc = KRK_OK;
        if (!device(&drc)) {
            if (forced) {
                *rc = drc;
                return -1;
            }
            return KRK_PLACE_HOST;
        }
    }
    return placement;
}

namespace {

// Fold a request's portion CRCs into the stream's piece sums (completer thread, the
// stream's requests in submission order).  Once a request has failed, later ones are
// not folded: a portion that continues a piece begun in the failed request would index
// a sum that was never written.
void stream_fold(Req* r) {
    auto* s = static_cast<krk_piece_stream*>(r->ctx);
    if (s->fold_stop) return;
    if (r->rc) {  // the owner sees r->rc when it drains r
        s->fold_stop = true;
        return;
    }
    if (!em::fold(s->sums, r->off, r->len, r->P, r->crcs.data(), r->crcs.size(), x8().v)) {
        // a continuation with no start: never expected in submission order
        s->fold_broken = true;
        s->fold_stop = true;
    }
}

int stream_drain(krk_piece_stream* s, size_t keep) {
    s->o.drain(keep);
    if (!s->o.err && s->fold_broken) {
        set_error(KRK_EHIP, "engine: piece stream portions out of order");
        s->o.fail(KRK_EHIP);
    }
    return s->o.status();
}

int stream_submit(krk_piece_stream* s, const uint8_t* src, uint64_t len) {
    if (!len) return KRK_OK;
    int rc = stream_drain(s, kOwnerInflight - 1);
    if (rc) return rc;
    Req* r = nullptr;
    rc = make_req(s->o.E, Kind::kCrc, nullptr, src, len, &r);
    if (rc) return rc;
    r->owner = s;
    r->off = s->submitted;
    r->P = s->P;
    r->on_done = stream_fold;
    r->ctx = s;
    s->o.push(Kind::kCrc, r);
    s->submitted += len;
    return KRK_OK;
}

// Host placement: calcPieceSums' loop (core/metainfo.go:157-179) on the caller's thread --
// each piece's crc32.Update value carried across calls, a sum appended when a piece fills.
// A large write is cut into spans (at piece ends, then at most `span` bytes) that idle
// host-pool threads hash beside the caller; the spans' CRCs are combined in order.
void stream_host_update(krk_piece_stream* s, const uint8_t* buf, uint64_t n) {
    const int idle = n >= (2u << 20) && s->P >= (64u << 10) ? host_pool_idle() : 0;
    if (idle <= 0) {  // (small pieces: a span a piece would cost more than it spreads)
        HostCpuToken tok;
        while (n) {
            const uint64_t take = std::min<uint64_t>(n, s->P - s->in_piece);
            s->crc = host_crc32_update(s->crc, buf, take);
            s->in_piece += take;
            s->submitted += take;
            buf += take;
            n -= take;
            if (s->in_piece == s->P) {
                s->sums.push_back(s->crc);
                s->crc = 0;
                s->in_piece = 0;
            }
        }
        return;
    }
    struct Span {
        const uint8_t* p;
        uint64_t n;
        bool ends_piece;
        uint32_t c;
    };
    // A span should outlast a pool thread's wake-up: at least ~40 us of one thread's CRC
    // (256 KiB on the 128-bit PCLMUL loop, ~1.7 MiB on AVX-512 VPCLMULQDQ, where 256 KiB spans
    // took ~6 us each and the caller finished its own before the helpers woke).
    static const uint64_t min_span = [] {
        const uint64_t b = (uint64_t)(host_crc_rate() * 40e-6);
        return std::max<uint64_t>(256u << 10, (b + 65535) & ~uint64_t(65535));
    }();
    const uint64_t span = std::max<uint64_t>(min_span, ((n / (uint64_t)(idle + 1)) + 63) & ~uint64_t(63));
    std::vector<Span> sp;
    for (uint64_t in = s->in_piece, o = 0; o < n;) {
        const uint64_t take = std::min<uint64_t>(n - o, s->P - in);
        for (uint64_t q = 0; q < take; q += span) {
            const uint64_t m = std::min(span, take - q);
            sp.push_back({buf + o + q, m, q + m == take && in + take == s->P, 0});
        }
        in = (in + take) % s->P;
        o += take;
    }
    host_parallel_for(sp.size(), idle, [&](size_t i) { sp[i].c = host_crc32_update(0, sp[i].p, sp[i].n); });
    for (const Span& x : sp) {
        s->crc = crc32_combine(s->crc, x.c, x.n);
        s->in_piece += x.n;
        s->submitted += x.n;
        if (x.ends_piece) {
            s->sums.push_back(s->crc);
            s->crc = 0;
            s->in_piece = 0;
        }
    }
}

}  // namespace
}  // namespace krk

extern "C" {

int krk_piece_stream_begin_on(int placement, int64_t piece_length, krk_piece_stream** out) {
    KRK_CHECK(out, KRK_EINVAL, "out is NULL");
    KRK_CHECK(placement >= KRK_PLACE_AUTO && placement <= KRK_PLACE_GPU, KRK_EINVAL, "unknown placement %d",
              placement);
    KRK_CHECK(piece_length > 0, KRK_EINVAL, "piece length must be positive");
    *out = nullptr;
    int rc = KRK_OK;
    const int where = resolve_crc_placement(placement, &rc);
    if (rc) return rc;
    Engine* E = nullptr;
    if (where == KRK_PLACE_GPU) {
        E = engine_of(place_device(), &rc);
        if (!E) return rc;
    }
    auto* s = new krk_piece_stream();
    s->o.E = E;
    s->P = (uint64_t)piece_length;
    *out = s;
    return KRK_OK;
}

int krk_piece_stream_begin(int64_t piece_length, krk_piece_stream** out) {
    return krk_piece_stream_begin_on(KRK_PLACE_AUTO, piece_length, out);
}

int krk_piece_stream_placement(const krk_piece_stream* s, int* placement) {
    KRK_CHECK(s && placement, KRK_EINVAL, "piece_stream_placement: null argument");
    *placement = s->o.E ? KRK_PLACE_GPU : KRK_PLACE_HOST;
    return KRK_OK;
}

int krk_piece_stream_update(krk_piece_stream* s, const uint8_t* buf, uint64_t n) {
    KRK_CHECK(s, KRK_EINVAL, "stream is NULL");
    KRK_CHECK(n == 0 || buf, KRK_EINVAL, "buffer is NULL");
    if (!s->o.E) {
        stream_host_update(s, buf, n);
        return KRK_OK;
    }
    if (s->o.status()) return s->o.err;
    const size_t S = engine_pool(s->o.E).S;
    while (n) {
        if (s->fill == 0 && n >= S) {  // a whole slot straight from the caller's buffer
            const int rc = stream_submit(s, buf, S);
            if (rc) return rc;
            buf += S;
            n -= S;
            continue;
        }
        if (!s->pend) s->pend = pend_acquire(s->o.E);
        const size_t take = std::min<uint64_t>(n, S - s->fill);
        memcpy(s->pend.get() + s->fill, buf, take);
        s->fill += take;
        buf += take;
        n -= take;
        if (s->fill == S) {
            const int rc = stream_submit(s, s->pend.get(), S);
            if (rc) return rc;
            s->fill = 0;
        }
    }
    return KRK_OK;
}

int krk_piece_stream_end(krk_piece_stream* s, uint32_t* sums_out, uint64_t cap, uint64_t* n_sums,
                         uint64_t* length) {
    KRK_CHECK(s, KRK_EINVAL, "stream is NULL");
    if (s->o.E) {
        if (s->o.status()) return s->o.err;
        int rc = stream_submit(s, s->pend.get(), s->fill);
        if (!rc) s->fill = 0;
        if (!rc) rc = stream_drain(s, 0);
        if (rc) return rc;
    }
    const uint64_t np = krk_num_pieces(s->submitted, (int64_t)s->P);
    if (n_sums) *n_sums = np;
    if (length) *length = s->submitted;
    KRK_CHECK(np <= cap || !sums_out, KRK_ERANGE, "sums capacity %llu < %llu pieces", (unsigned long long)cap,
              (unsigned long long)np);
    const uint64_t have = s->sums.size() + (!s->o.E && s->in_piece ? 1 : 0);
    KRK_CHECK(have >= np, KRK_EHIP, "engine: %llu of %llu piece sums folded", (unsigned long long)have,
              (unsigned long long)np);
    if (sums_out && np) {
        const uint64_t full = std::min<uint64_t>(np, s->sums.size());
        memcpy(sums_out, s->sums.data(), full * 4);
        if (full < np) sums_out[full] = s->crc;  // host: the partial last piece (io.CopyN n > 0)
    }
    return KRK_OK;
}

void krk_piece_stream_free(krk_piece_stream* s) {
    if (!s) return;
    if (s->o.E) {
        stream_drain(s, 0);
        pend_release(s->o.E, std::move(s->pend));
    }
    delete s;
}

// crc32.Update(crc, IEEETable, p): on the caller's thread (HOST, and AUTO below the
// crossover or for writes of at most KRK_CRC_HOST_MAX bytes), else through the device's
// CRC queue (slot-sized portions combined in order on this thread).
int krk_crc32_update_on(int placement, uint32_t crc, const uint8_t* data, uint64_t n, uint32_t* out) {
    KRK_CHECK(out, KRK_EINVAL, "out is NULL");
    KRK_CHECK(n == 0 || data, KRK_EINVAL, "data is NULL");
    KRK_CHECK(placement >= KRK_PLACE_AUTO && placement <= KRK_PLACE_GPU, KRK_EINVAL, "unknown placement %d",
              placement);
    static const size_t host_max = env_size(KRK_OP_ENV("KRK_CRC_HOST_MAX"), 64 << 10);
    int rc = KRK_OK;
    const int where = (placement == KRK_PLACE_AUTO && n <= host_max) ? KRK_PLACE_HOST
                                                                      : resolve_crc_placement(placement, &rc);
    if (rc) return rc;
    if (where == KRK_PLACE_HOST) {
        *out = host_crc32_update_par(crc, data, n);
        return KRK_OK;
    }
    Owner o;
    o.E = engine_of(place_device(), &rc);
    if (!o.E) return rc;
    const size_t S = engine_pool(o.E).S;
    uint32_t c = crc;
    auto combine = [&](Req* r, int e) {  // up to the first failed portion
        if (!e && !o.err) c = gf2_mulmod(c, x8n(r->len, x8().v)) ^ r->crcs[0];
    };
    for (uint64_t off = 0; off < n; off += S) {
        if (o.drain(kOwnerInflight - 1, combine)) break;  // bounded: the slots recycle
        Req* r = nullptr;
        o.fail(make_req(o.E, Kind::kCrc, nullptr, data + off, std::min<uint64_t>(S, n - off), &r));
        if (!r) break;
        r->owner = &o;
        r->off = off;
        r->P = 0;
        o.push(Kind::kCrc, r);
    }
    rc = o.drain(0, combine);
    if (!rc) *out = c;
    return rc;
}

int krk_crc32_update(uint32_t crc, const uint8_t* data, uint64_t n, uint32_t* out) {
    return krk_crc32_update_on(KRK_PLACE_AUTO, crc, data, n, out);
}

int krk_set_crc_placement(int placement) {
    KRK_CHECK(placement >= KRK_PLACE_AUTO && placement <= KRK_PLACE_GPU, KRK_EINVAL, "unknown placement %d",
              placement);
    crc_placement_setting();  // the environment is read first, so this call wins over it
    g_crc_placement.store(placement);
    return KRK_OK;
}

}  // extern "C"
