// digester.cpp -- krk_digester_*: the streaming SHA-256 Digester on its two placements.
//
// Host crossover: a digester created while few digesters are live runs
// SHA-NI on its caller's thread (one core ~2 GB/s vs one GPU stream ~59 MB/s); product code
// (host_meta.cpp).  Beyond it a digester owns a state row of its device's submission engine
// (engine.cpp) and hands it its bytes a slot at a time.
#include "engine.hpp"
#include "offload.hpp"

namespace krk {
namespace {

std::atomic<int64_t> g_live_digesters{0};
std::atomic<int64_t> g_host_streams{-1};  // -1: default (host threads x per-stream rate ratio)

// Live digesters up to which new ones run on their caller's thread: below the crossover
// where the GPU engine's aggregate (live streams x the planner's per-stream rate, capped by
// the host link) overtakes the host's (the CPU budget x one thread's SHA-NI rate), both
// from the calling thread's device's planner rates (planner_math.hpp digester_crossover; the
// nominal ones without a device).  KRK_DIGESTER_HOST_STREAMS / krk_set_digester_host_streams
// pin it.
int64_t host_stream_limit() {
    const int64_t v = g_host_streams.load(std::memory_order_relaxed);
    if (v >= 0) return v;
    static const int64_t env = [] {
        const char* e = KRK_OP_ENV("KRK_DIGESTER_HOST_STREAMS");
        return e && *e ? std::max<int64_t>(0, strtoll(e, nullptr, 10)) : int64_t(-1);
    }();
    if (env >= 0) return env;
    int drc = KRK_OK;
    const int64_t x = digester_crossover(planner_rates(device(&drc)), (int)host_threads());
    return x == INT64_MAX ? x : x - 1;
}

}  // namespace
}  // namespace krk

using namespace krk;

struct krk_digester {
    Owner o;  // o.E null: host placement
    // host placement: midstate after every block and the partial block
    uint32_t h[8];
    uint64_t absorbed = 0;
    uint8_t tail[64];
    size_t ntail = 0;
    // GPU placement: the engine state row, bytes not yet submitted (pend[0, fill)),
    // bytes handed to the engine
    uint32_t row = 0;
    Slot* cur = nullptr;               // pending bytes filled in place in a staging slot, or
    std::unique_ptr<uint8_t[]> pend;   // in a host buffer when the pool is near its cap
    size_t fill = 0;
    uint64_t submitted = 0;
    uint8_t last_digest[32] = {};
};

namespace {

// Wait until at most `keep` of d's requests are in flight; a failed one poisons d.
int digester_drain(krk_digester* d, size_t keep) {
    return d->o.drain(keep, [d](Req* r, int rc) {
        if (rc == KRK_OK && r->final) memcpy(d->last_digest, r->digest, 32);
    });
}

// Submit `len` bytes: from the slot `sl` the digester filled in place (handed over to the
// request), else copied from `src` into a fresh slot.
int digester_submit(krk_digester* d, const uint8_t* src, uint64_t len, bool final, Slot* sl = nullptr) {
    Engine* E = d->o.E;
    auto t0 = Clock::now();
    int rc = digester_drain(d, owner_inflight(E) - 1);
    trace_slow(E, "drain", t0);
    t0 = Clock::now();
    if (rc) {
        engine_pool(E).release(sl);
        return rc;
    }
    Req* r = nullptr;
    rc = make_req(E, Kind::kSha, sl, src, len, &r);
    if (rc) return rc;
    trace_slow(E, sl ? "stage" : "make_req", t0);
    r->owner = d;
    r->row = d->row;
    r->prefix = d->submitted;
    r->final = final;
    d->o.push(Kind::kSha, r);
    if (!final) d->submitted += len;
    return KRK_OK;
}

}  // namespace

extern "C" {

int krk_digester_new_on(int placement, krk_digester** out) {
    KRK_CHECK(out, KRK_EINVAL, "out is NULL");
    KRK_CHECK(placement >= KRK_PLACE_AUTO && placement <= KRK_PLACE_GPU, KRK_EINVAL, "unknown placement %d",
              placement);
    *out = nullptr;
    const int64_t live = g_live_digesters.fetch_add(1) + 1;
    bool host = placement == KRK_PLACE_HOST || (placement == KRK_PLACE_AUTO && live <= host_stream_limit());
    if (!host) {
        // GPU placement needs a gfx950 device (KRK_ENODEV without one); AUTO on a host with
        // none is the host placement: the product's own SHA-NI path (host_meta.cpp).
        int drc = KRK_OK;
        if (!device(&drc)) {
            if (placement == KRK_PLACE_GPU) {
                g_live_digesters.fetch_sub(1);
                return drc;
            }
            host = true;
        }
    }
    auto* d = new krk_digester();
    memcpy(d->h, kIV, sizeof d->h);
    if (!host) {
        int rc = KRK_OK;
        d->o.E = engine_of(place_device(), &rc);
        if (d->o.E) d->row = row_acquire(d->o.E, &rc);
        if (d->o.E && !rc) engine_live_digesters(d->o.E).fetch_add(1);
        if (rc) {
            delete d;
            g_live_digesters.fetch_sub(1);
            return rc;
        }
    }
    *out = d;
    return KRK_OK;
}

int krk_digester_new(krk_digester** out) { return krk_digester_new_on(KRK_PLACE_AUTO, out); }

int krk_digester_placement(const krk_digester* d, int* placement) {
    KRK_CHECK(d && placement, KRK_EINVAL, "digester_placement: null argument");
    *placement = d->o.E ? KRK_PLACE_GPU : KRK_PLACE_HOST;
    return KRK_OK;
}

int krk_digester_write(krk_digester* d, const uint8_t* buf, uint64_t n) {
    KRK_CHECK(d, KRK_EINVAL, "digester is NULL");
    KRK_CHECK(n == 0 || buf, KRK_EINVAL, "buffer is NULL");
    Engine* E = d->o.E;
    if (!E) {  // host: whole blocks straight from the caller's buffer
        if (d->ntail) {
            const size_t take = std::min<uint64_t>(n, 64 - d->ntail);
            memcpy(d->tail + d->ntail, buf, take);
            d->ntail += take;
            buf += take;
            n -= take;
            if (d->ntail < 64) return KRK_OK;
            host_sha256_blocks(d->h, d->tail, 1);
            d->absorbed += 64;
            d->ntail = 0;
        }
        const uint64_t nb = n / 64;
        if (nb) host_sha256_blocks(d->h, buf, nb);
        d->absorbed += nb * 64;
        memcpy(d->tail, buf + nb * 64, n - nb * 64);
        d->ntail = n - nb * 64;
        return KRK_OK;
    }
    if (d->o.status()) return d->o.err;
    SlotPool& pool = engine_pool(E);
    const size_t S = pool.S;
    while (n) {
        if (d->fill == 0 && n >= S) {  // a whole slot straight from the caller's buffer
            const int rc = digester_submit(d, buf, S, false);
            if (rc) return rc;
            buf += S;
            n -= S;
            continue;
        }
        if (d->fill == 0 && !d->cur) {
            const auto t0 = Clock::now();
            d->cur = pool.try_acquire(pool.reserve());
            trace_slow(E, "try_acquire", t0);
        }
        uint8_t* dst;
        if (d->cur) {
            dst = d->cur->host;
        } else {
            if (!d->pend) d->pend = pend_acquire(E);
            dst = d->pend.get();
        }
        const size_t take = std::min<uint64_t>(n, S - d->fill);
        const auto tc = Clock::now();
        memcpy(dst + d->fill, buf, take);
        trace_slow(E, d->cur ? "memcpy_slot" : "memcpy_pend", tc);
        d->fill += take;
        buf += take;
        n -= take;
        if (d->fill == S) {
            Slot* sl = d->cur;
            d->cur = nullptr;
            const int rc = digester_submit(d, dst, S, false, sl);
            if (rc) return rc;
            d->fill = 0;
        }
    }
    return KRK_OK;
}

int krk_digester_sum(krk_digester* d, uint8_t out32[32]) {
    KRK_CHECK(d && out32, KRK_EINVAL, "digester_sum: null argument");
    Engine* E = d->o.E;
    if (!E) {
        host_sha256_final(d->h, d->absorbed, d->tail, d->ntail, out32);
        return KRK_OK;
    }
    if (d->o.status()) return d->o.err;
    // the pending bytes stay pending (Digest() does not reset: writing may continue): a
    // slot filled in place goes with the final request and its bytes move to the host
    // buffer
    Slot* sl = d->cur;
    if (sl) {
        if (!d->pend) d->pend = pend_acquire(E);
        memcpy(d->pend.get(), sl->host, d->fill);
        d->cur = nullptr;
    }
    int rc = digester_submit(d, d->pend.get(), d->fill, true, sl);
    if (!rc) rc = digester_drain(d, 0);
    if (!rc) memcpy(out32, d->last_digest, 32);
    return rc;
}

void krk_digester_free(krk_digester* d) {
    if (!d) return;
    if (Engine* E = d->o.E) {
        digester_drain(d, 0);
        engine_pool(E).release(d->cur);
        row_release(E, d->row);
        pend_release(E, std::move(d->pend));
        engine_live_digesters(E).fetch_sub(1);
    }
    g_live_digesters.fetch_sub(1);
    delete d;
}

int krk_set_digester_host_streams(int64_t n) {
    g_host_streams.store(n < 0 ? -1 : n);
    return KRK_OK;
}

int krk_digester_host_streams(int64_t* n) {
    KRK_CHECK(n, KRK_EINVAL, "n is NULL");
    *n = host_stream_limit();
    return KRK_OK;
}

}  // extern "C"
