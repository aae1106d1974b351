// placement.cpp -- the C ABI's HRW ordering and ring.Locations placement, with the per-device
// cache of shard owner tables.
#include <numeric>

#include "runtime.hpp"
#include "staging.hpp"

using namespace krk;

extern "C" {

// ---------------------------------------------------------------- HRW
static int hexv(char c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}

// A ring's node table (label bytes, label offsets, weights) and, for the Locations
// table, the healthy flags: ONE upload (one copy on the stream instead of four).
struct DevNodes {
    void* pack = nullptr;
    const uint8_t* labels = nullptr;
    const uint64_t* off = nullptr;
    const int64_t* w = nullptr;
    const uint8_t* healthy = nullptr;
};

static int upload_nodes(Device* D, const krk_nodes* nodes, DevNodes& dn, hipStream_t s,
                        const uint8_t* healthy = nullptr) {
    KRK_CHECK(nodes && nodes->n_nodes > 0 && nodes->label_off && nodes->weights, KRK_EINVAL,
              "nodes: empty or null");
    KRK_CHECK(nodes->n_nodes <= 4096, KRK_EINVAL, "more than 4096 nodes");
    const uint64_t N = nodes->n_nodes, lb = nodes->label_off[N];
    KRK_CHECK(lb == 0 || nodes->labels, KRK_EINVAL, "nodes: labels are null");
    const size_t o_w = (N + 1) * 8, o_lab = o_w + N * 8, o_h = o_lab + lb;  // 8-byte parts first
    std::vector<uint8_t> pk(o_h + (healthy ? N : 0) + 1, 0);
    memcpy(pk.data(), nodes->label_off, (N + 1) * 8);
    memcpy(pk.data() + o_w, nodes->weights, N * 8);
    if (lb) memcpy(pk.data() + o_lab, nodes->labels, lb);
    if (healthy) memcpy(pk.data() + o_h, healthy, N);
    int r = upload(D, pk.data(), pk.size(), &dn.pack, s);
    if (r) return r;
    const uint8_t* b = static_cast<const uint8_t*>(dn.pack);
    dn.off = reinterpret_cast<const uint64_t*>(b);
    dn.w = reinterpret_cast<const int64_t*>(b + o_w);
    dn.labels = b + o_lab;
    dn.healthy = healthy ? b + o_h : nullptr;
    return KRK_OK;
}

static void free_nodes(Device* D, DevNodes& dn, hipStream_t s) {
    if (dn.pack) scratch_free(D, dn.pack, s);
    dn = DevNodes();
}

// Order + Locations table for nk decoded keys already on the device; result rows
// on the device.
static int hrw_table_dev(Device* D, const void* d_kb, const void* d_koff, const void* d_bad, uint64_t nk,
                         const krk_nodes* nodes, const uint8_t* healthy, int32_t max_replica, uint32_t row_out,
                         int32_t** d_locs, uint8_t** d_counts, hipStream_t s) {
    const uint32_t N = nodes->n_nodes;
    DevNodes dn;
    int r = upload_nodes(D, nodes, dn, s, healthy);
    int32_t* d_order = nullptr;
    if (!r && scratch_alloc(D, reinterpret_cast<void**>(&d_order), nk * N * 4, s) != hipSuccess) r = KRK_ENOMEM;
    if (!r && scratch_alloc(D, reinterpret_cast<void**>(d_locs), nk * row_out * 4, s) != hipSuccess) r = KRK_ENOMEM;
    if (!r && scratch_alloc(D, reinterpret_cast<void**>(d_counts), nk, s) != hipSuccess) r = KRK_ENOMEM;
    if (!r) {
        HrwArgs a{static_cast<const uint8_t*>(d_kb), static_cast<const uint64_t*>(d_koff), nk, dn.labels, dn.off,
                  dn.w, N, N, static_cast<const uint8_t*>(d_bad), d_order, nullptr};
        hipError_t e = timed(K_HRW, s, [&] { return launch_hrw_order(a, s); });
        if (e == hipSuccess)
            e = timed(K_FILTER, s, [&] {
                return launch_ring_filter(d_order, nk, N, dn.healthy, max_replica, row_out, *d_locs, *d_counts, s);
            });
        if (e != hipSuccess) { set_error(KRK_EHIP, "hrw launch: %s", launch_error_text(e)); r = KRK_EHIP; }
    }
    free_nodes(D, dn, s);
    if (d_order) scratch_free(D, d_order, s);
    return r;
}

// The same for keys given on the host.
static int hrw_table(Device* D, const std::vector<uint8_t>& kb, const std::vector<uint64_t>& koff,
                     const std::vector<uint8_t>& bad, const krk_nodes* nodes, const uint8_t* healthy,
                     int32_t max_replica, uint32_t row_out, int32_t** d_locs, uint8_t** d_counts,
                     hipStream_t s) {
    void *d_kb = nullptr, *d_koff = nullptr, *d_bad = nullptr;
    int r = upload(D, kb.data(), kb.size(), &d_kb, s);
    if (!r) r = upload(D, koff.data(), koff.size() * 8, &d_koff, s);
    if (!r) r = upload(D, bad.data(), bad.size(), &d_bad, s);
    if (!r) r = hrw_table_dev(D, d_kb, d_koff, d_bad, koff.size() - 1, nodes, healthy, max_replica, row_out,
                              d_locs, d_counts, s);
    for (void* p : {d_kb, d_koff, d_bad})
        if (p) scratch_free(D, p, s);
    return r;
}

int krk_hrw_ordered(const char* keys, const uint64_t* key_off, uint64_t n_keys, const krk_nodes* nodes,
                    uint32_t n_out, int32_t* order_out, double* scores_out) {
    if (!n_keys) return KRK_OK;
    KRK_CHECK(keys && key_off && order_out, KRK_EINVAL, "hrw_ordered: null argument");
    // rows are n_out wide (-1 padded past the node count); bounded like the node count
    KRK_CHECK(n_out <= 4096, KRK_EINVAL, "n_out %u exceeds 4096", n_out);
    KRK_DEVICE(D);
    hipStream_t s = D->s_main;
    // hex.DecodeString per key (rendezvous.go:154-157).
    std::vector<uint8_t> kb;
    std::vector<uint64_t> koff(n_keys + 1, 0);
    std::vector<uint8_t> bad(n_keys, 0);
    bool any_bad = false;
    for (uint64_t i = 0; i < n_keys; ++i) {
        const char* k = keys + key_off[i];
        const uint64_t len = key_off[i + 1] - key_off[i];
        koff[i] = kb.size();
        bool ok = (len % 2) == 0;
        for (uint64_t q = 0; ok && q + 1 < len; q += 2) {
            const int a = hexv(k[q]), b = hexv(k[q + 1]);
            if (a < 0 || b < 0) { ok = false; break; }
            kb.push_back((uint8_t)(a << 4 | b));
        }
        if (!ok) { kb.resize(koff[i]); bad[i] = 1; any_bad = true; }
    }
    koff[n_keys] = kb.size();
    if (kb.empty()) kb.push_back(0);
    DevNodes dn;
    int r = upload_nodes(D, nodes, dn, s);
    const uint32_t N = nodes ? nodes->n_nodes : 0;
    void *d_kb = nullptr, *d_koff = nullptr, *d_bad = nullptr;
    int32_t* d_order = nullptr;
    double* d_sc = nullptr;
    if (!r) r = upload(D, kb.data(), kb.size(), &d_kb, s);
    if (!r) r = upload(D, koff.data(), koff.size() * 8, &d_koff, s);
    if (!r) r = upload(D, bad.data(), bad.size(), &d_bad, s);
    if (!r && scratch_alloc(D, reinterpret_cast<void**>(&d_order), n_keys * n_out * 4 + 4, s) != hipSuccess) r = KRK_ENOMEM;
    if (!r && scores_out && scratch_alloc(D, reinterpret_cast<void**>(&d_sc), n_keys * N * 8, s) != hipSuccess)
        r = KRK_ENOMEM;
    if (!r) {
        HrwArgs a{static_cast<const uint8_t*>(d_kb), static_cast<const uint64_t*>(d_koff), n_keys, dn.labels, dn.off,
                  dn.w, N, n_out, static_cast<const uint8_t*>(d_bad), d_order, d_sc};
        // n_out == 0 with scores wanted still scores (the kernel then writes no order entry)
        hipError_t e = n_out || d_sc ? timed(K_HRW, s, [&] { return launch_hrw_order(a, s); }) : hipSuccess;
        if (e != hipSuccess) { set_error(KRK_EHIP, "hrw launch: %s", launch_error_text(e)); r = KRK_EHIP; }
    }
    // Copy-out: drain the stream, then blocking copies into the caller's (pageable) memory.
    if (hipStreamSynchronize(s) != hipSuccess && !r) { set_error(KRK_EHIP, "hrw sync"); r = KRK_EHIP; }
    if (!r && n_out && hipMemcpy(order_out, d_order, n_keys * n_out * 4, hipMemcpyDeviceToHost) != hipSuccess)
        r = KRK_EHIP;
    if (!r && scores_out && hipMemcpy(scores_out, d_sc, n_keys * N * 8, hipMemcpyDeviceToHost) != hipSuccess)
        r = KRK_EHIP;
    free_nodes(D, dn, s);
    for (void* p : {d_kb, d_koff, d_bad, static_cast<void*>(d_order), static_cast<void*>(d_sc)})
        if (p) scratch_free(D, p, s);
    if (hipStreamSynchronize(s) != hipSuccess && !r) { set_error(KRK_EHIP, "hrw sync"); r = KRK_EHIP; }
    if (!r && any_bad) {
        set_error(KRK_EHEX, "invalid hex key: Score is NaN");
        return KRK_EHEX;
    }
    return r;
}

int krk_hrw_uint64_to_float64(const uint8_t* sums8, uint64_t n, int rehash, double* out) {
    if (!n) return KRK_OK;
    KRK_CHECK(sums8 && out, KRK_EINVAL, "hrw_uint64_to_float64: null argument");
    KRK_DEVICE(D);
    hipStream_t s = D->s_main;
    std::vector<uint64_t> v(n);
    for (uint64_t i = 0; i < n; ++i) {  // binary.BigEndian.Uint64
        uint64_t x = 0;
        for (int k = 0; k < 8; ++k) x = x << 8 | sums8[8 * i + k];
        v[i] = x;
    }
    void* d_v = nullptr;
    double* d_o = nullptr;
    int r = upload(D, v.data(), n * 8, &d_v, s);
    if (!r && scratch_alloc(D, &d_o, n * 8, s) != hipSuccess) r = KRK_ENOMEM;
    if (!r) {
        hipError_t e = launch_u64_to_f64(static_cast<const uint64_t*>(d_v), n, rehash, d_o, s);
        if (e != hipSuccess) { set_error(KRK_EHIP, "u64_to_f64 launch: %s", launch_error_text(e)); r = KRK_EHIP; }
    }
    if (hipStreamSynchronize(s) != hipSuccess && !r) { set_error(KRK_EHIP, "u64_to_f64 sync"); r = KRK_EHIP; }
    if (!r && hipMemcpy(out, d_o, n * 8, hipMemcpyDeviceToHost) != hipSuccess) r = KRK_EHIP;
    if (d_v) scratch_free(D, d_v, s);
    if (d_o) scratch_free(D, d_o, s);
    return r;
}

static void shard_keys(std::vector<uint8_t>& kb, std::vector<uint64_t>& koff, const std::vector<uint32_t>& shards) {
    kb.resize(shards.size() * 2);
    koff.resize(shards.size() + 1);
    for (size_t i = 0; i < shards.size(); ++i) {
        kb[2 * i] = (uint8_t)(shards[i] >> 8);
        kb[2 * i + 1] = (uint8_t)shards[i];
        koff[i] = 2 * i;
    }
    koff[shards.size()] = kb.size();
}

// Owner counts are one byte each (counts_out, the table's d_tc, the packed rows): a shard of
// a ring of more than 255 nodes with MaxReplica past 255 would have more owners than a count
// can say.  Refused before anything is launched or written.
static int check_owner_count(const krk_nodes* nodes, int32_t max_replica) {
    const int64_t most = std::min<int64_t>(max_replica, nodes->n_nodes);
    KRK_CHECK(most <= 255, KRK_ERANGE, "ring: up to %lld owners a shard do not fit the 8-bit owner counts (<= 255)",
              (long long)most);
    return KRK_OK;
}

int krk_ring_locations(const uint8_t* digests32, uint64_t n, const krk_nodes* nodes, const uint8_t* healthy,
                       int32_t max_replica, int32_t* locs_out, uint8_t* counts_out) {
    if (!n) return KRK_OK;
    KRK_CHECK(digests32 && nodes && healthy && locs_out && counts_out, KRK_EINVAL, "ring_locations: null argument");
    if (const int rc = check_owner_count(nodes, max_replica)) return rc;
    KRK_DEVICE(D);
    hipStream_t s = D->s_main;
    const uint32_t row_out = (uint32_t)std::max<int32_t>(1, max_replica);
    // Only the shards present: Locations depends on d only through ShardID.
    std::vector<int32_t> row_of(65536, -1);
    std::vector<uint32_t> shards;
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t sh = (uint32_t)digests32[32 * i] << 8 | digests32[32 * i + 1];
        if (row_of[sh] < 0) { row_of[sh] = (int32_t)shards.size(); shards.push_back(sh); }
    }
    std::vector<uint8_t> kb, bad(shards.size(), 0);
    std::vector<uint64_t> koff;
    shard_keys(kb, koff, shards);
    int32_t* d_locs = nullptr;
    uint8_t* d_counts = nullptr;
    int r = hrw_table(D, kb, koff, bad, nodes, healthy, max_replica, row_out, &d_locs, &d_counts, s);
    std::vector<int32_t> tl(shards.size() * row_out);
    std::vector<uint8_t> tc(shards.size());
    if (hipStreamSynchronize(s) != hipSuccess && !r) { set_error(KRK_EHIP, "ring sync"); r = KRK_EHIP; }
    if (!r && hipMemcpy(tl.data(), d_locs, tl.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) r = KRK_EHIP;
    if (!r && hipMemcpy(tc.data(), d_counts, tc.size(), hipMemcpyDeviceToHost) != hipSuccess) r = KRK_EHIP;
    if (d_locs) scratch_free(D, d_locs, s);
    if (d_counts) scratch_free(D, d_counts, s);
    if (hipStreamSynchronize(s) != hipSuccess && !r) { set_error(KRK_EHIP, "ring sync"); r = KRK_EHIP; }
    if (r) return r;
    for (uint64_t i = 0; i < n; ++i) {
        const int32_t row = row_of[(uint32_t)digests32[32 * i] << 8 | digests32[32 * i + 1]];
        memcpy(locs_out + i * row_out, tl.data() + (uint64_t)row * row_out, row_out * 4);
        counts_out[i] = tc[row];
    }
    return KRK_OK;
}

}  // extern "C"

// The 65,536-row owner table (one row per ShardID) on the device: d_tl rows of row_out
// node indices (-1 padded), d_tc counts.  Released by the caller with scratch_free.
static int shard_owner_table(Device* D, const krk_nodes* nodes, const uint8_t* healthy, int32_t max_replica,
                             uint32_t row_out, int32_t** d_tl, uint8_t** d_tc, hipStream_t s) {
    std::call_once(D->shard_once, [D] {
        std::vector<uint32_t> shards(65536);
        std::iota(shards.begin(), shards.end(), 0u);
        std::vector<uint8_t> kb, bad(65536, 0);
        std::vector<uint64_t> koff;
        shard_keys(kb, koff, shards);
        if (hipMalloc(&D->shard_kb, kb.size()) != hipSuccess || hipMalloc(&D->shard_koff, koff.size() * 8) != hipSuccess ||
            hipMalloc(&D->shard_bad, bad.size()) != hipSuccess ||
            hipMemcpy(D->shard_kb, kb.data(), kb.size(), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(D->shard_koff, koff.data(), koff.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(D->shard_bad, bad.data(), bad.size(), hipMemcpyHostToDevice) != hipSuccess)
            D->shard_rc = KRK_ENOMEM;
    });
    KRK_CHECK(D->shard_rc == KRK_OK, D->shard_rc, "shard key table allocation failed");
    return hrw_table_dev(D, D->shard_kb, D->shard_koff, D->shard_bad, 65536, nodes, healthy, max_replica, row_out,
                         d_tl, d_tc, s);
}

// The shard owner tables of the last few memberships a device served (ring.Refresh caches
// its hrw in the reference, lib/hashring/ring.go:141-165; Locations never recomputes it):
// keyed by the exact membership bytes (labels, weights, health, MaxReplica).  A table is
// built once on the caller's stream (ready event); later callers wait for that event and
// record a per-stream "used" event, and an evicted table's blocks go back to the scratch
// cache stream-ordered behind every stream that used it.
namespace krk {
struct OwnerTable {
    std::vector<uint8_t> key;
    int32_t* tl = nullptr;
    uint8_t* tc = nullptr;
    uint32_t* tp = nullptr;  // packed rows (launch_pack_owner_rows) when N <= 255 and row <= 3
    hipEvent_t ready = nullptr;
    std::vector<std::pair<hipStream_t, hipEvent_t>> used;
    uint64_t stamp = 0;
    int inflight = 0;  // callers between owner_table() and owner_used(): not evictable
};
struct OwnerTables {
    std::vector<OwnerTable> e;
    uint64_t clock = 0;
};
}  // namespace krk
static constexpr size_t kOwnerTables = 8;

static std::vector<uint8_t> owner_key(const krk_nodes* nodes, const uint8_t* healthy, int32_t max_replica) {
    const uint32_t N = nodes->n_nodes;
    std::vector<uint8_t> k;
    auto put = [&k](const void* p, size_t n) {
        const uint8_t* b = static_cast<const uint8_t*>(p);
        k.insert(k.end(), b, b + n);
    };
    put(&N, 4);
    put(&max_replica, 4);
    put(nodes->label_off, (N + 1) * 8);
    put(nodes->labels + nodes->label_off[0], nodes->label_off[N] - nodes->label_off[0]);
    put(nodes->weights, N * 8);
    put(healthy, N);
    return k;
}

static void owner_release(Device* D, OwnerTable& t, hipStream_t s) {
    for (auto& u : t.used) {
        hipStreamWaitEvent(s, u.second, 0);
        hipEventDestroy(u.second);
    }
    if (t.ready) hipEventDestroy(t.ready);
    if (t.tl) scratch_free(D, t.tl, s);
    if (t.tc) scratch_free(D, t.tc, s);
    if (t.tp) scratch_free(D, t.tp, s);
    const int inflight = t.inflight;
    t = OwnerTable{};
    t.inflight = inflight;
}

// Device pointers of the owner table of (nodes, healthy, max_replica), usable on stream s
// once the call returns (s waits for its build); the caller's use is recorded after its
// launch with owner_used(), which every successful call must be followed by.  Slots are
// stable: a failed build leaves its slot empty instead of erasing it, and a slot
// with a caller between the two calls is never evicted (the cache grows past kOwnerTables
// rather than release a table a launch is about to read).
static int owner_table(Device* D, const krk_nodes* nodes, const uint8_t* healthy, int32_t max_replica,
                       uint32_t row_out, int32_t** d_tl, uint8_t** d_tc, uint32_t** d_tp, size_t* slot,
                       hipStream_t s) {
    std::vector<uint8_t> key = owner_key(nodes, healthy, max_replica);
    std::lock_guard<std::mutex> g(D->owners_mu);
    if (!D->owners) D->owners = new OwnerTables();
    OwnerTables& C = *D->owners;
    for (size_t i = 0; i < C.e.size(); ++i)
        if (C.e[i].key == key) {
            KRK_HIP(hipStreamWaitEvent(s, C.e[i].ready, 0));
            C.e[i].stamp = ++C.clock;
            C.e[i].inflight++;
            *d_tl = C.e[i].tl;
            *d_tc = C.e[i].tc;
            *d_tp = C.e[i].tp;
            *slot = i;
            return KRK_OK;
        }
    size_t i = C.e.size();
    for (size_t j = 0; j < C.e.size(); ++j)  // an empty slot (a failed build) first
        if (C.e[j].key.empty() && !C.e[j].inflight) {
            i = j;
            break;
        }
    if (i == C.e.size() && C.e.size() >= kOwnerTables) {  // else the least recently used idle one goes
        for (size_t j = 0; j < C.e.size(); ++j)
            if (!C.e[j].inflight && (i == C.e.size() || C.e[j].stamp < C.e[i].stamp)) i = j;
        if (i < C.e.size()) owner_release(D, C.e[i], s);
    }
    if (i == C.e.size()) C.e.emplace_back();
    OwnerTable& t = C.e[i];
    int r = shard_owner_table(D, nodes, healthy, max_replica, row_out, &t.tl, &t.tc, s);
    if (!r && nodes->n_nodes <= 255 && row_out <= 3 &&
        (scratch_alloc(D, &t.tp, 65536 * sizeof(uint32_t), s) != hipSuccess ||
         launch_pack_owner_rows(t.tl, t.tc, row_out, t.tp, s) != hipSuccess)) {
        set_error(KRK_EHIP, "ring owner table: packed rows");
        r = KRK_EHIP;
    }
    if (!r && (hipEventCreateWithFlags(&t.ready, hipEventDisableTiming) != hipSuccess ||
               hipEventRecord(t.ready, s) != hipSuccess)) {
        set_error(KRK_EHIP, "ring owner table: event");
        r = KRK_EHIP;
    }
    if (r) {
        owner_release(D, t, s);  // the slot stays, empty (key cleared), for the next build
        return r;
    }
    t.key = std::move(key);
    t.stamp = ++C.clock;
    t.inflight++;
    *d_tl = t.tl;
    *d_tc = t.tc;
    *d_tp = t.tp;
    *slot = i;
    return KRK_OK;
}

void krk::owner_tables_teardown(Device& D) {
    if (!D.owners) return;
    for (OwnerTable& t : D.owners->e) owner_release(&D, t, D.s_main);
    hipStreamSynchronize(D.s_main);
    delete D.owners;
    D.owners = nullptr;
}

static void owner_used(Device* D, size_t slot, hipStream_t s) {
    std::lock_guard<std::mutex> g(D->owners_mu);
    OwnerTable& t = D->owners->e[slot];
    t.inflight--;
    for (auto& u : t.used)
        if (u.first == s) {
            hipEventRecord(u.second, s);
            return;
        }
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess && hipEventRecord(ev, s) == hipSuccess)
        t.used.push_back({s, ev});
    else if (ev) {
        hipEventDestroy(ev);
        hipStreamSynchronize(s);  // no event to order the release behind: the use is done now
    }
}

// Where the placement kernels may write [p, p + n): device memory, or page-locked host
// memory the GPU maps at its host address (krk_host_alloc / hipHostMalloc / registered:
// the gather then writes the owner lists over PCIe and the caller needs no copy-back).
// Pageable memory, or a mapping at another address, is refused -- the kernel would fault.
bool krk::device_writable(const void* p, uint64_t n) {
    auto ok_at = [](const void* q) {
        hipPointerAttribute_t a{};
        if (hipPointerGetAttributes(&a, q) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        // device memory, managed / unified memory, or page-locked host memory
        // the GPU maps at its host address
        if (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged || a.type == hipMemoryTypeUnified)
            return true;
        return a.type == hipMemoryTypeHost && a.devicePointer == q;
    };
    return ok_at(p) && (n <= 1 || ok_at(static_cast<const uint8_t*>(p) + n - 1));
}

template <typename T>
static int ring_locations_dev(const uint8_t* digests32_dev, uint64_t n, const krk_nodes* nodes,
                              const uint8_t* healthy, int32_t max_replica, T* locs_dev, uint8_t* counts_dev,
                              void* stream) {
    if (!n) return KRK_OK;
    KRK_CHECK(digests32_dev && healthy && locs_dev && counts_dev && nodes, KRK_EINVAL,
              "ring_locations_dev: null argument");
    KRK_CHECK(sizeof(T) != 1 || nodes->n_nodes <= 255, KRK_ERANGE,
              "ring_locations_u8_dev: %u nodes do not fit 8-bit owner indices (<= 255)", nodes->n_nodes);
    if (const int rc = check_owner_count(nodes, max_replica)) return rc;
    KRK_DEVICE(D);
    hipStream_t s = pick(D, stream);
    const uint32_t row_out = (uint32_t)std::max<int32_t>(1, max_replica);
    KRK_CHECK(device_writable(locs_dev, n * row_out * sizeof(T)) && device_writable(counts_dev, n), KRK_EINVAL,
              "ring_locations_dev: locs and counts must be device memory or page-locked host memory");
    int32_t* d_tl = nullptr;
    uint8_t* d_tc = nullptr;
    uint32_t* d_tp = nullptr;
    size_t slot = 0;
    int r = owner_table(D, nodes, healthy, max_replica, row_out, &d_tl, &d_tc, &d_tp, &slot, s);
    if (!r) {
        hipError_t e = timed(K_GATHER, s, [&] {
            if constexpr (sizeof(T) == 1) {
                // word stores need word-aligned outputs and a 2-byte aligned digest array
                const bool words = d_tp && !((uintptr_t)digests32_dev & 1) && !((uintptr_t)locs_dev & 3) &&
                                   !((uintptr_t)counts_dev & 3);
                if (words) return launch_shard_gather_packed(digests32_dev, n, d_tp, row_out, locs_dev, counts_dev, s);
                return launch_shard_gather_u8(digests32_dev, n, d_tl, d_tc, row_out, locs_dev, counts_dev, s);
            } else
                return launch_shard_gather(digests32_dev, n, d_tl, d_tc, row_out, locs_dev, counts_dev, s);
        });
        owner_used(D, slot, s);
        if (e != hipSuccess) { set_error(KRK_EHIP, "gather launch: %s", launch_error_text(e)); r = KRK_EHIP; }
    }
    return r;
}

extern "C" {

int krk_ring_owner_table(const krk_nodes* nodes, const uint8_t* healthy, int32_t max_replica, int32_t* locs_out,
                         uint8_t* counts_out) {
    KRK_CHECK(nodes && healthy && locs_out && counts_out, KRK_EINVAL, "ring_owner_table: null argument");
    if (const int rc = check_owner_count(nodes, max_replica)) return rc;
    KRK_DEVICE(D);
    hipStream_t s = D->s_main;
    const uint32_t row_out = (uint32_t)std::max<int32_t>(1, max_replica);
    int32_t* d_tl = nullptr;
    uint8_t* d_tc = nullptr;
    int r = shard_owner_table(D, nodes, healthy, max_replica, row_out, &d_tl, &d_tc, s);
    if (hipStreamSynchronize(s) != hipSuccess && !r) { set_error(KRK_EHIP, "owner table sync"); r = KRK_EHIP; }
    if (!r && (hipMemcpy(locs_out, d_tl, size_t(65536) * row_out * 4, hipMemcpyDeviceToHost) != hipSuccess ||
               hipMemcpy(counts_out, d_tc, 65536, hipMemcpyDeviceToHost) != hipSuccess)) {
        set_error(KRK_EHIP, "owner table copy");
        r = KRK_EHIP;
    }
    if (d_tl) scratch_free(D, d_tl, s);
    if (d_tc) scratch_free(D, d_tc, s);
    return r;
}

int krk_ring_locations_dev(const uint8_t* digests32_dev, uint64_t n, const krk_nodes* nodes,
                           const uint8_t* healthy, int32_t max_replica, int32_t* locs_dev, uint8_t* counts_dev,
                           void* stream) {
    return ring_locations_dev(digests32_dev, n, nodes, healthy, max_replica, locs_dev, counts_dev, stream);
}

int krk_ring_locations_u8_dev(const uint8_t* digests32_dev, uint64_t n, const krk_nodes* nodes,
                              const uint8_t* healthy, int32_t max_replica, uint8_t* locs_dev, uint8_t* counts_dev,
                              void* stream) {
    return ring_locations_dev(digests32_dev, n, nodes, healthy, max_replica, locs_dev, counts_dev, stream);
}

}  // extern "C"
