// info_hash_dev.cpp -- the C ABI's device InfoHash: krk_info_hash_batch_dev over piece sums in
// device memory (info_hash.hip), the process-wide placement krk_metainfo_batch_dev consults,
// and the host hook that runs the kernel's arithmetic (info_hash_math.hpp) on the CPU.
#include "info_hash_math.hpp"
#include "runtime.hpp"

namespace krk {

int info_hash_dev(Device* D, const int64_t* piece_lengths, const uint32_t* sums_dev, const uint64_t* sums_off,
                  const uint64_t* n_sums, const char* names, const uint64_t* name_off, const int64_t* lengths,
                  uint64_t n, uint8_t* out20, hipStream_t s) {
    if (!n) return KRK_OK;
    KRK_CHECK(piece_lengths && sums_off && n_sums && lengths && out20, KRK_EINVAL, "info_hash_batch_dev: null argument");
    KRK_CHECK(names ? name_off != nullptr : (!name_off || name_off[n] == name_off[0]), KRK_EINVAL,
              "info_hash_batch_dev: names is NULL but a name is not empty");
    KRK_CHECK(n < (1ull << 32), KRK_EINVAL, "more than 2^32 blobs in one call");
    uint64_t lo = UINT64_MAX, hi = 0;  // the sums the launch reads
    for (uint64_t i = 0; i < n; ++i) {
        KRK_CHECK(!names || name_off[i] <= name_off[i + 1], KRK_EINVAL, "info_hash_batch_dev: name offsets decrease");
        if (!n_sums[i]) continue;
        KRK_CHECK(sums_dev, KRK_EINVAL, "info_hash_batch_dev: null sums");
        KRK_CHECK(sums_off[i] < (1ull << 60) && n_sums[i] < (1ull << 60), KRK_EINVAL,  // no overflow below
                  "info_hash_batch_dev: sums range of blob %llu is out of range", (unsigned long long)i);
        lo = std::min(lo, sums_off[i]);
        hi = std::max(hi, sums_off[i] + n_sums[i]);
    }
    KRK_CHECK(hi <= lo || device_writable(sums_dev + lo, (hi - lo) * 4), KRK_EINVAL,
              "info_hash_batch_dev: sums_dev must be device memory");
    KRK_CHECK(device_writable(out20, 20 * n), KRK_EINVAL,
              "info_hash_batch_dev: out20 must be device memory or page-locked host memory");
    // One upload: [jobs][name bytes], copied into the library's pinned staging before this
    // returns (the caller may reuse its arrays at once).  Longest chains first.
    const uint64_t nb = names ? name_off[0] : 0, nbytes = names ? name_off[n] - name_off[0] : 0;
    std::vector<uint8_t> pack(n * sizeof(InfoHashJob) + nbytes);
    InfoHashJob* jobs = reinterpret_cast<InfoHashJob*>(pack.data());
    for (uint64_t i = 0; i < n; ++i) {
        InfoHashJob& j = jobs[i];
        j.piece_length = piece_lengths[i];
        j.length = lengths[i];
        j.first_sum = n_sums[i] ? sums_off[i] : 0;
        j.n_sums = n_sums[i];
        j.name_off = names ? name_off[i] - nb : 0;
        j.name_len = names ? name_off[i + 1] - name_off[i] : 0;
        j.out = i;
        j.pad = 0;
    }
    std::stable_sort(jobs, jobs + n, [](const InfoHashJob& a, const InfoHashJob& b) {
        return 12 * a.n_sums + a.name_len > 12 * b.n_sums + b.name_len;
    });
    if (nbytes) memcpy(pack.data() + n * sizeof(InfoHashJob), names + nb, nbytes);
    void* d_pack = nullptr;
    int r = upload(D, pack.data(), pack.size(), &d_pack, s);
    if (r) return r;
    const uint8_t* dp = static_cast<const uint8_t*>(d_pack);
    hipError_t e = timed(K_INFOHASH, s, [&] {
        return launch_info_hash(reinterpret_cast<const InfoHashJob*>(dp), (uint32_t)n, sums_dev,
                                dp + n * sizeof(InfoHashJob), out20, s);
    });
    scratch_free(D, d_pack, s);
    KRK_CHECK(e == hipSuccess, KRK_EHIP, "info_hash launch: %s", launch_error_text(e));
    return KRK_OK;
}

namespace {

std::atomic<int> g_ih_placement{KRK_PLACE_AUTO};  // krk_set_info_hash_placement / KRK_INFOHASH_PLACEMENT

int ih_placement_setting() {
    static std::once_flag once;
    std::call_once(once, [] {
        if (const char* e = KRK_OP_ENV("KRK_INFOHASH_PLACEMENT")) {
            const int v = atoi(e);
            if (v >= KRK_PLACE_AUTO && v <= KRK_PLACE_GPU) g_ih_placement.store(v);
        }
    });
    return g_ih_placement.load(std::memory_order_relaxed);
}

}  // namespace

// AUTO is HOST: the host InfoHash hides behind later groups' kernels (batch_dev.cpp), and on
// C5 regen the device one measured 1.9 % slower, so it is opt-in.
int info_hash_placement_resolved() { return ih_placement_setting() == KRK_PLACE_GPU ? KRK_PLACE_GPU : KRK_PLACE_HOST; }

}  // namespace krk

using namespace krk;

extern "C" {

int krk_info_hash_batch_dev(const int64_t* piece_lengths, const uint32_t* sums_dev, const uint64_t* sums_off,
                            const uint64_t* n_sums, const char* names, const uint64_t* name_off,
                            const int64_t* lengths, uint64_t n, uint8_t* out20, void* stream) {
    KRK_DEVICE(D);
    return info_hash_dev(D, piece_lengths, sums_dev, sums_off, n_sums, names, name_off, lengths, n, out20,
                         pick(D, stream));
}

int krk_set_info_hash_placement(int placement) {
    KRK_CHECK(placement >= KRK_PLACE_AUTO && placement <= KRK_PLACE_GPU, KRK_EINVAL, "unknown placement %d",
              placement);
    ih_placement_setting();  // the environment is read first, so this call wins over it
    g_ih_placement.store(placement);
    return KRK_OK;
}

int krk_info_hash_placement(int* placement) {
    KRK_CHECK(placement, KRK_EINVAL, "info_hash_placement: null argument");
    *placement = ih_placement_setting();
    return KRK_OK;
}

// One InfoHash on the calling thread through info_hash_math.hpp alone, the kernel's steps run
// one lane after another: the header, 64 name bytes a step, 64 sums a step at the offsets an
// exclusive scan of their byte counts gives, "ee" and the padding, all through the byte ring.
int krk_info_hash_math_host(int64_t piece_length, const uint32_t* sums, uint64_t n_sums, const char* name,
                            uint64_t name_len, int64_t length, uint8_t out20[20]) {
    KRK_CHECK(out20 && (!n_sums || sums) && (!name_len || name), KRK_EINVAL, "info_hash_math_host: null argument");
    uint32_t ring[ih::kRingWords] = {};
    uint8_t* ring8 = reinterpret_cast<uint8_t*>(ring);
    uint32_t h[5];
    ih::sha1_init(h);
    uint64_t pos = 0, done = 0;
    auto put = [&](uint64_t at, uint8_t c) { ring8[ih::ring_byte(at)] = c; };
    auto drain = [&] {
        for (; pos - done >= 64; done += 64) {
            uint32_t w[16];
            memcpy(w, ring + ih::ring_block(done), sizeof w);
            ih::sha1_block(h, w);
        }
    };
    pos += ih::header_before_name(length, name_len, pos, put);
    drain();
    for (uint64_t base = 0; base < name_len; base += 64) {
        const uint64_t m = std::min<uint64_t>(64, name_len - base);
        for (uint64_t l = 0; l < m; ++l) put(pos + l, (uint8_t)name[base + l]);
        pos += m;
        drain();
    }
    pos += ih::header_after_name(piece_length, pos, put);
    drain();
    for (uint64_t base = 0; base < n_sums; base += 64) {
        const uint64_t m = std::min<uint64_t>(64, n_sums - base);
        uint32_t off = 0;  // the exclusive scan
        for (uint64_t l = 0; l < m; ++l) {
            const uint32_t v = sums[base + l], nd = ih::digits(v);
            ih::emit_sum(v, nd, pos + off, put);
            off += nd + 2;
        }
        pos += off;
        drain();
    }
    put(pos, (uint8_t)'e');
    put(pos + 1, (uint8_t)'e');
    pos += 2;
    const uint64_t total = pos;
    const uint32_t n_pad = ih::pad_bytes(total);
    for (uint32_t k = 0; k < n_pad; ++k) put(total + k, ih::pad_byte(k, n_pad, total));
    pos += n_pad;
    drain();
    for (uint32_t k = 0; k < 20; ++k) out20[k] = ih::digest_byte(h, k);
    return KRK_OK;
}

}  // extern "C"
