// verify.cpp -- blobs against the MetaInfo already stored for them, answered as piece
// bitfields (Torrent.Bitfield(), lib/torrent/storage/agentstorage/torrent.go:130-140): the host
// packer (krk_piece_bitfield, bit-identical to piece_bitfield.hip), the device-resident batch
// (krk_verify_batch_dev) and the cache-file batch (krk_verify_files).
#include "bitfield_math.hpp"
#include "runtime.hpp"

using namespace krk;

extern "C" {

uint64_t krk_bitfield_words(uint64_t n_pieces) { return bf::words(n_pieces); }

int krk_piece_bitfield(const uint32_t* sums, const uint32_t* expected, uint64_t n_pieces, uint64_t* bits_out,
                       uint32_t* n_bad_out) {
    KRK_CHECK(n_pieces <= 0xFFFFFFFFull, KRK_EINVAL, "piece_bitfield: more than 2^32 pieces in one blob");
    KRK_CHECK(!n_pieces || (sums && expected && bits_out), KRK_EINVAL, "piece_bitfield: null argument");
    const uint64_t good = bf::pack(sums, expected, n_pieces, bits_out);
    if (n_bad_out) *n_bad_out = (uint32_t)(n_pieces - good);
    return KRK_OK;
}

int krk_verify_batch_dev(const krk_blob* blobs, uint64_t n_blobs, const uint32_t* expected_host,
                         const uint8_t* expected_digests_host, uint64_t* bits_out, uint32_t* n_bad_out,
                         uint8_t* digest_ok_out, void* stream) {
    if (!n_blobs) return KRK_OK;
    KRK_DEVICE(D);
    int r = validate_blobs(blobs, n_blobs);
    if (r) return r;
    KRK_CHECK(n_blobs < (1ull << 32), KRK_EINVAL, "more than 2^32 blobs in one call");
    KRK_CHECK(n_bad_out, KRK_EINVAL, "verify_batch_dev: n_bad_out is NULL");
    KRK_CHECK((expected_digests_host != nullptr) == (digest_ok_out != nullptr), KRK_EINVAL,
              "verify_batch_dev: digest_ok_out must be given exactly when expected digests are");
    uint64_t lo, hi;
    sums_span(blobs, n_blobs, &lo, &hi);
    // One upload: [descriptors][expected sums of the span][expected digests], each 16-byte aligned.
    const uint64_t n_exp = hi - lo, exp_at = n_blobs * sizeof(BitfieldBlob);
    const uint64_t dig_at = (exp_at + n_exp * 4 + 15) & ~15ull;
    std::vector<uint8_t> pack(dig_at + (expected_digests_host ? 32 * n_blobs : 0));
    BitfieldBlob* desc = reinterpret_cast<BitfieldBlob*>(pack.data());
    std::vector<krk_blob> local(blobs, blobs + n_blobs);  // sums indexed from the span's start
    uint64_t words = 0;
    for (uint64_t i = 0; i < n_blobs; ++i) {
        const uint64_t np = krk_num_pieces(blobs[i].length, blobs[i].piece_length);
        local[i].sums_offset = np ? blobs[i].sums_offset - lo : 0;
        desc[i] = BitfieldBlob{local[i].sums_offset, np, words, 0};
        words += krk_bitfield_words(np);
    }
    KRK_CHECK(!n_exp || (expected_host && bits_out), KRK_EINVAL, "verify_batch_dev: null argument");
    KRK_CHECK(!((uintptr_t)bits_out & 7) && !((uintptr_t)n_bad_out & 3), KRK_EINVAL,
              "verify_batch_dev: bits_out must be 8-byte and n_bad_out 4-byte aligned");
    KRK_CHECK((!words || device_writable(bits_out, 8 * words)) && device_writable(n_bad_out, 4 * n_blobs) &&
                  (!digest_ok_out || device_writable(digest_ok_out, n_blobs)),
              KRK_EINVAL, "verify_batch_dev: outputs must be device memory or page-locked host memory");
    if (n_exp) memcpy(pack.data() + exp_at, expected_host + lo, n_exp * 4);
    if (expected_digests_host) memcpy(pack.data() + dig_at, expected_digests_host, 32 * n_blobs);

    hipStream_t s = pick(D, stream);
    uint32_t* d_sums = nullptr;  // the sums and the digests live in scratch and never reach the host
    uint8_t* d_dig = nullptr;
    void* d_pack = nullptr;
    KRK_HIP(scratch_alloc(D, &d_sums, std::max<uint64_t>(n_exp, 1) * 4, s));
    if (expected_digests_host && scratch_alloc(D, &d_dig, 32 * n_blobs, s) != hipSuccess) {
        scratch_free(D, d_sums, s);
        set_error(KRK_EHIP, "verify_batch_dev: digest scratch");
        return KRK_EHIP;
    }
    // With digests: SHA-256 and CRC on two streams joined back into s, the host offload as set
    // (krk_metainfo_digest_dev); without: the piece-sum launch alone.
    r = d_dig ? krk_metainfo_digest_dev(local.data(), n_blobs, d_sums, d_dig, s)
              : piece_sums_dev(D, local.data(), n_blobs, d_sums, s);
    if (!r) r = upload(D, pack.data(), pack.size(), &d_pack, s);
    if (!r) {
        const uint8_t* dp = static_cast<const uint8_t*>(d_pack);
        const hipError_t e = timed(K_BITFIELD, s, [&] {
            const hipError_t eb =
                launch_piece_bitfield(reinterpret_cast<const BitfieldBlob*>(dp), n_blobs, words, d_sums,
                                      reinterpret_cast<const uint32_t*>(dp + exp_at), bits_out, n_bad_out, s);
            return eb != hipSuccess || !d_dig ? eb : launch_digest_equal(d_dig, dp + dig_at, n_blobs, digest_ok_out, s);
        });
        if (e != hipSuccess) {
            set_error(KRK_EHIP, "piece_bitfield launch: %s", launch_error_text(e));
            r = KRK_EHIP;
        }
    }
    scratch_free(D, d_pack, s);
    scratch_free(D, d_dig, s);
    scratch_free(D, d_sums, s);
    return r;
}

int krk_verify_files(const krk_file_blob* files, uint64_t n_files, const uint32_t* expected,
                     const uint8_t* expected_digests, uint64_t* bits_host, uint32_t* n_bad_host,
                     uint8_t* digest_ok_host) {
    if (!n_files) return KRK_OK;
    KRK_CHECK(files && n_bad_host, KRK_EINVAL, "verify_files: null argument");
    KRK_CHECK((expected_digests != nullptr) == (digest_ok_host != nullptr), KRK_EINVAL,
              "verify_files: digest_ok_host must be given exactly when expected digests are");
    uint64_t hi = 0;
    for (uint64_t i = 0; i < n_files; ++i) {
        KRK_CHECK(files[i].path, KRK_EINVAL, "file %llu: path is NULL", (unsigned long long)i);
        const int r = validate_pieces(files[i]);
        if (r) return r;
        const uint64_t np = krk_num_pieces(files[i].length, files[i].piece_length);
        if (np) hi = std::max(hi, files[i].sums_offset + np);
    }
    KRK_CHECK(!hi || (expected && bits_host), KRK_EINVAL, "verify_files: null argument");
    // The underlying calls leave the sums on the host (the CRC placement rule of
    // krk_piece_sums_files; with digests the one read a byte of krk_metainfo_digest_files), so
    // the host packer answers.
    std::vector<uint32_t> sums(std::max<uint64_t>(hi, 1));
    std::vector<uint8_t> dig(expected_digests ? 32 * n_files : 0);
    const int r = expected_digests ? krk_metainfo_digest_files(files, n_files, sums.data(), dig.data())
                                   : krk_piece_sums_files(files, n_files, sums.data());
    if (r) return r;
    uint64_t word = 0;
    for (uint64_t i = 0; i < n_files; ++i) {
        const uint64_t np = krk_num_pieces(files[i].length, files[i].piece_length);
        const uint64_t so = np ? files[i].sums_offset : 0;
        krk_piece_bitfield(sums.data() + so, expected ? expected + so : nullptr, np, bits_host ? bits_host + word : nullptr,
                           n_bad_host + i);
        word += krk_bitfield_words(np);
        if (expected_digests) digest_ok_host[i] = memcmp(dig.data() + 32 * i, expected_digests + 32 * i, 32) == 0;
    }
    return KRK_OK;
}

}  // extern "C"
