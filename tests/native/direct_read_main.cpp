// direct_read_main.cpp -- direct_pread of kraken_amd/csrc/direct_read.hpp as a stand-alone CPU
// program: the O_DIRECT read of a block-aligned request into a window, its bounce loop (1 MiB
// reads into a buffer of the reading thread, copied out), the process-wide switch and the diag
// build's simulated refusal (KRK_DIRECT_REFUSE).  Every return value and every destination byte
// is compared with one pread of the same request on a buffered descriptor of the same file,
// and the bytes before the destination and after dst + returned must keep their filler.
//
//   direct_read_main DIR          every case but the seam's (the switch forced on)
//   direct_read_main DIR seam     KRK_DIRECT_REFUSE=N in the environment: the N-th read flips
//
// Exit status 0 and "0 mismatches" on success, 77 when DIR takes no O_DIRECT open.
#define KRK_DIAG 1
#include "../../kraken_amd/csrc/direct_read.hpp"

#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <thread>
#include <vector>

using namespace krk;

namespace {
constexpr size_t KiB4 = 4096, MiB = size_t(1) << 20;
constexpr uint8_t kFill = 0xCD;
constexpr size_t kGuard = 2 * KiB4;
int g_bad = 0;
long g_checks = 0;

#define EXPECT(cond, ...)                      \
    do {                                       \
        ++g_checks;                            \
        if (!(cond)) {                         \
            ++g_bad;                           \
            if (g_bad <= 20) {                 \
                fprintf(stderr, "MISMATCH: "); \
                fprintf(stderr, __VA_ARGS__);  \
                fprintf(stderr, "\n");         \
            }                                  \
        }                                      \
    } while (0)

uint8_t byte_at(unsigned id, uint64_t pos) {
    uint64_t x = (pos + 1) * 0x9E3779B97F4A7C15ull + id * 0xD1B54A32D192ED03ull;
    x ^= x >> 29;
    x *= 0xBF58476D1CE4E5B9ull;
    return (uint8_t)(x >> 56);
}

std::string make_file(const std::string& dir, unsigned id, uint64_t len) {
    const std::string path = dir + "/dr" + std::to_string(id);
    std::vector<uint8_t> data(len);
    for (uint64_t i = 0; i < len; ++i) data[i] = byte_at(id, i);
    const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0600);
    if (fd < 0) {
        perror(path.c_str());
        exit(2);
    }
    for (uint64_t a = 0; a < len;) {
        const ssize_t w = write(fd, data.data() + a, len - a);
        if (w <= 0) {
            perror("write");
            exit(2);
        }
        a += (uint64_t)w;
    }
    fsync(fd);
    close(fd);
    return path;
}

struct Fds {
    int direct = -1, buffered = -1;
    explicit Fds(const std::string& path) {
        direct = open(path.c_str(), O_RDONLY | O_DIRECT | O_CLOEXEC);
        buffered = open(path.c_str(), O_RDONLY | O_CLOEXEC);
        if (direct < 0 || buffered < 0) {
            perror(path.c_str());
            exit(2);
        }
    }
    ~Fds() {
        close(direct);
        close(buffered);
    }
};

// A destination of `want` bytes, 4 KiB-aligned, with a guard before and after.
struct Dest {
    void* raw = nullptr;
    size_t want;
    explicit Dest(size_t want_) : want(want_) {
        if (posix_memalign(&raw, KiB4, kGuard + want + kGuard) != 0) exit(2);
        memset(raw, kFill, kGuard + want + kGuard);
    }
    ~Dest() { free(raw); }
    uint8_t* dst() { return static_cast<uint8_t*>(raw) + kGuard; }
    // bytes outside [dst, dst + got) that lost their filler
    size_t touched(size_t got) {
        const uint8_t* p = static_cast<const uint8_t*>(raw);
        size_t n = 0;
        for (size_t i = 0; i < kGuard; ++i) n += p[i] != kFill;
        for (size_t i = kGuard + got; i < kGuard + want + kGuard; ++i) n += p[i] != kFill;
        return n;
    }
};

// One request through direct_pread against one buffered pread of the same request.
// bounced: the bytes came through the bounce buffer, so nothing past dst + returned is written
// (a read straight into the destination may leave the kernel's block padding inside the request).
ssize_t check_request(const Fds& f, uint64_t off, size_t want, ReadCounts* rc, const char* what, bool bounced = true) {
    Dest d(want);
    std::vector<uint8_t> ref(want);
    const ssize_t expect = pread(f.buffered, ref.data(), want, (off_t)off);
    const ssize_t got = direct_pread(f.direct, d.dst(), want, (off_t)off, rc);
    EXPECT(got == expect, "%s off %llu want %zu: returned %zd, buffered pread %zd", what, (unsigned long long)off, want,
           got, expect);
    if (got > 0 && got == expect) {
        size_t first = 0;
        while (first < (size_t)got && d.dst()[first] == ref[first]) ++first;
        EXPECT(first == (size_t)got, "%s off %llu want %zu: byte %zu differs", what, (unsigned long long)off, want, first);
    }
    const size_t kept = bounced ? (got > 0 ? (size_t)got : 0) : want;
    const size_t t = d.touched(kept);
    EXPECT(t == 0, "%s off %llu want %zu: %zu bytes outside [dst, dst + %zu) written", what, (unsigned long long)off, want,
           t, kept);
    return got;
}

const size_t kSizes[] = {KiB4, MiB - KiB4, MiB, MiB + KiB4, 3 * MiB, 3 * MiB + KiB4};
const uint64_t kOffsets[] = {0, KiB4, MiB - KiB4};

void whole_requests(const std::string& dir) {
    const uint64_t len = (MiB - KiB4) + (3 * MiB + KiB4) + 2 * KiB4;
    Fds f(make_file(dir, 1, len));
    for (uint64_t off : kOffsets)
        for (size_t want : kSizes) {
            ReadCounts rc;
            const ssize_t got = check_request(f, off, want, &rc, "whole");
            EXPECT(got == (ssize_t)want, "whole off %llu want %zu: short read %zd", (unsigned long long)off, want, got);
            EXPECT(rc.bounce_bytes.load() == want && rc.window_bytes.load() == 0, "whole want %zu: counted %llu bounced",
                   want, (unsigned long long)rc.bounce_bytes.load());
            EXPECT(rc.bounce_preads.load() == (want + kBounce - 1) / kBounce, "whole want %zu: %llu bounce preads", want,
                   (unsigned long long)rc.bounce_preads.load());
        }
}

void files_ending_inside(const std::string& dir) {
    unsigned id = 100;
    for (uint64_t off : kOffsets) {
        const uint64_t lens[] = {off + 1,       off + 4095,    off + 4096,          off + MiB - 1,
                                 off + MiB,     off + MiB + 1, off + 2 * MiB + 4097};
        for (uint64_t len : lens) {
            Fds f(make_file(dir, id++, len));
            for (size_t want : kSizes) {
                const ssize_t got = check_request(f, off, want, nullptr, "ending");
                const uint64_t in_file = std::min<uint64_t>(want, len - off);
                EXPECT(got == (ssize_t)in_file, "ending len %llu off %llu want %zu: returned %zd",
                       (unsigned long long)len, (unsigned long long)off, want, got);
                if (got > 0 && (uint64_t)got < want) {  // the file ended inside: the next read sees EOF
                    Dest d(KiB4);
                    const ssize_t next = direct_pread(f.direct, d.dst(), KiB4, (off_t)(off + (uint64_t)got));
                    EXPECT(next == 0, "ending len %llu off %llu want %zu: the read after returned %zd (errno %d)",
                           (unsigned long long)len, (unsigned long long)off, want, next, errno);
                    EXPECT(d.touched(0) == 0, "ending len %llu: the read at EOF wrote", (unsigned long long)len);
                }
            }
        }
    }
}

void at_eof_and_bad_descriptors(const std::string& dir) {
    Fds f(make_file(dir, 2, 2 * KiB4));
    for (size_t want : {KiB4, MiB + KiB4}) {
        Dest d(want);
        const ssize_t got = direct_pread(f.direct, d.dst(), want, (off_t)(2 * KiB4));
        EXPECT(got == 0, "at EOF want %zu: returned %zd", want, got);
        EXPECT(d.touched(0) == 0, "at EOF want %zu: wrote", want);
    }
    int closed = open((dir + "/dr2").c_str(), O_RDONLY | O_DIRECT | O_CLOEXEC);
    close(closed);
    for (int fd : {-1, closed}) {
        Dest d(MiB + KiB4);
        ReadCounts rc;
        errno = 0;
        const ssize_t got = direct_pread(fd, d.dst(), MiB + KiB4, 0, &rc);
        const int e = errno;
        EXPECT(got == -1 && e == EBADF, "descriptor %d: returned %zd, errno %d", fd, got, e);
        EXPECT(d.touched(0) == 0, "descriptor %d: wrote", fd);
        EXPECT(rc.bounce_bytes.load() == 0 && rc.window_bytes.load() == 0, "descriptor %d: bytes counted", fd);
    }
}

// The switch off and an ordinary destination: the bytes go into the destination itself, no bounce
// pread is made and the switch stays off.  (The direct path has no pread counter of its own: that
// it is ONE pread is read off direct_pread, not verified here.)
void switch_off(const std::string& dir) {
    Fds f(make_file(dir, 3, 2 * MiB + 5));
    for (size_t want : {KiB4, MiB + KiB4, 3 * MiB}) {
        ReadCounts rc;
        const ssize_t got = check_request(f, KiB4, want, &rc, "switch off", false);
        EXPECT(rc.bounce_preads.load() == 0 && rc.bounce_bytes.load() == 0, "switch off want %zu: %llu bounce preads", want,
               (unsigned long long)rc.bounce_preads.load());
        EXPECT(got > 0 && rc.window_bytes.load() == (uint64_t)got, "switch off want %zu: %llu window bytes of %zd", want,
               (unsigned long long)rc.window_bytes.load(), got);
        EXPECT(!direct_reads_bounce().load(), "switch off want %zu: the switch went on", want);
    }
}

void four_threads(const std::string& dir) {
    std::vector<std::string> paths;
    for (unsigned t = 0; t < 4; ++t) paths.push_back(make_file(dir, 10 + t, 3 * MiB + 4097 + t * 4099));
    struct Out {
        int bad = 0;
        char text[160] = "";
    } out[4];
    std::vector<std::thread> th;
    for (unsigned t = 0; t < 4; ++t)
        th.emplace_back([&, t] {
            Fds f(paths[t]);
            for (int round = 0; round < 3; ++round)
                for (size_t want : kSizes) {
                    const uint64_t off = (uint64_t)round * KiB4;
                    std::vector<uint8_t> ref(want);
                    Dest d(want);
                    const ssize_t expect = pread(f.buffered, ref.data(), want, (off_t)off);
                    const ssize_t got = direct_pread(f.direct, d.dst(), want, (off_t)off);
                    if (got != expect || (got > 0 && memcmp(d.dst(), ref.data(), (size_t)got) != 0) ||
                        d.touched(got > 0 ? (size_t)got : 0)) {
                        if (!out[t].bad++)
                            snprintf(out[t].text, sizeof out[t].text, "thread %u off %llu want %zu: returned %zd of %zd or wrong bytes",
                                     t, (unsigned long long)off, want, got, expect);
                    }
                }
        });
    for (auto& x : th) x.join();
    for (unsigned t = 0; t < 4; ++t) EXPECT(out[t].bad == 0, "%s (%d in all)", out[t].text, out[t].bad);
}

// KRK_DIRECT_REFUSE=N: reads 1 .. N-1 go into the destination, read N is refused, flips the
// switch and still returns the right bytes, and the switch stays on.
void seam(const std::string& dir) {
    const char* v = getenv("KRK_DIRECT_REFUSE");
    const long N = v ? atol(v) : 0;
    if (N < 1) {
        fprintf(stderr, "seam: KRK_DIRECT_REFUSE is not set\n");
        exit(2);
    }
    Fds f(make_file(dir, 4, 2 * MiB + 4097));
    for (long i = 1; i <= N + 2; ++i) {
        ReadCounts rc;
        const size_t want = i % 2 ? MiB + KiB4 : KiB4;
        const ssize_t got = check_request(f, KiB4, want, &rc, "seam", i >= N);
        EXPECT(got == (ssize_t)want, "seam read %ld: returned %zd", i, got);
        if (i < N) {
            EXPECT(!direct_reads_bounce().load() && rc.bounce_preads.load() == 0 && rc.window_bytes.load() == want,
                   "seam read %ld of N = %ld: bounced early", i, N);
        } else {
            EXPECT(direct_reads_bounce().load() && rc.window_bytes.load() == 0 && rc.bounce_bytes.load() == want,
                   "seam read %ld of N = %ld: switch %d, %llu bounced", i, N, (int)direct_reads_bounce().load(),
                   (unsigned long long)rc.bounce_bytes.load());
        }
    }
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s DIR [seam]\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    {
        const std::string probe = make_file(dir, 0, KiB4);
        const int fd = open(probe.c_str(), O_RDONLY | O_DIRECT | O_CLOEXEC);
        if (fd < 0) {
            printf("no O_DIRECT in %s: %s\n", dir.c_str(), strerror(errno));
            return 77;
        }
        close(fd);
    }
    if (argc > 2 && std::string(argv[2]) == "seam") {
        seam(dir);
    } else {
        switch_off(dir);
        direct_reads_bounce().store(true);
        whole_requests(dir);
        files_ending_inside(dir);
        at_eof_and_bad_descriptors(dir);
        four_threads(dir);
        EXPECT(direct_reads_bounce().load(), "the switch went off");
    }
    printf("direct_read: %ld checks, %d mismatches\n", g_checks, g_bad);
    return g_bad ? 1 : 0;
}
