// hjd_jpeg_orientation robustness harness, built with AddressSanitizer + UBSan
// on the CPU (tests/test_orient_cpu.py builds and runs it): for every JPEG file
// named on the command line, the reader is called on the file, on every
// truncation of it, and on ITERATIONS seeded byte mutations of its APP1
// segment (flips, a rewritten segment length, a cut right after it).  Every
// input is an exact-size heap copy, so a read past its end aborts the run.
// The result must be an orientation in 1..8, and HJD_OK or HJD_E_INVALID.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "hjd_host.h"
#include "hjd_internal.h"

int hjd_internal::set_error(int code, const char*, ...) { return code; }

static long g_calls = 0, g_ok = 0;

static bool run(const std::vector<uint8_t>& d)
{
    uint8_t* buf = static_cast<uint8_t*>(malloc(d.size() ? d.size() : 1));
    std::copy(d.begin(), d.end(), buf);
    int32_t o = -1;
    const int rc = hjd_jpeg_orientation(buf, d.size(), &o);
    free(buf);
    ++g_calls;
    if (rc == HJD_OK) ++g_ok;
    if ((rc != HJD_OK && rc != HJD_E_INVALID) || o < 1 || o > 8) {
        fprintf(stderr, "hjd_jpeg_orientation: rc %d, orientation %d\n", rc, static_cast<int>(o));
        return false;
    }
    return true;
}

int main(int argc, char** argv)
{
    if (argc < 3) {
        fprintf(stderr, "usage: %s ITERATIONS file.jpg...\n", argv[0]);
        return 2;
    }
    const int iters = atoi(argv[1]);
    std::mt19937 rng(20112);
    for (int a = 2; a < argc; ++a) {
        FILE* fp = fopen(argv[a], "rb");
        if (!fp) return 2;
        std::vector<uint8_t> src;
        for (int c; (c = fgetc(fp)) != EOF;) src.push_back(static_cast<uint8_t>(c));
        fclose(fp);
        if (!run(src)) return 3;
        for (size_t n = 0; n < src.size(); ++n)   // every truncation
            if (!run(std::vector<uint8_t>(src.begin(), src.begin() + static_cast<long>(n)))) return 3;
        // the first APP1 segment (marker at `at`), or the file's first 256 bytes
        size_t at = 2, len = std::min<size_t>(src.size(), 256);
        for (size_t p = 2; p + 4 <= src.size() && src[p] == 0xFF;) {
            const size_t l = static_cast<size_t>(src[p + 2]) << 8 | src[p + 3];
            if (src[p + 1] == 0xE1) {
                at = p;
                len = std::min(l + 2, src.size() - p);
                break;
            }
            if (src[p + 1] == 0xDA) break;
            p += 2 + l;
        }
        for (int i = 0; i < iters; ++i) {
            std::vector<uint8_t> d = src;
            const int nflip = 1 + static_cast<int>(rng() % 6);
            for (int k = 0; k < nflip; ++k) {
                const size_t off = at + rng() % len;
                d[off] = (rng() % 4 == 0) ? 0xFF : (rng() % 4 == 0) ? 0 : static_cast<uint8_t>(rng());
            }
            if (rng() % 8 == 0 && at + 4 <= d.size()) {   // a segment length of its own
                d[at + 2] = static_cast<uint8_t>(rng() % 3 == 0 ? rng() : 0);
                d[at + 3] = static_cast<uint8_t>(rng());
            }
            if (rng() % 8 == 0) d.resize(at + rng() % (len + 8 < d.size() - at ? len + 8 : d.size() - at) + 1);
            if (!run(d)) return 3;
        }
    }
    printf("hjd_jpeg_orientation: %ld calls, %ld HJD_OK\n", g_calls, g_ok);
    return 0;
}
