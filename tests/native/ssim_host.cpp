// tests/native/ssim_host.cpp -- xeve_amd/csrc/ssim_core.h (the per-lane code of ssim.hip: a 4x4 block's sums, a window's q from four records) compiled for the HOST and run
// over whole planes.  tests/test_ssim_host.py builds this with the address and undefined-behaviour sanitizers and -ffp-contract=off and compares its output with the numpy
// restatement (tests/_ssim.py).  Every plane is a heap block of exactly pw * ph samples, so a block read past the last whole one is a report.
//   ssim_host <jobs file> <output file>
// jobs file: int64 count, then per job 2 x int64 { pw, ph } followed by the two planes (pw * ph 16-bit samples each, rows of pw).  Output per job: int64 Q, int64 n, then the
// n windows' q in raster order.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../xeve_amd/csrc/ssim_core.h"

using namespace xssim;

int main(int argc, char **argv)
{
    if(argc != 3) return 2;
    FILE   *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    int64_t n = 0;
    if(!f || !o || fread(&n, 8, 1, f) != 1) return 2;
    for(int64_t k = 0; k < n; k++) {
        int64_t j[2];
        if(fread(j, 8, 2, f) != 2) return 3;
        const int    pw = (int)j[0], ph = (int)j[1], bx = pw >> 2, by = ph >> 2;
        const size_t ns = (size_t)pw * ph;
        if(pw < 8 || ph < 8) return 4;
        uint16_t *a = static_cast<uint16_t *>(malloc(ns * 2)), *b = static_cast<uint16_t *>(malloc(ns * 2)); // (exactly the described samples)
        if(!a || !b || fread(a, 2, ns, f) != ns || fread(b, 2, ns, f) != ns) return 3;
        std::vector<Block> rec((size_t)bx * by);
        for(int y = 0; y < by; y++)
            for(int x = 0; x < bx; x++) {
                uint64_t ra[4], rb[4];
                for(int r = 0; r < 4; r++) memcpy(&ra[r], a + (size_t)(4 * y + r) * pw + 4 * x, 8), memcpy(&rb[r], b + (size_t)(4 * y + r) * pw + 4 * x, 8);
                rec[(size_t)y * bx + x] = block_sums(ra, rb);
            }
        std::vector<int64_t> out(2);
        for(int y = 0; y + 1 < by; y++)
            for(int x = 0; x + 1 < bx; x++) {
                const Block *p = &rec[(size_t)y * bx + x];
                out.push_back(window_q(p[0], p[1], p[bx], p[bx + 1]));
                out[0] += out.back();
            }
        out[1] = (int64_t)out.size() - 2;
        if(fwrite(out.data(), 8, out.size(), o) != out.size()) return 7;
        free(a), free(b);
    }
    fclose(f);
    return fclose(o) == 0 ? 0 : 7;
}
