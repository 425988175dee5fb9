// xeve_amd/csrc/ssim_core.h -- the structural similarity of two planes at the codec's 10 bits: the arithmetic of ssim.hip (xeve_hip_ssim_planes), as what ONE lane runs -- the
// sums of a 4x4 block, and a window's figure from the records of its 2x2 blocks.  __host__ __device__ and plain C++: tests/native/ssim_host.cpp compiles the same source for
// the host and holds it to a numpy restatement without a GPU.  The reference has no counterpart, so the definition is this project's own (include/xeve_hip.h states it):
//   block_sums    of the 16 sample pairs (a, b) of a block: s1 = sum a, s2 = sum b, ss = sum (a^2 + b^2), s12 = sum a b
//   window_q      over the 64 pairs of a window (the four records added): A = 2 s1 s2 + C1, B = 2 (64 s12 - s1 s2) + C2, Cn = s1^2 + s2^2 + C1, D = 64 ss - s1^2 - s2^2 + C2 in
//                 int64 (each below 2^34 in magnitude: exact as a double); x = (A * B) / (Cn * D), two IEEE multiplications and one IEEE division, nothing fused (the library
//                 and the test program are built with -ffp-contract=off and without fast-math); q = floor(x * 2^30), scaling and floor exact
// Cn >= C1 and D >= C2 are positive (64 sum a^2 >= (sum a)^2), |A| <= Cn and |B| <= D, so |q| <= 2^30.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#define XQ __host__ __device__ inline __attribute__((always_inline))
#else
#define XQ inline __attribute__((always_inline))
#endif

namespace xssim {

constexpr int64_t C1 = 428658;  // rnd(0.01^2 * 1023^2 * 64^2)
constexpr int64_t C2 = 3797644; // rnd(0.03^2 * 1023^2 * 64 * 63)

// a block's record, 12 bytes.  With 10-bit samples s1, s2 <= 16 * 1023 (14 bits: the four of a window add up inside their 16), ss <= 2^25, s12 <= 2^24
struct Block {
    uint32_t s; // s1 | s2 << 16
    uint32_t ss, s12;
};

// a[r], b[r]: row r of the block in the two planes, four 16-bit samples as they lie in memory (little-endian: sample k in bits 16 k .. 16 k + 15)
XQ Block block_sums(const uint64_t a[4], const uint64_t b[4])
{
    uint32_t s1 = 0, s2 = 0, ss = 0, s12 = 0;
    for(int r = 0; r < 4; r++)
        for(int k = 0; k < 4; k++) {
            const uint32_t x = (uint32_t)(a[r] >> (16 * k)) & 0xFFFFu, y = (uint32_t)(b[r] >> (16 * k)) & 0xFFFFu;
            s1 += x, s2 += y, ss += x * x + y * y, s12 += x * y;
        }
    Block B;
    B.s = s1 | (s2 << 16), B.ss = ss, B.s12 = s12;
    return B;
}

// the window of the blocks tl tr / bl br
XQ int64_t window_q(const Block &tl, const Block &tr, const Block &bl, const Block &br)
{
    const uint32_t s = tl.s + tr.s + bl.s + br.s; // (no carry between the halves: 4 * 16 * 1023 < 2^16)
    const int64_t  s1 = s & 0xFFFFu, s2 = s >> 16, ss = (int64_t)tl.ss + tr.ss + bl.ss + br.ss, s12 = (int64_t)tl.s12 + tr.s12 + bl.s12 + br.s12;
    const int64_t  A = 2 * s1 * s2 + C1, B = 2 * (64 * s12 - s1 * s2) + C2, Cn = s1 * s1 + s2 * s2 + C1, D = 64 * ss - s1 * s1 - s2 * s2 + C2;
    const double   num = (double)A * (double)B, den = (double)Cn * (double)D;
    const double   x = num / den;
    return (int64_t)floor(x * 1073741824.0);
}

} // namespace xssim
