// xeve_amd/csrc/scale_core.h -- decoder surfaces (planar or semi-planar 4:2:0, pitched, 8 bits or 10 bits low- / msb-aligned in 16) -> the planar frames xeve_hip_enc_push
// takes, at another size: the arithmetic of scale.hip (xeve_hip_surface_to_yuv420), as what ONE lane runs for one sample of each pass, and the host's exact derivation of
// the tables.  __host__ __device__ and plain C++: tests/native/scale_host.cpp compiles the same source for the host and holds it to a numpy / Fraction restatement without a
// GPU.  The reference has no scaler, so the definition is this project's own (include/xeve_hip.h states it):
//   sample_of     a source sample: (container >> shift) & (2^d - 1)
//   filter        (host) one axis' table -- per destination index the first tap and NTAPS coefficients at 14 fractional bits -- from the stretched Catmull-Rom kernel at the
//                 exact rational centres, in __int128: no double anywhere; every row sums to 2^14
//   bounds_ok     (host) what lets the passes run in 32-bit sums with a 16-bit intermediate, proven from the tables' sums of |c|
//   hpass         T = (sum c * s + 2^9) >> 10 of one destination column from one source row (four fractional bits kept)
//   vpass         clamp((sum c * T + 2^17) >> 18, 0, 2^d - 1) of one destination sample from one column of T
// A tap outside the plane reads the clamped index and keeps its coefficient.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define XS __host__ __device__ inline __attribute__((always_inline))
#else
#define XS inline __attribute__((always_inline))
#endif
#include <vector>

namespace xscl {

constexpr int CBITS = 14;    // fractional bits of a coefficient
constexpr int HSHIFT = 10;   // the horizontal pass keeps CBITS - HSHIFT = 4 fractional bits
constexpr int VSHIFT = 18;   // the vertical pass drops them with its own 14
constexpr int MAX_RATIO = 8; // per axis, either way
constexpr int MAX_TAPS = 4 * MAX_RATIO + 1;
enum { KIND_PLAIN = 0, KIND_LEFT = 1 }; // KIND_LEFT: chroma co-sited with the even luma columns; the lengths handed over are the LUMA widths

XS int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
XS int sample_of(unsigned container, int shift, unsigned mask) { return (int)((container >> shift) & mask); }

// row[0] is the sample of source column `base`; coefficient j at c[j * cstride]; sn: the plane's length along the axis
XS int hpass(const uint16_t *row, int base, int sn, const int16_t *c, int cstride, int first, int ntaps)
{
    int acc = 1 << (HSHIFT - 1);
    for(int j = 0; j < ntaps; j++) acc += (int)c[j * cstride] * (int)row[clampi(first + j, 0, sn - 1) - base];
    return acc >> HSHIFT;
}
// col[0] is T of source row `base`, rows rstride apart
XS int vpass(const int16_t *col, int rstride, int base, int sn, const int16_t *c, int cstride, int first, int ntaps, int maxv)
{
    int acc = 1 << (VSHIFT - 1);
    for(int j = 0; j < ntaps; j++) acc += (int)c[j * cstride] * (int)col[(clampi(first + j, 0, sn - 1) - base) * rstride];
    return clampi(acc >> VSHIFT, 0, maxv);
}

// ---- host only: the tables, exact -------------------------------------------------------------
typedef __int128 i128;
inline i128 floor_div(i128 a, i128 b) // b > 0
{
    const i128 q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}
inline i128 rnd_div(i128 num, i128 den) // round half away from zero; den > 0
{
    const bool neg = num < 0;
    const i128 q = ((neg ? -num : num) * 2 + den) / (2 * den);
    return neg ? -q : q;
}
struct Axis {
    int                  sn = 0, dn = 0; // the PLANE's lengths (KIND_LEFT: half the lengths handed over)
    int                  ntaps = 0;      // of every row: the longest row's; shorter rows end in zeros
    int                  sum_abs = 0;    // the largest sum of |c| over a row
    std::vector<int32_t> first;          // [dn] the lowest tap of the row (may lie outside the plane: read clamped)
    std::vector<int16_t> coef;           // [dn][ntaps]
};
// The table of one axis.  kind 0: src_n -> dst_n samples of a plane (1 .. 8192 each); kind 1: the chroma columns of a picture src_n -> dst_n LUMA samples wide (even).
// false: outside the accepted lengths and ratios, or a row that does not fit the table's types
inline bool filter(int src_n, int dst_n, int kind, Axis &A)
{
    if(kind != KIND_PLAIN && kind != KIND_LEFT) return false;
    if(src_n < 1 || dst_n < 1 || src_n > 8192 || dst_n > 8192 || src_n > MAX_RATIO * dst_n || dst_n > MAX_RATIO * src_n) return false;
    if(kind == KIND_LEFT && ((src_n | dst_n) & 1)) return false;
    A.sn = kind == KIND_LEFT ? src_n / 2 : src_n, A.dn = kind == KIND_LEFT ? dst_n / 2 : dst_n;
    const i128 den = kind == KIND_LEFT ? 4 * (i128)dst_n : 2 * (i128)dst_n;
    const i128 a = dst_n < src_n ? dst_n : 1, b = dst_n < src_n ? src_n : 1; // the stretch min(1, dn / sn)
    const i128 D = den * b, D2 = D * D, D3 = D2 * D;                           // t = T / D with T = (k * den - num) * a
    std::vector<int32_t> rows((size_t)A.dn * MAX_TAPS, 0);
    std::vector<int>     count(A.dn, 0);
    A.first.assign(A.dn, 0), A.ntaps = 0, A.sum_abs = 0;
    for(int i = 0; i < A.dn; i++) {
        const i128 num = kind == KIND_LEFT ? (4 * (i128)i + 1) * src_n - dst_n : (2 * (i128)i + 1) * src_n - dst_n;
        const i128 k0 = floor_div(num * a - 2 * D, den * a) + 1, k1 = -floor_div(-(num * a + 2 * D), den * a) - 1; // the integers k with |T| < 2 D
        const int  n = (int)(k1 - k0 + 1);
        if(n < 1 || n > MAX_TAPS) return false;
        i128 W[MAX_TAPS], sum = 0;
        int  best = 0;
        for(int j = 0; j < n; j++) {
            const i128 T = ((k0 + j) * den - num) * a, u = T < 0 ? -T : T;
            W[j] = u <= D ? 3 * u * u * u - 5 * u * u * D + 2 * D3 : -(u * u * u) + 5 * u * u * D - 8 * u * D2 + 4 * D3; // w(t) * 2 D^3
            sum += W[j];
            if(W[j] > W[best]) best = j;
        }
        if(sum <= 0) return false;
        int64_t total = 0;
        int32_t *c = &rows[(size_t)i * MAX_TAPS];
        for(int j = 0; j < n; j++) c[j] = (int32_t)rnd_div(W[j] * ((i128)1 << CBITS), sum), total += c[j];
        c[best] += (int32_t)((1 << CBITS) - total);
        int sa = 0;
        for(int j = 0; j < n; j++) {
            if(c[j] < -32768 || c[j] > 32767) return false;
            sa += c[j] < 0 ? -c[j] : c[j];
        }
        A.first[i] = (int32_t)k0, count[i] = n;
        if(n > A.ntaps) A.ntaps = n;
        if(sa > A.sum_abs) A.sum_abs = sa;
    }
    A.coef.assign((size_t)A.dn * A.ntaps, 0);
    for(int i = 0; i < A.dn; i++)
        for(int j = 0; j < count[i]; j++) A.coef[(size_t)i * A.ntaps + j] = (int16_t)rows[(size_t)i * MAX_TAPS + j];
    return true;
}
// The narrowed types of the two passes for a pair of tables at depth d: the horizontal sum and the vertical sum in int32, T in int16.  |sum c s| <= sum_abs_h * (2^d - 1),
// so |T| <= tmax = ((sum_abs_h * (2^d - 1) + 2^9) >> 10) + 1, and |sum c T| <= sum_abs_v * tmax
inline bool bounds_ok(int sum_abs_h, int sum_abs_v, int depth)
{
    const int64_t maxv = ((int64_t)1 << depth) - 1, hacc = (int64_t)sum_abs_h * maxv + (1 << (HSHIFT - 1));
    if(hacc > INT32_MAX) return false;
    const int64_t tmax = (hacc >> HSHIFT) + 1;
    if(tmax > 32767) return false;
    return (int64_t)sum_abs_v * tmax + (1 << (VSHIFT - 1)) <= INT32_MAX;
}

// ---- host only: one plane through the lane functions (the restatement's counterpart; scale.hip's kernel differs in how it loads, tiles and stores only).  src: the plane's
// first byte; a source element is `estep` containers of `sb` bytes, the sample is container `eoff` of it; rows `pitch` bytes apart.  out: [V.dn][H.dn] ----
inline void scale_plane(const uint8_t *src, int sb, int estep, int eoff, int64_t pitch, int shift, int depth, const Axis &H, const Axis &V, uint16_t *out)
{
    const unsigned        mask = (1u << depth) - 1;
    std::vector<uint16_t> row(H.sn);
    std::vector<int16_t>  T((size_t)V.sn * H.dn);
    for(int r = 0; r < V.sn; r++) {
        const uint8_t *p = src + (int64_t)r * pitch;
        for(int x = 0; x < H.sn; x++) {
            const size_t at = ((size_t)x * estep + eoff) * sb;
            row[x] = (uint16_t)sample_of(sb == 1 ? (unsigned)p[at] : (unsigned)p[at] | ((unsigned)p[at + 1] << 8), shift, mask);
        }
        for(int x = 0; x < H.dn; x++) T[(size_t)r * H.dn + x] = (int16_t)hpass(row.data(), 0, H.sn, &H.coef[(size_t)x * H.ntaps], 1, H.first[x], H.ntaps);
    }
    for(int y = 0; y < V.dn; y++)
        for(int x = 0; x < H.dn; x++) out[(size_t)y * H.dn + x] = (uint16_t)vpass(T.data() + x, H.dn, 0, V.sn, &V.coef[(size_t)y * V.ntaps], 1, V.first[y], V.ntaps, (int)mask);
}

} // namespace xscl
