// xeve_amd/csrc/color_core.h -- RGB <-> planar 4:2:0 Y'CbCr in integers: the arithmetic of color.hip (xeve_hip_rgb_to_yuv420 / xeve_hip_yuv420_to_rgb), as what ONE lane
// runs for one 2x2 block.  __host__ __device__ and plain C++: tests/native/color_host.cpp compiles the same source for the host and holds it to a numpy / Fraction
// restatement without a GPU.  Nothing here is a codec tool -- the reference takes Y'CbCr only -- so the definition is this project's own (include/xeve_hip.h states it):
//   c16           a component as 16 bits: uint8 * 257; floats widened to float32, NaN -> 0, clamped to [0, 1], floor(x * 65535 + 0.5) with product and sum each rounded
//                 to float32 (never fused)
//   matrix        (host) the coefficients at S = 24 fractional bits from Kr, Kb as exact decimals, rounded half away from zero in __int128 -- no double anywhere;
//                 the chroma rows sum to 0 (greys give exactly oC), the luma row to rnd(a)
//   fwd_block     4 luma samples and one Cb, Cr pair from the block's taps: chroma from the SUM of the c16 triples (siting centre: the 2x2 block; left: columns
//                 2i - 1, 2i, 2i + 1 with weights 1 2 1, two rows), one rounding, clamped (full-range chroma reaches 2^d)
//   inv_block     4 RGB triples as 16 bits from 4 luma samples and the 3x3 chroma neighbourhood: chroma bilinear as a sum of weight 16, one rounding, clamped
//   out_*         16 bits to uint8 ((v + 128) / 257), float32 (v / 65535), float16 / bfloat16 (that float32 rounded to nearest-even)
// The half and bfloat16 conversions are done on the bits, so host and device run the same code.
#pragma once
#include <stdint.h>
#include <string.h>
#if defined(__HIPCC__)
#define XC __host__ __device__ inline __attribute__((always_inline))
#define XC_UNROLL _Pragma("unroll")
#else
#define XC inline __attribute__((always_inline))
#define XC_UNROLL
#endif

namespace xcol {

constexpr int S = 24; // fractional bits of every coefficient
enum { DT_U8 = 0, DT_F16 = 1, DT_BF16 = 2, DT_F32 = 3 };
enum { SIT_LEFT = 0, SIT_CENTRE = 1 };
template <int DT> struct Elem { typedef uint16_t type; };
template <> struct Elem<DT_U8> { typedef uint8_t type; };
template <> struct Elem<DT_F32> { typedef float type; };

struct Fwd {
    int64_t m[9];   // rows Y, Cb, Cr; columns R, G, B
    int64_t oY, oC; // at the output depth
    int32_t maxv, reserved;
};
struct Inv {
    int64_t iY, rCr, gCb, gCr, bCb;
    int64_t oY, oC; // at the codec's 10 bits
};

XC float bits_f32(uint32_t u)
{
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
XC uint32_t f32_bits(float f)
{
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}
XC float f16_to_f32(uint16_t h)
{
    const uint32_t s = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
    if(e == 0) { // zero and subnormals: m * 2^-24, exact
        const float v = (float)m * bits_f32(0x33800000u);
        return s ? -v : v;
    }
    if(e == 31) return bits_f32(s | 0x7F800000u | (m << 13));
    return bits_f32(s | ((e + 112u) << 23) | (m << 13));
}
XC float bf16_to_f32(uint16_t h) { return bits_f32((uint32_t)h << 16); }
// a float32 of [0, 1] to the nearest half, ties to even (subnormal halves included: 1 / 65535 is one)
XC uint16_t f32_to_f16(float f)
{
    const uint32_t u = f32_bits(f), m = u & 0x7FFFFFu;
    const int      e = (int)(u >> 23) - 127;
    if((u << 1) == 0) return 0;
    uint32_t v, shift;
    if(e >= -14) v = ((uint32_t)(e + 15) << 23) | m, shift = 13; // (a carry out of the mantissa raises the exponent)
    else v = m | 0x800000u, shift = (uint32_t)(13 + (-14 - e));
    if(shift > 25) return 0;
    const uint32_t h = v >> shift, rem = v & ((1u << shift) - 1u), half = 1u << (shift - 1);
    return (uint16_t)(h + ((rem > half || (rem == half && (h & 1u))) ? 1u : 0u));
}
XC uint16_t f32_to_bf16(float f) // (finite input)
{
    const uint32_t u = f32_bits(f);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

XC int c16_of(float x)
{
    if(!(x == x)) x = 0.0f;
    x = x < 0.0f ? 0.0f : x > 1.0f ? 1.0f : x;
#if defined(__HIP_DEVICE_COMPILE__)
    const float t = __fadd_rn(__fmul_rn(x, 65535.0f), 0.5f);
#else
    volatile float p = x * 65535.0f; // (the host builds with -ffp-contract=off as well; the product is rounded to float32 either way)
    const float    t = p + 0.5f;
#endif
    return (int)t; // t >= 0.5: truncation is floorf
}
template <int DT> XC int c16_load(const void *base, int64_t idx)
{
    if constexpr(DT == DT_U8) return (int)static_cast<const uint8_t *>(base)[idx] * 257;
    else if constexpr(DT == DT_F16) return c16_of(f16_to_f32(static_cast<const uint16_t *>(base)[idx]));
    else if constexpr(DT == DT_BF16) return c16_of(bf16_to_f32(static_cast<const uint16_t *>(base)[idx]));
    else return c16_of(static_cast<const float *>(base)[idx]);
}
template <int DT> XC int c16_elem(typename Elem<DT>::type v) { return c16_load<DT>(&v, 0); }
template <int DT> XC typename Elem<DT>::type out_elem(int v16)
{
    if constexpr(DT == DT_U8) return (uint8_t)((v16 + 128) / 257);
    else {
#if defined(__HIP_DEVICE_COMPILE__)
        const float f = __fdiv_rn((float)v16, 65535.0f);
#else
        const float f = (float)v16 / 65535.0f;
#endif
        if constexpr(DT == DT_F16) return f32_to_f16(f);
        else if constexpr(DT == DT_BF16) return f32_to_bf16(f);
        else return f;
    }
}

XC int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

// p[row][k][component]: rows 2j, 2j + 1 of the block; k = 0: column 2i - 1 clamped (siting left only, otherwise unused), k = 1, 2: columns 2i, 2i + 1.
// y[row][column], u, v: the block's samples at the output depth
template <int SIT> XC void fwd_block(const Fwd &F, const int (&p)[2][3][3], int (&y)[2][2], int &u, int &v)
{
XC_UNROLL
    for(int r = 0; r < 2; r++)
XC_UNROLL
        for(int k = 0; k < 2; k++) {
            const int64_t acc = F.m[0] * p[r][k + 1][0] + F.m[1] * p[r][k + 1][1] + F.m[2] * p[r][k + 1][2] + (F.oY << S) + ((int64_t)1 << (S - 1));
            y[r][k] = (int)clamp64(acc >> S, 0, F.maxv);
        }
    constexpr int L = SIT == SIT_CENTRE ? 2 : 3;
    int64_t       s[3];
XC_UNROLL
    for(int c = 0; c < 3; c++) {
        if constexpr(SIT == SIT_CENTRE) s[c] = (int64_t)p[0][1][c] + p[0][2][c] + p[1][1][c] + p[1][2][c];
        else s[c] = (int64_t)p[0][0][c] + 2 * (int64_t)p[0][1][c] + p[0][2][c] + p[1][0][c] + 2 * (int64_t)p[1][1][c] + p[1][2][c];
    }
    const int64_t off = (F.oC << (S + L)) + ((int64_t)1 << (S + L - 1));
    u = (int)clamp64((F.m[3] * s[0] + F.m[4] * s[1] + F.m[5] * s[2] + off) >> (S + L), 0, F.maxv);
    v = (int)clamp64((F.m[6] * s[0] + F.m[7] * s[1] + F.m[8] * s[2] + off) >> (S + L), 0, F.maxv);
}

// y[row][column]: the block's luma; cb, cr[r][k]: chroma rows cy - 1, cy, cy + 1 and columns cx - 1, cx, cx + 1, each clamped to the plane.
// out[row][column][R, G, B] as 16 bits
template <int SIT> XC void inv_block(const Inv &I, const int (&y)[2][2], const int (&cb)[3][3], const int (&cr)[3][3], int (&out)[2][2][3])
{
XC_UNROLL
    for(int dy = 0; dy < 2; dy++) {
        int vb[3], vr[3]; // vertical: the block's chroma row 3, the nearer neighbour 1
XC_UNROLL
        for(int k = 0; k < 3; k++) vb[k] = 3 * cb[1][k] + cb[dy ? 2 : 0][k], vr[k] = 3 * cr[1][k] + cr[dy ? 2 : 0][k];
XC_UNROLL
        for(int dx = 0; dx < 2; dx++) {
            int sb, sr;
            if constexpr(SIT == SIT_CENTRE) sb = 3 * vb[1] + vb[dx ? 2 : 0], sr = 3 * vr[1] + vr[dx ? 2 : 0];
            else sb = dx ? 2 * vb[1] + 2 * vb[2] : 4 * vb[1], sr = dx ? 2 * vr[1] + 2 * vr[2] : 4 * vr[1];
            const int64_t l = 16 * I.iY * ((int64_t)y[dy][dx] - I.oY) + ((int64_t)1 << (S + 3)), db = (int64_t)sb - 16 * I.oC, dr = (int64_t)sr - 16 * I.oC;
            out[dy][dx][0] = (int)clamp64((l + I.rCr * dr) >> (S + 4), 0, 65535);
            out[dy][dx][1] = (int)clamp64((l + I.gCb * db + I.gCr * dr) >> (S + 4), 0, 65535);
            out[dy][dx][2] = (int)clamp64((l + I.bCb * db) >> (S + 4), 0, 65535);
        }
    }
}

// ---- host only: the coefficients, exact -------------------------------------------------------
typedef __int128 i128;
inline int64_t rnd_div(i128 num, i128 den) // round half away from zero; den > 0
{
    const bool neg = num < 0;
    const i128 q = ((neg ? -num : num) * 2 + den) / (2 * den);
    return (int64_t)(neg ? -q : q);
}
// matrix: 0 bt601, 1 bt709, 2 bt2020nc; depth 8 | 10 sets the forward side, the inverse side is always the codec's 10 bits.  false: outside the set
inline bool matrix(int mat, int full_range, int depth, Fwd &F, Inv &I)
{
    static const int KR[3] = {2990, 2126, 2627}, KB[3] = {1140, 722, 593}; // in 1 / 10000
    if(mat < 0 || mat > 2 || (full_range != 0 && full_range != 1) || (depth != 8 && depth != 10)) return false;
    const i128 D = 10000, kr = KR[mat], kb = KB[mat], kg = D - kr - kb, one = (i128)1 << S, U = 65535;
    const i128 sY = full_range ? (1 << depth) - 1 : 219 << (depth - 8), sC = full_range ? (1 << depth) - 1 : 224 << (depth - 8);
    F.m[0] = rnd_div(sY * one * kr, U * D), F.m[2] = rnd_div(sY * one * kb, U * D), F.m[1] = rnd_div(sY * one, U) - F.m[0] - F.m[2];
    F.m[5] = rnd_div(sC * one, 2 * U), F.m[3] = rnd_div(-(sC * one * kr), U * 2 * (D - kb)), F.m[4] = -F.m[5] - F.m[3];
    F.m[6] = rnd_div(sC * one, 2 * U), F.m[8] = rnd_div(-(sC * one * kb), U * 2 * (D - kr)), F.m[7] = -F.m[6] - F.m[8];
    F.oY = full_range ? 0 : 16 << (depth - 8), F.oC = 1 << (depth - 1), F.maxv = (1 << depth) - 1, F.reserved = 0;
    const i128 tY = full_range ? 1023 : 219 << 2, tC = full_range ? 1023 : 224 << 2; // the inverse: d = 10
    I.iY = rnd_div(U * one, tY);
    I.rCr = rnd_div(2 * (D - kr) * U * one, D * tC), I.bCb = rnd_div(2 * (D - kb) * U * one, D * tC);
    I.gCb = rnd_div(-(2 * kb * (D - kb) * U * one), D * kg * tC), I.gCr = rnd_div(-(2 * kr * (D - kr) * U * one), D * kg * tC);
    I.oY = full_range ? 0 : 64, I.oC = 512;
    return true;
}

// ---- host only: whole pictures through the block functions, any strides (the restatement's counterpart; color.hip's kernels differ in how they load and store only) ----
inline int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
template <int DT, int SIT, typename OUT> void forward_picture(const Fwd &F, const void *rgb, int64_t sx, int64_t sy, int64_t sc, int w, int h, OUT *yuv)
{
    OUT *Y = yuv, *U = yuv + (int64_t)w * h, *V = U + (int64_t)(w / 2) * (h / 2);
    for(int j = 0; j < h / 2; j++)
        for(int i = 0; i < w / 2; i++) {
            int p[2][3][3] = {}, y[2][2], u, v;
            for(int r = 0; r < 2; r++)
                for(int k = (SIT == SIT_LEFT ? 0 : 1); k < 3; k++)
                    for(int c = 0; c < 3; c++) p[r][k][c] = c16_load<DT>(rgb, (int64_t)(2 * j + r) * sy + (int64_t)clampi(2 * i - 1 + k, 0, w - 1) * sx + c * sc);
            fwd_block<SIT>(F, p, y, u, v);
            for(int r = 0; r < 2; r++)
                for(int k = 0; k < 2; k++) Y[(int64_t)(2 * j + r) * w + 2 * i + k] = (OUT)y[r][k];
            U[(int64_t)j * (w / 2) + i] = (OUT)u, V[(int64_t)j * (w / 2) + i] = (OUT)v;
        }
}
template <int DT, int SIT> void inverse_picture(const Inv &I, const uint16_t *yuv, int w, int h, void *rgb, int64_t sx, int64_t sy, int64_t sc)
{
    const int       cw = w / 2, ch = h / 2;
    const uint16_t *Y = yuv, *U = yuv + (int64_t)w * h, *V = U + (int64_t)cw * ch;
    typename Elem<DT>::type *o = static_cast<typename Elem<DT>::type *>(rgb);
    for(int j = 0; j < ch; j++)
        for(int i = 0; i < cw; i++) {
            int y[2][2], cb[3][3], cr[3][3], out[2][2][3];
            for(int r = 0; r < 2; r++)
                for(int k = 0; k < 2; k++) y[r][k] = Y[(int64_t)(2 * j + r) * w + 2 * i + k];
            for(int r = 0; r < 3; r++)
                for(int k = 0; k < 3; k++) {
                    const int64_t at = (int64_t)clampi(j - 1 + r, 0, ch - 1) * cw + clampi(i - 1 + k, 0, cw - 1);
                    cb[r][k] = U[at], cr[r][k] = V[at];
                }
            inv_block<SIT>(I, y, cb, cr, out);
            for(int r = 0; r < 2; r++)
                for(int k = 0; k < 2; k++)
                    for(int c = 0; c < 3; c++) o[(int64_t)(2 * j + r) * sy + (int64_t)(2 * i + k) * sx + c * sc] = out_elem<DT>(out[r][k][c]);
        }
}

} // namespace xcol
