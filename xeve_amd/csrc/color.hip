// xeve_amd/csrc/color.hip -- the front door for tensors: RGB of any torch view (uint8 / float16 / bfloat16 / float32, strides in elements) <-> the planar 4:2:0 frames
// xeve_hip_enc_push takes and xeve_hip_enc_recon hands out.  The reference has nothing of the kind (its application reads and writes Y'CbCr files); the arithmetic is
// this project's own, all integer, in color_core.h -- the same source tests/native/color_host.cpp runs on the host.
//   xeve_hip_rgb_to_yuv420   RGB -> Y, U, V at 8 bits (one byte per sample) or 10 bits (16-bit little-endian), chroma filtered for siting left or centre
//   xeve_hip_yuv420_to_rgb   10-bit Y, U, V -> RGB, chroma interpolated bilinearly for the same sitings
//   xeve_hip_color_matrix    the coefficients both use (host only)
// Both are bandwidth kernels shaped as frames.hip's: a lane owns whole 2x2 blocks (the unit a chroma sample belongs to), CL_TURNS of them, consecutive lanes on consecutive
// blocks of a row; a block's luma pairs go out (come in) as one 2- or 4-byte access, its chroma as one sample per plane -- consecutive lanes, consecutive samples.  The
// tensor side is read / written by the element type and the layout the TEMPLATE says: strided (any view), planar (stride_x 1: a block row's two pixels are neighbours
// in each component plane) or interleaved (stride_c 1, stride_x 3: a block row is six neighbouring elements).  No LDS, no scratch; all addressing is 64-bit; the picture
// index is blockIdx.y.  Nothing outside the described samples is read or written: the left siting's column 2i - 1 and the inverse's chroma neighbours are clamped.
#include "xh_common.h"
#include "color_core.h"

namespace {
using namespace xcol;
constexpr int CL_THREADS = 256;
constexpr int CL_TURNS = 4; // blocks per thread
enum { LAY_STRIDED = 0, LAY_PLANAR = 1, LAY_INTERLEAVED = 2 };
typedef uint32_t cl_u32_a2 __attribute__((aligned(2)));
typedef uint16_t cl_u16_a1 __attribute__((aligned(1)));

struct ClFwdArgs {
    const void *rgb;
    long long   sx, sy, sc, sp; // elements
    uint8_t    *yuv;
    long long   yuv_pic;        // bytes
    int         w, h;
    Fwd         F;
};
struct ClInvArgs {
    const uint16_t *yuv;
    long long       yuv_pic; // samples
    void           *rgb;
    long long       sx, sy, sc, sp;
    int             w, h;
    Inv             I;
};

// SB: bytes per output sample.  grid: (2x2 blocks of a picture / (CL_THREADS * CL_TURNS), pictures)
template <int DT, int LAY, int SIT, int SB> __global__ void __launch_bounds__(CL_THREADS) k_rgb_to_yuv420(ClFwdArgs A)
{
    typedef typename Elem<DT>::type E;
    const E        *src = static_cast<const E *>(A.rgb) + (long long)blockIdx.y * A.sp;
    uint8_t        *dst = A.yuv + (long long)blockIdx.y * A.yuv_pic;
    const int       bw = A.w >> 1, n = bw * (A.h >> 1); // at most 4096 * 2160
    const long long nl = (long long)A.w * A.h, nc = nl >> 2;
    for(int t = 0, b = blockIdx.x * CL_THREADS + threadIdx.x; t < CL_TURNS && b < n; t++, b += gridDim.x * CL_THREADS) {
        const int j = b / bw, i = b - j * bw;
        int       p[2][3][3], y[2][2], u, v;
#pragma unroll
        for(int r = 0; r < 2; r++) {
            const E *row = src + (long long)(2 * j + r) * A.sy;
            if constexpr(LAY == LAY_INTERLEAVED) {
                E e[6];
                __builtin_memcpy(e, row + 6LL * i, sizeof(e));
#pragma unroll
                for(int k = 0; k < 2; k++)
#pragma unroll
                    for(int c = 0; c < 3; c++) p[r][k + 1][c] = c16_elem<DT>(e[3 * k + c]);
            }
            else if constexpr(LAY == LAY_PLANAR) {
#pragma unroll
                for(int c = 0; c < 3; c++) {
                    E e[2];
                    __builtin_memcpy(e, row + c * A.sc + 2LL * i, sizeof(e));
                    p[r][1][c] = c16_elem<DT>(e[0]), p[r][2][c] = c16_elem<DT>(e[1]);
                }
            }
            else {
#pragma unroll
                for(int k = 0; k < 2; k++)
#pragma unroll
                    for(int c = 0; c < 3; c++) p[r][k + 1][c] = c16_load<DT>(row, (2LL * i + k) * A.sx + c * A.sc);
            }
            if constexpr(SIT == SIT_LEFT) {
                const long long at = (long long)(i ? 2 * i - 1 : 0) * A.sx;
#pragma unroll
                for(int c = 0; c < 3; c++) p[r][0][c] = c16_load<DT>(row, at + c * A.sc);
            }
            else p[r][0][0] = p[r][0][1] = p[r][0][2] = 0;
        }
        fwd_block<SIT>(A.F, p, y, u, v);
        const long long at_l = (long long)(2 * j) * A.w + 2 * i, at_c = (long long)j * bw + i;
        if constexpr(SB == 1) {
            *reinterpret_cast<cl_u16_a1 *>(dst + at_l) = (uint16_t)(y[0][0] | (y[0][1] << 8));
            *reinterpret_cast<cl_u16_a1 *>(dst + at_l + A.w) = (uint16_t)(y[1][0] | (y[1][1] << 8));
            dst[nl + at_c] = (uint8_t)u, dst[nl + nc + at_c] = (uint8_t)v;
        }
        else {
            uint16_t *d16 = reinterpret_cast<uint16_t *>(dst);
            *reinterpret_cast<cl_u32_a2 *>(d16 + at_l) = (uint32_t)y[0][0] | ((uint32_t)y[0][1] << 16);
            *reinterpret_cast<cl_u32_a2 *>(d16 + at_l + A.w) = (uint32_t)y[1][0] | ((uint32_t)y[1][1] << 16);
            d16[nl + at_c] = (uint16_t)u, d16[nl + nc + at_c] = (uint16_t)v;
        }
    }
}

template <int DT, int LAY, int SIT> __global__ void __launch_bounds__(CL_THREADS) k_yuv420_to_rgb(ClInvArgs A)
{
    typedef typename Elem<DT>::type E;
    const uint16_t *src = A.yuv + (long long)blockIdx.y * A.yuv_pic;
    E              *dst = static_cast<E *>(A.rgb) + (long long)blockIdx.y * A.sp;
    const int       bw = A.w >> 1, bh = A.h >> 1, n = bw * bh;
    const long long nl = (long long)A.w * A.h, nc = nl >> 2;
    for(int t = 0, b = blockIdx.x * CL_THREADS + threadIdx.x; t < CL_TURNS && b < n; t++, b += gridDim.x * CL_THREADS) {
        const int j = b / bw, i = b - j * bw;
        int       y[2][2], cb[3][3], cr[3][3], out[2][2][3];
#pragma unroll
        for(int r = 0; r < 2; r++) {
            const uint32_t two = *reinterpret_cast<const cl_u32_a2 *>(src + (long long)(2 * j + r) * A.w + 2 * i);
            y[r][0] = (int)(two & 0xFFFFu), y[r][1] = (int)(two >> 16);
        }
        const int cols[3] = {i ? i - 1 : 0, i, i + 1 < bw ? i + 1 : bw - 1}, rows[3] = {j ? j - 1 : 0, j, j + 1 < bh ? j + 1 : bh - 1};
#pragma unroll
        for(int r = 0; r < 3; r++)
#pragma unroll
            for(int k = 0; k < 3; k++) {
                const long long at = nl + (long long)rows[r] * bw + cols[k];
                cb[r][k] = src[at], cr[r][k] = src[at + nc];
            }
        inv_block<SIT>(A.I, y, cb, cr, out);
#pragma unroll
        for(int r = 0; r < 2; r++) {
            E *row = dst + (long long)(2 * j + r) * A.sy;
            if constexpr(LAY == LAY_INTERLEAVED) {
                E e[6];
#pragma unroll
                for(int k = 0; k < 2; k++)
#pragma unroll
                    for(int c = 0; c < 3; c++) e[3 * k + c] = out_elem<DT>(out[r][k][c]);
                __builtin_memcpy(row + 6LL * i, e, sizeof(e));
            }
            else if constexpr(LAY == LAY_PLANAR) {
#pragma unroll
                for(int c = 0; c < 3; c++) {
                    const E e[2] = {out_elem<DT>(out[r][0][c]), out_elem<DT>(out[r][1][c])};
                    __builtin_memcpy(row + c * A.sc + 2LL * i, e, sizeof(e));
                }
            }
            else {
#pragma unroll
                for(int k = 0; k < 2; k++)
#pragma unroll
                    for(int c = 0; c < 3; c++) row[(2LL * i + k) * A.sx + c * A.sc] = out_elem<DT>(out[r][k][c]);
            }
        }
    }
}

dim3 cl_grid(int w, int h, int npics)
{
    const long blocks = (long)(w / 2) * (h / 2);
    return dim3((unsigned)((blocks + CL_THREADS * CL_TURNS - 1) / (CL_THREADS * CL_TURNS)), (unsigned)npics, 1);
}
// the template a call runs: chosen once on the host
template <int DT, int LAY, int SIT> void cl_fwd_sb(int sb, dim3 g, hipStream_t st, const ClFwdArgs &A)
{
    if(sb == 1) k_rgb_to_yuv420<DT, LAY, SIT, 1><<<g, CL_THREADS, 0, st>>>(A);
    else k_rgb_to_yuv420<DT, LAY, SIT, 2><<<g, CL_THREADS, 0, st>>>(A);
}
template <int DT, int LAY> void cl_fwd_sit(int sit, int sb, dim3 g, hipStream_t st, const ClFwdArgs &A)
{
    if(sit == SIT_LEFT) cl_fwd_sb<DT, LAY, SIT_LEFT>(sb, g, st, A);
    else cl_fwd_sb<DT, LAY, SIT_CENTRE>(sb, g, st, A);
}
template <int DT> void cl_fwd_lay(int lay, int sit, int sb, dim3 g, hipStream_t st, const ClFwdArgs &A)
{
    if(lay == LAY_INTERLEAVED) cl_fwd_sit<DT, LAY_INTERLEAVED>(sit, sb, g, st, A);
    else if(lay == LAY_PLANAR) cl_fwd_sit<DT, LAY_PLANAR>(sit, sb, g, st, A);
    else cl_fwd_sit<DT, LAY_STRIDED>(sit, sb, g, st, A);
}
template <int DT, int LAY> void cl_inv_sit(int sit, dim3 g, hipStream_t st, const ClInvArgs &A)
{
    if(sit == SIT_LEFT) k_yuv420_to_rgb<DT, LAY, SIT_LEFT><<<g, CL_THREADS, 0, st>>>(A);
    else k_yuv420_to_rgb<DT, LAY, SIT_CENTRE><<<g, CL_THREADS, 0, st>>>(A);
}
template <int DT> void cl_inv_lay(int lay, int sit, dim3 g, hipStream_t st, const ClInvArgs &A)
{
    if(lay == LAY_INTERLEAVED) cl_inv_sit<DT, LAY_INTERLEAVED>(sit, g, st, A);
    else if(lay == LAY_PLANAR) cl_inv_sit<DT, LAY_PLANAR>(sit, g, st, A);
    else cl_inv_sit<DT, LAY_STRIDED>(sit, g, st, A);
}

int  cl_elem_bytes(int dtype) { return dtype == DT_U8 ? 1 : dtype == DT_F32 ? 4 : 2; }
int  cl_layout(const xeve_hip_rgb_desc *d) { return d->stride_c == 1 && d->stride_x == 3 ? LAY_INTERLEAVED : d->stride_x == 1 ? LAY_PLANAR : LAY_STRIDED; }
bool cl_aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
bool cl_color_ok(const xeve_hip_color *c)
{
    return c && c->matrix >= 0 && c->matrix <= 2 && (c->full_range == 0 || c->full_range == 1) && (c->siting == 0 || c->siting == 1) && (c->depth == 8 || c->depth == 10);
}
bool cl_on_device(const void *p)
{
    hipPointerAttribute_t a;
    if(hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeDevice;
}
constexpr long long CL_MAX_STRIDE = 1LL << 40; // (row * stride_y and picture * stride_pic stay far inside 64 bits)
} // namespace

extern "C" int xeve_hip_color_matrix(const xeve_hip_color *color, int64_t fwd[9], int64_t fwd_off[2], int64_t inv[5])
{
    Fwd F;
    Inv I;
    if(!cl_color_ok(color) || !fwd || !fwd_off || !inv || !matrix(color->matrix, color->full_range, color->depth, F, I)) {
        xh_set_error("invalid argument: xeve_hip_color_matrix takes matrix 0 .. 2, full_range 0 | 1, siting 0 | 1, depth 8 | 10 and three outputs");
        return XEVE_HIP_ERR_ARG;
    }
    for(int k = 0; k < 9; k++) fwd[k] = F.m[k];
    fwd_off[0] = F.oY, fwd_off[1] = F.oC;
    inv[0] = I.iY, inv[1] = I.rCr, inv[2] = I.gCb, inv[3] = I.gCr, inv[4] = I.bCb;
    return XEVE_HIP_OK;
}

extern "C" int xeve_hip_rgb_to_yuv420(const void *rgb, const xeve_hip_rgb_desc *desc, const xeve_hip_color *color, int w, int h, int npics, void *yuv, int64_t yuv_pic_bytes,
                                      void *stream)
{
    XH_ENTER();
    XH_REQUIRE(rgb && desc && yuv && cl_color_ok(color) && npics >= 1 && npics <= 65535);
    XH_REQUIRE(w >= 2 && h >= 2 && (w & 1) == 0 && (h & 1) == 0 && w <= 8192 && h <= 4320);
    XH_REQUIRE(desc->dtype >= DT_U8 && desc->dtype <= DT_F32);
    XH_REQUIRE(desc->stride_x >= 0 && desc->stride_y >= 0 && desc->stride_c >= 0 && desc->stride_pic >= 0); // (0: an expanded axis)
    XH_REQUIRE(desc->stride_x <= CL_MAX_STRIDE && desc->stride_y <= CL_MAX_STRIDE && desc->stride_c <= CL_MAX_STRIDE && desc->stride_pic <= CL_MAX_STRIDE);
    const int sb = color->depth > 8 ? 2 : 1;
    XH_REQUIRE(cl_aligned(rgb, cl_elem_bytes(desc->dtype)) && cl_aligned(yuv, sb) && (yuv_pic_bytes & (sb - 1)) == 0 && yuv_pic_bytes >= (int64_t)w * h * 3 / 2 * sb);
    XH_REQUIRE(cl_on_device(rgb) && cl_on_device(yuv));
    ClFwdArgs A = {};
    Inv       I;
    A.rgb = rgb, A.sx = desc->stride_x, A.sy = desc->stride_y, A.sc = desc->stride_c, A.sp = desc->stride_pic, A.yuv = static_cast<uint8_t *>(yuv), A.yuv_pic = yuv_pic_bytes;
    A.w = w, A.h = h;
    XH_REQUIRE(matrix(color->matrix, color->full_range, color->depth, A.F, I));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3  g = cl_grid(w, h, npics);
    const int   lay = cl_layout(desc);
    switch(desc->dtype) {
    case DT_U8: cl_fwd_lay<DT_U8>(lay, color->siting, sb, g, st, A); break;
    case DT_F16: cl_fwd_lay<DT_F16>(lay, color->siting, sb, g, st, A); break;
    case DT_BF16: cl_fwd_lay<DT_BF16>(lay, color->siting, sb, g, st, A); break;
    default: cl_fwd_lay<DT_F32>(lay, color->siting, sb, g, st, A); break;
    }
    XH_HIP(hipGetLastError());
    return XEVE_HIP_OK;
}

extern "C" int xeve_hip_yuv420_to_rgb(const uint16_t *yuv, int64_t yuv_pic_samples, const xeve_hip_color *color, int w, int h, int npics, void *rgb, const xeve_hip_rgb_desc *desc,
                                      void *stream)
{
    XH_ENTER();
    XH_REQUIRE(rgb && desc && yuv && cl_color_ok(color) && color->depth == 10 && npics >= 1 && npics <= 65535); // (the codec's reconstruction is 10-bit)
    XH_REQUIRE(w >= 2 && h >= 2 && (w & 1) == 0 && (h & 1) == 0 && w <= 8192 && h <= 4320);
    XH_REQUIRE(desc->dtype >= DT_U8 && desc->dtype <= DT_F32);
    XH_REQUIRE(desc->stride_x >= 1 && desc->stride_y >= 1 && desc->stride_c >= 1 && desc->stride_pic >= (npics > 1 ? 1 : 0)); // (an output: every element is a place of its own)
    XH_REQUIRE(desc->stride_x <= CL_MAX_STRIDE && desc->stride_y <= CL_MAX_STRIDE && desc->stride_c <= CL_MAX_STRIDE && desc->stride_pic <= CL_MAX_STRIDE);
    XH_REQUIRE(cl_aligned(rgb, cl_elem_bytes(desc->dtype)) && cl_aligned(yuv, 2) && yuv_pic_samples >= (int64_t)w * h * 3 / 2);
    XH_REQUIRE(cl_on_device(rgb) && cl_on_device(yuv));
    ClInvArgs A = {};
    Fwd       F;
    A.yuv = yuv, A.yuv_pic = yuv_pic_samples, A.rgb = rgb, A.sx = desc->stride_x, A.sy = desc->stride_y, A.sc = desc->stride_c, A.sp = desc->stride_pic, A.w = w, A.h = h;
    XH_REQUIRE(matrix(color->matrix, color->full_range, color->depth, F, A.I));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3  g = cl_grid(w, h, npics);
    const int   lay = cl_layout(desc);
    switch(desc->dtype) {
    case DT_U8: cl_inv_lay<DT_U8>(lay, color->siting, g, st, A); break;
    case DT_F16: cl_inv_lay<DT_F16>(lay, color->siting, g, st, A); break;
    case DT_BF16: cl_inv_lay<DT_BF16>(lay, color->siting, g, st, A); break;
    default: cl_inv_lay<DT_F32>(lay, color->siting, g, st, A); break;
    }
    XH_HIP(hipGetLastError());
    return XEVE_HIP_OK;
}
