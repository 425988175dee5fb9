// xeve_amd/csrc/scale.hip -- the front door for decoded pictures: a decoder's surface (NV12 / P010 or planar, rows a pitch apart, at the SOURCE's size) -> the planar 4:2:0
// frames xeve_hip_enc_push takes, at the run's size.  The reference has nothing of the kind (its application reads Y'CbCr files of the coded size); the arithmetic is this
// project's own, all integer, in scale_core.h -- the same source tests/native/scale_host.cpp runs on the host.
//   xeve_hip_scale_filter        one axis' table: stretched Catmull-Rom at the exact centres, 14 fractional bits, rows summing to 2^14 (host only)
//   xeve_hip_surface_to_yuv420   de-interleave, >> shift, pitch removal and the two-pass resampling in ONE kernel; three launches (Y, U, V) whatever npics is
// k_scale: a workgroup of 256 lanes owns a tile of SC_TW x SC_TH output samples of one plane of one picture (the picture is blockIdx.y).  The tile's source window --
// the rows and columns its taps reach, clamped to the plane -- goes through the horizontal pass ONCE, as many source rows per round as keep the staged segments within
// 16 KB (the whole window up to about 3 : 1, SC_RB rows at least): the rows' segments are loaded into LDS as 16-bit samples (16-byte chunks by the widest loads the chunk's
// address allows -- chunks of a row are 16 bytes apart, so the choice is uniform over the lanes of a row; the de-interleave of UV and the shift happen while the chunk is
// unpacked; a chunk the segment ends inside is read sample by sample, so no byte behind a row's last sample is touched), then every lane makes T of one output column
// for its share of the rows, into the tile's T block in LDS.  The vertical pass reads T columns out of LDS (a wave: one output row, 64 columns -- consecutive banks, the
// row's coefficients broadcast) and leaves the tile in LDS, from where it is stored in 16-byte chunks again by the widest stores the address allows (an 8-bit chroma row
// of odd length starts on any byte).  Coefficients and first taps of the tile's columns and rows are staged in LDS once (the columns' transposed: lanes of a wave read
// consecutive addresses); nothing is evaluated per lane.  All addressing is 64-bit.
// THE TABLES live in a cache of the library's own, keyed by (device, source length, destination length, kind): an axis is derived on first use (host, __int128), uploaded
// once and kept; they are freed at the first call after xeve_hip_shutdown or a re-bind, and a call that would take a device's share past 64 axes waits for that device
// and frees its axes.  Nothing is allocated unless the entry point is called.
#include <mutex>
#include <vector>

#include "xh_common.h"
#include "scale_core.h"

namespace {
using namespace xscl;
constexpr int SC_THREADS = 256;
constexpr int SC_TW = 64, SC_TH = 16; // the output tile
constexpr int SC_RB = 8;              // source rows per horizontal round at least ...
constexpr int SC_SEG = 8192;          // ... and as many as keep the segment block within this many samples (a 2 : 1 tile's whole window is one round)
constexpr int SC_CACHE = 64;          // axes kept

struct ScArgs {
    const uint8_t *src;          // the plane's first byte (interleaved chroma: the first pair's)
    long long      pitch, pic;   // bytes between the plane's rows / between consecutive pictures' planes
    uint8_t       *dst;          // the output plane of picture 0
    long long      dst_pic;      // bytes
    const int32_t *hfirst, *vfirst;
    const int16_t *hcoef, *vcoef;
    int            nth, ntv;     // taps per row of the two tables
    int            sw, sh, dw, dh; // the plane's source and destination size
    int            eoff;         // the component of an interleaved element
    int            shift, maxv;
    int            tiles_x;
    int            spitch;       // samples between the rows of the segment block (a multiple of 16)
    int            rows_max;     // rows of the T block
    int            rb;           // source rows per horizontal round
};

// 16 bytes at p, whatever p's alignment, as 4 little-endian dwords -- by the widest loads p allows
__device__ __forceinline__ void sc_read16(const uint8_t *__restrict__ p, unsigned (&d)[4])
{
    const unsigned a = (unsigned)reinterpret_cast<uintptr_t>(p);
    if(!(a & 15)) {
        const uint4 v = *reinterpret_cast<const uint4 *>(p);
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
    }
    else if(!(a & 7)) {
#pragma unroll
        for(int i = 0; i < 2; i++) {
            const uint2 v = reinterpret_cast<const uint2 *>(p)[i];
            d[2 * i] = v.x, d[2 * i + 1] = v.y;
        }
    }
    else if(!(a & 3)) {
#pragma unroll
        for(int i = 0; i < 4; i++) d[i] = reinterpret_cast<const unsigned *>(p)[i];
    }
    else if(!(a & 1)) {
#pragma unroll
        for(int i = 0; i < 4; i++) d[i] = (unsigned)reinterpret_cast<const uint16_t *>(p)[2 * i] | ((unsigned)reinterpret_cast<const uint16_t *>(p)[2 * i + 1] << 16);
    }
    else {
#pragma unroll
        for(int i = 0; i < 4; i++) d[i] = (unsigned)p[4 * i] | ((unsigned)p[4 * i + 1] << 8) | ((unsigned)p[4 * i + 2] << 16) | ((unsigned)p[4 * i + 3] << 24);
    }
}
__device__ __forceinline__ void sc_write16(uint8_t *__restrict__ p, const unsigned (&d)[4])
{
    const unsigned a = (unsigned)reinterpret_cast<uintptr_t>(p);
    if(!(a & 15)) *reinterpret_cast<uint4 *>(p) = make_uint4(d[0], d[1], d[2], d[3]);
    else if(!(a & 7)) {
#pragma unroll
        for(int i = 0; i < 2; i++) reinterpret_cast<uint2 *>(p)[i] = make_uint2(d[2 * i], d[2 * i + 1]);
    }
    else if(!(a & 3)) {
#pragma unroll
        for(int i = 0; i < 4; i++) reinterpret_cast<unsigned *>(p)[i] = d[i];
    }
    else if(!(a & 1)) {
#pragma unroll
        for(int i = 0; i < 4; i++) reinterpret_cast<uint16_t *>(p)[2 * i] = (uint16_t)d[i], reinterpret_cast<uint16_t *>(p)[2 * i + 1] = (uint16_t)(d[i] >> 16);
    }
    else {
#pragma unroll
        for(int i = 0; i < 4; i++) p[4 * i] = (uint8_t)d[i], p[4 * i + 1] = (uint8_t)(d[i] >> 8), p[4 * i + 2] = (uint8_t)(d[i] >> 16), p[4 * i + 3] = (uint8_t)(d[i] >> 24);
    }
}

// the LDS block, in 16-bit units behind the two int32 arrays; every part starts on a 16-byte boundary
__host__ __device__ inline int sc_round8(int v) { return (v + 7) & ~7; }
struct ScLds {
    int hc, vc, t, s, total_bytes;
};
__host__ __device__ inline ScLds sc_lds(int nth, int ntv, int spitch, int rows_max, int rb)
{
    ScLds     L;
    const int s_units = rb * spitch > SC_TH * SC_TW ? rb * spitch : SC_TH * SC_TW; // (the finished tile takes the segment block's place)
    L.hc = (SC_TW + SC_TH) * 2; // (behind hfirst[SC_TW], vfirst[SC_TH])
    L.vc = L.hc + sc_round8(nth * SC_TW);
    L.t = L.vc + sc_round8(SC_TH * ntv);
    L.s = L.t + sc_round8(rows_max * SC_TW);
    L.total_bytes = (L.s + s_units) * 2;
    return L;
}

// SBI: bytes per source container; ESTEP: containers per source element (2: interleaved UV); SBO: bytes per output sample (launched with SBO == SBI: the depth is one).
// grid: (tiles of the plane, pictures)
template <int SBI, int ESTEP, int SBO> __global__ void __launch_bounds__(SC_THREADS) k_scale(ScArgs A)
{
    extern __shared__ __align__(16) uint8_t sc_block[];
    const ScLds L = sc_lds(A.nth, A.ntv, A.spitch, A.rows_max, A.rb);
    int32_t    *sHf = reinterpret_cast<int32_t *>(sc_block), *sVf = sHf + SC_TW;
    int16_t    *sHc = reinterpret_cast<int16_t *>(sc_block) + L.hc, *sVc = reinterpret_cast<int16_t *>(sc_block) + L.vc, *sT = reinterpret_cast<int16_t *>(sc_block) + L.t;
    uint16_t   *sS = reinterpret_cast<uint16_t *>(sc_block) + L.s;
    const int   tid = threadIdx.x, nth = A.nth, ntv = A.ntv;
    const int   ty = blockIdx.x / A.tiles_x, tx = blockIdx.x - ty * A.tiles_x, x0 = tx * SC_TW, y0 = ty * SC_TH;
    const int   tw = min(SC_TW, A.dw - x0), th = min(SC_TH, A.dh - y0);
    constexpr int EB = SBI * ESTEP, NE = 16 / EB; // bytes per source element, elements per chunk

    for(int i = tid; i < tw; i += SC_THREADS) sHf[i] = A.hfirst[x0 + i];
    for(int i = tid; i < th; i += SC_THREADS) sVf[i] = A.vfirst[y0 + i];
    for(int i = tid; i < tw * nth; i += SC_THREADS) {
        const int x = i / nth, j = i - x * nth;
        sHc[j * SC_TW + x] = A.hcoef[(long long)(x0 + x) * nth + j];
    }
    for(int i = tid; i < th * ntv; i += SC_THREADS) sVc[i] = A.vcoef[(long long)y0 * ntv + i];
    // the tile's window (first taps do not decrease along an axis): columns lo .. hi, rows rlo .. rhi of the source plane
    const int lo = clampi(A.hfirst[x0], 0, A.sw - 1), hi = clampi(A.hfirst[x0 + tw - 1] + nth - 1, 0, A.sw - 1);
    const int rlo = clampi(A.vfirst[y0], 0, A.sh - 1), rhi = clampi(A.vfirst[y0 + th - 1] + ntv - 1, 0, A.sh - 1);
    const int nrows = rhi - rlo + 1, rowbytes = (hi - lo + 1) * EB, cpr = (rowbytes + 15) >> 4;
    const uint8_t *src = A.src + (long long)blockIdx.y * A.pic + (long long)rlo * A.pitch + (long long)lo * EB;
    const unsigned mask = (unsigned)A.maxv;
    __syncthreads();

    for(int g = 0; g < nrows; g += A.rb) {
        const int nr = min(A.rb, nrows - g);
        for(int i = tid; i < nr * cpr; i += SC_THREADS) {
            const int      r = i / cpr, c = i - r * cpr;
            const uint8_t *p = src + (long long)(g + r) * A.pitch + c * 16;
            uint16_t      *s = sS + r * A.spitch + c * NE;
            if(c * 16 + 16 <= rowbytes) {
                unsigned d[4], o[NE / 2];
                sc_read16(p, d);
#pragma unroll
                for(int k = 0; k < NE; k++) {
                    unsigned v;
                    if constexpr(SBI == 1 && ESTEP == 1) v = (d[k >> 2] >> (8 * (k & 3))) & 0xFFu;
                    else if constexpr(SBI == 1) v = (((d[k >> 1] >> (16 * (k & 1))) & 0xFFFFu) >> (8 * A.eoff)) & 0xFFu;
                    else if constexpr(ESTEP == 1) v = (d[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
                    else v = (d[k] >> (16 * A.eoff)) & 0xFFFFu;
                    v = (unsigned)sample_of(v, A.shift, mask);
                    if(k & 1) o[k >> 1] |= v << 16;
                    else o[k >> 1] = v;
                }
#pragma unroll
                for(int k = 0; k < NE / 2; k++) reinterpret_cast<unsigned *>(s)[k] = o[k];
            }
            else { // the segment ends inside this chunk: sample by sample
                const int left = (rowbytes - c * 16) / EB;
                for(int k = 0; k < left; k++) {
                    const unsigned v = SBI == 1 ? (unsigned)p[k * ESTEP + A.eoff] : (unsigned)reinterpret_cast<const uint16_t *>(p)[k * ESTEP + A.eoff];
                    s[k] = (uint16_t)sample_of(v, A.shift, mask);
                }
            }
        }
        __syncthreads();
        for(int i = tid; i < nr * SC_TW; i += SC_THREADS) {
            const int r = i / SC_TW, x = i - r * SC_TW;
            if(x < tw) sT[(g + r) * SC_TW + x] = (int16_t)hpass(sS + r * A.spitch, lo, A.sw, sHc + x, SC_TW, sHf[x], nth);
        }
        __syncthreads();
    }

    uint16_t *sO = sS; // (every read of the segment block is behind the last barrier)
    for(int i = tid; i < SC_TH * SC_TW; i += SC_THREADS) {
        const int y = i / SC_TW, x = i - y * SC_TW;
        if(y < th && x < tw) sO[i] = (uint16_t)vpass(sT + x, SC_TW, rlo, A.sh, sVc + y * ntv, 1, sVf[y], ntv, A.maxv);
    }
    __syncthreads();

    constexpr int NO = 16 / SBO; // samples per output chunk
    const int     outbytes = tw * SBO, cpo = (outbytes + 15) >> 4;
    uint8_t      *dst = A.dst + (long long)blockIdx.y * A.dst_pic + ((long long)y0 * A.dw + x0) * SBO;
    for(int i = tid; i < th * cpo; i += SC_THREADS) {
        const int       y = i / cpo, c = i - y * cpo;
        uint8_t        *q = dst + (long long)y * A.dw * SBO + c * 16;
        const uint16_t *o = sO + y * SC_TW + c * NO;
        if(c * 16 + 16 <= outbytes) {
            unsigned d[4];
#pragma unroll
            for(int k = 0; k < 4; k++) {
                if constexpr(SBO == 2) d[k] = reinterpret_cast<const unsigned *>(o)[k];
                else d[k] = (unsigned)o[4 * k] | ((unsigned)o[4 * k + 1] << 8) | ((unsigned)o[4 * k + 2] << 16) | ((unsigned)o[4 * k + 3] << 24);
            }
            sc_write16(q, d);
        }
        else { // the tile's row ends inside this chunk
            const int left = (outbytes - c * 16) / SBO;
            for(int k = 0; k < left; k++) {
                if constexpr(SBO == 2) reinterpret_cast<uint16_t *>(q)[k] = o[k];
                else q[k] = (uint8_t)o[k];
            }
        }
    }
}

// ---- the tables on the device ------------------------------------------------------------------
struct ScAxis {
    int      device = -1, src_n = 0, dst_n = 0, kind = 0;
    Axis     A;                       // (the host copy: the windows are sized from it)
    int      span_w = 0, span_h = 0;  // the widest window of a tile of SC_TW columns / the tallest of a tile of SC_TH rows, in source samples
    int32_t *d_first = nullptr;
    int16_t *d_coef = nullptr;
};
struct ScCache {
    std::mutex           mu;
    uint32_t             gen = 0;
    std::vector<ScAxis*> axes;
    void drop(bool free_them)
    {
        for(ScAxis *a : axes) {
            if(free_them) (void)hipFree(a->d_first), (void)hipFree(a->d_coef);
            delete a;
        }
        axes.clear();
    }
} g_scale;

int sc_span(const Axis &A, int tile)
{
    int span = 1;
    for(int i0 = 0; i0 < A.dn; i0 += tile) {
        const int i1 = i0 + tile < A.dn ? i0 + tile : A.dn;
        const int lo = clampi(A.first[i0], 0, A.sn - 1), hi = clampi(A.first[i1 - 1] + A.ntaps - 1, 0, A.sn - 1);
        if(hi - lo + 1 > span) span = hi - lo + 1;
    }
    return span;
}
struct ScKey {
    int src_n, dst_n, kind;
};
const ScAxis *sc_find(int dev, const ScKey &k)
{
    for(const ScAxis *a : g_scale.axes)
        if(a->device == dev && a->src_n == k.src_n && a->dst_n == k.dst_n && a->kind == k.kind) return a;
    return nullptr;
}
// room for those of the n axes that are not cached yet (the caller holds g_scale.mu).  A call whose axes are all there touches nothing; one that would take the current
// device's share past SC_CACHE waits for that device -- launches on any of its streams may still read the tables -- and frees that device's axes, no other's
bool sc_room(const ScKey *keys, int n)
{
    ScCache &C = g_scale;
    int      dev = 0, have = 0, missing = 0;
    if(hipGetDevice(&dev) != hipSuccess) { xh_set_error("hipGetDevice failed"); return false; }
    if(C.gen != xh_generation()) C.drop(true), C.gen = xh_generation(); // (shut down or re-bound since: both have waited for the device, and neither frees these tables)
    for(const ScAxis *a : C.axes) have += a->device == dev;
    for(int i = 0; i < n; i++) {
        bool twice = false;
        for(int j = 0; j < i; j++) twice = twice || (keys[j].src_n == keys[i].src_n && keys[j].dst_n == keys[i].dst_n && keys[j].kind == keys[i].kind);
        missing += !twice && !sc_find(dev, keys[i]);
    }
    if(have + missing <= SC_CACHE) return true;
    if(hipDeviceSynchronize() != hipSuccess) { xh_set_error("hipDeviceSynchronize failed"); return false; }
    std::vector<ScAxis *> kept;
    for(ScAxis *a : C.axes) {
        if(a->device != dev) { kept.push_back(a); continue; }
        (void)hipFree(a->d_first), (void)hipFree(a->d_coef);
        delete a;
    }
    C.axes.swap(kept);
    return true;
}
// the axis' device tables (the caller holds g_scale.mu and has made room); NULL with the error set
const ScAxis *sc_axis(int src_n, int dst_n, int kind)
{
    ScCache &C = g_scale;
    int      dev = 0;
    if(hipGetDevice(&dev) != hipSuccess) { xh_set_error("hipGetDevice failed"); return nullptr; }
    if(const ScAxis *hit = sc_find(dev, ScKey{src_n, dst_n, kind})) return hit;
    ScAxis *a = new ScAxis;
    a->device = dev, a->src_n = src_n, a->dst_n = dst_n, a->kind = kind;
    if(!filter(src_n, dst_n, kind, a->A)) {
        delete a;
        xh_set_error("invalid argument: no filter table for %d -> %d samples (kind %d)", src_n, dst_n, kind);
        return nullptr;
    }
    a->span_w = sc_span(a->A, SC_TW), a->span_h = sc_span(a->A, SC_TH);
    const size_t fb = a->A.first.size() * sizeof(int32_t), cb = a->A.coef.size() * sizeof(int16_t);
    if(hipMalloc((void **)&a->d_first, fb) != hipSuccess || hipMalloc((void **)&a->d_coef, cb) != hipSuccess || hipMemcpy(a->d_first, a->A.first.data(), fb, hipMemcpyHostToDevice) != hipSuccess ||
       hipMemcpy(a->d_coef, a->A.coef.data(), cb, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(a->d_first), (void)hipFree(a->d_coef);
        delete a;
        xh_set_error("the filter tables could not be placed on the device");
        return nullptr;
    }
    C.axes.push_back(a);
    return a;
}

bool sc_aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
bool sc_on_device(const void *p)
{
    hipPointerAttribute_t a;
    if(hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeDevice;
}
constexpr long long SC_MAX_DIST = 1LL << 44; // (a pitch times 4320 rows and a picture distance times 65535 pictures stay inside 64 bits)

// source rows per horizontal round: the whole window where the segment block stays within SC_SEG samples, SC_RB rows at least
int sc_rounds(int spitch, int rows_max)
{
    const int fit = SC_SEG / spitch > SC_RB ? SC_SEG / spitch : SC_RB;
    return fit < rows_max ? fit : rows_max;
}
// the passes' 32-bit sums and 16-bit T are proven for this pair of tables, and a tile's block fits the LDS a launch may ask for
bool sc_fits(const ScAxis *H, const ScAxis *V, int depth)
{
    const int spitch = (H->span_w + 15) & ~15;
    return bounds_ok(H->A.sum_abs, V->A.sum_abs, depth) && sc_lds(H->A.ntaps, V->A.ntaps, spitch, V->span_h, sc_rounds(spitch, V->span_h)).total_bytes <= 64 * 1024;
}
// one plane of every picture: the launch
int sc_plane(const uint8_t *src, int sbi, int estep, int eoff, long long pitch, long long pic, int sw, int sh, const ScAxis *H, const ScAxis *V, int shift, int depth, uint8_t *dst,
             long long dst_pic, int npics, hipStream_t st)
{
    ScArgs A = {};
    A.src = src, A.pitch = pitch, A.pic = pic, A.dst = dst, A.dst_pic = dst_pic, A.hfirst = H->d_first, A.vfirst = V->d_first, A.hcoef = H->d_coef, A.vcoef = V->d_coef;
    A.nth = H->A.ntaps, A.ntv = V->A.ntaps, A.sw = sw, A.sh = sh, A.dw = H->A.dn, A.dh = V->A.dn, A.eoff = eoff, A.shift = shift, A.maxv = (1 << depth) - 1;
    A.tiles_x = (A.dw + SC_TW - 1) / SC_TW, A.spitch = (H->span_w + 15) & ~15, A.rows_max = V->span_h;
    A.rb = sc_rounds(A.spitch, A.rows_max);
    const ScLds L = sc_lds(A.nth, A.ntv, A.spitch, A.rows_max, A.rb);
    const dim3 g((unsigned)(A.tiles_x * ((A.dh + SC_TH - 1) / SC_TH)), (unsigned)npics, 1);
    if(sbi == 1 && estep == 1) k_scale<1, 1, 1><<<g, SC_THREADS, (size_t)L.total_bytes, st>>>(A); // (bytes in, bytes out; words in, words out: the depth is one)
    else if(sbi == 1) k_scale<1, 2, 1><<<g, SC_THREADS, (size_t)L.total_bytes, st>>>(A);
    else if(estep == 1) k_scale<2, 1, 2><<<g, SC_THREADS, (size_t)L.total_bytes, st>>>(A);
    else k_scale<2, 2, 2><<<g, SC_THREADS, (size_t)L.total_bytes, st>>>(A);
    return XEVE_HIP_OK;
}
} // namespace

extern "C" int xeve_hip_scale_filter(int src_n, int dst_n, int kind, int32_t *first, int16_t *coef, size_t cap, int *ntaps)
{
    Axis A;
    if(!first || !coef || !ntaps || !filter(src_n, dst_n, kind, A)) {
        xh_set_error("invalid argument: xeve_hip_scale_filter takes lengths of 1 .. 8192 (kind 1: even) no more than 8 : 1 apart, kind 0 | 1 and three outputs");
        return XEVE_HIP_ERR_ARG;
    }
    if(cap < A.coef.size()) {
        xh_set_error("invalid argument: xeve_hip_scale_filter needs room for %zu coefficients (%d rows of %d), cap is %zu", A.coef.size(), A.dn, A.ntaps, cap);
        return XEVE_HIP_ERR_ARG;
    }
    for(int i = 0; i < A.dn; i++) first[i] = A.first[i];
    for(size_t i = 0; i < A.coef.size(); i++) coef[i] = A.coef[i];
    *ntaps = A.ntaps;
    return XEVE_HIP_OK;
}

extern "C" int xeve_hip_surface_to_yuv420(const xeve_hip_surface *src, int sw, int sh, int siting, int w, int h, int depth, int npics, void *yuv, int64_t yuv_pic_bytes, void *stream)
{
    XH_ENTER();
    XH_REQUIRE(src && yuv && npics >= 1 && npics <= 65535 && (siting == 0 || siting == 1));
    XH_REQUIRE(sw >= 2 && sh >= 2 && (sw & 1) == 0 && (sh & 1) == 0 && sw <= 8192 && sh <= 4320);
    XH_REQUIRE(w >= 2 && h >= 2 && (w & 1) == 0 && (h & 1) == 0 && w <= 8192 && h <= 4320);
    XH_REQUIRE(sw <= MAX_RATIO * w && w <= MAX_RATIO * sw && sh <= MAX_RATIO * h && h <= MAX_RATIO * sh);
    XH_REQUIRE((src->layout == 0 || src->layout == 1) && (src->sample_bytes == 1 || src->sample_bytes == 2) && (src->depth == 8 || src->depth == 10));
    XH_REQUIRE(src->depth == depth); // (no conversion between depths: the frame has the surface's)
    const int sbi = src->sample_bytes, sbo = depth > 8 ? 2 : 1, semi = src->layout == 1;
    XH_REQUIRE((sbi == 1) == (depth == 8));                                 // (a byte holds 8 bits, a 16-bit word 10)
    XH_REQUIRE(src->shift == 0 || (sbi == 2 && src->shift == 16 - depth));  // (low-aligned, or msb-aligned in a 16-bit word)
    XH_REQUIRE(src->plane[0] && src->plane[1] && (semi || src->plane[2]));
    XH_REQUIRE(sc_aligned(src->plane[0], sbi) && sc_aligned(src->plane[1], sbi) && (semi || sc_aligned(src->plane[2], sbi)));
    XH_REQUIRE(src->pitch_l >= (int64_t)sw * sbi && src->pitch_c >= (int64_t)(sw / 2) * sbi * (semi ? 2 : 1) && src->pitch_l <= SC_MAX_DIST && src->pitch_c <= SC_MAX_DIST);
    XH_REQUIRE((src->pitch_l & (sbi - 1)) == 0 && (src->pitch_c & (sbi - 1)) == 0 && (src->pic_l & (sbi - 1)) == 0 && (src->pic_c & (sbi - 1)) == 0);
    XH_REQUIRE(src->pic_l >= 0 && src->pic_c >= 0 && src->pic_l <= SC_MAX_DIST && src->pic_c <= SC_MAX_DIST); // (0: one surface for every picture)
    const int64_t nl = (int64_t)w * h, nc = nl / 4, frame = (nl + 2 * nc) * sbo;
    XH_REQUIRE(sc_aligned(yuv, sbo) && (yuv_pic_bytes & (sbo - 1)) == 0 && yuv_pic_bytes >= frame);
    // the bytes either side spans: an output inside the source would be read while it is written
    const uintptr_t out0 = reinterpret_cast<uintptr_t>(yuv), out1 = out0 + (uint64_t)(npics - 1) * yuv_pic_bytes + frame;
    const int      nplanes = semi ? 2 : 3;
    for(int p = 0; p < nplanes; p++) {
        const int64_t  rows = p ? sh / 2 : sh, pitch = p ? src->pitch_c : src->pitch_l, pic = p ? src->pic_c : src->pic_l;
        const int64_t  rowb = p ? (int64_t)(sw / 2) * sbi * (semi ? 2 : 1) : (int64_t)sw * sbi;
        const uintptr_t s0 = reinterpret_cast<uintptr_t>(src->plane[p]), s1 = s0 + (uint64_t)(npics - 1) * pic + (rows - 1) * pitch + rowb;
        XH_REQUIRE(s1 <= out0 || out1 <= s0);
        XH_REQUIRE(sc_on_device(reinterpret_cast<const void *>(s0)) && sc_on_device(reinterpret_cast<const void *>(s1 - 1)));
    }
    XH_REQUIRE(sc_on_device(reinterpret_cast<const void *>(out0)) && sc_on_device(reinterpret_cast<const void *>(out1 - 1)));
    hipStream_t                 st = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lk(g_scale.mu); // (held over the launches: a call that empties the cache waits for them)
    const ScKey keys[4] = {{sw, w, KIND_PLAIN}, {sh, h, KIND_PLAIN}, siting == 0 ? ScKey{sw, w, KIND_LEFT} : ScKey{sw / 2, w / 2, KIND_PLAIN}, {sh / 2, h / 2, KIND_PLAIN}};
    if(!sc_room(keys, 4)) return XEVE_HIP_ERR_DEVICE;
    // tables: luma columns and rows; chroma columns by the siting, chroma rows (the exact centres depend on the lengths' ratio only, but every plane has its own table)
    const ScAxis *ax[4] = {};
    for(int i = 0; i < 4; i++)
        if(!(ax[i] = sc_axis(keys[i].src_n, keys[i].dst_n, keys[i].kind))) return XEVE_HIP_ERR_ARG;
    const ScAxis *hl = ax[0], *vl = ax[1], *hc = ax[2], *vc = ax[3];
    XH_REQUIRE(sc_fits(hl, vl, depth) && sc_fits(hc, vc, depth)); // (the narrowed types hold for THESE tables, or nothing is launched)
    uint8_t *out = static_cast<uint8_t *>(yuv);
    int      rc = sc_plane(static_cast<const uint8_t *>(src->plane[0]), sbi, 1, 0, src->pitch_l, src->pic_l, sw, sh, hl, vl, src->shift, depth, out, yuv_pic_bytes, npics, st);
    if(rc != XEVE_HIP_OK) return rc;
    for(int c = 0; c < 2; c++) {
        const uint8_t *plane = static_cast<const uint8_t *>(semi ? src->plane[1] : src->plane[1 + c]);
        rc = sc_plane(plane, sbi, semi ? 2 : 1, semi ? c : 0, src->pitch_c, src->pic_c, sw / 2, sh / 2, hc, vc, src->shift, depth, out + (nl + c * nc) * sbo, yuv_pic_bytes, npics, st);
        if(rc != XEVE_HIP_OK) return rc;
    }
    XH_HIP(hipGetLastError());
    return XEVE_HIP_OK;
}
