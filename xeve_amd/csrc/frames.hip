// xeve_amd/csrc/frames.hip -- the two ends of a picture whose size is even but no multiple of 8.  The reference codes ALIGN8(w) x ALIGN8(h) (xeve_enc.c:1574-1583): its
// application reads the w x h input into images of the coded size it zeroed once (xeve_app.c:1150-1153, imgb_read), and hands the reconstruction out narrowed to the
// cropping window again (XEVE_CFG_GET_RECON, xeve.c:268-278).  Here:
//   xeve_hip_frames_load   pushed frames (rows of src_w / src_w / 2 samples of one or two bytes, no padding) -> the W x H original planes at the codec's 10 bits, every
//                          sample right of the input and below it 0
//   xeve_hip_recon_crop    the cw x ch window at the top left of the stacked picture stores -> packed Y, U, V without padding (the application's -r layout)
// Both are bandwidth kernels with ONE aligned side: the planes of the codec (rows on 16-byte boundaries in luma, 8-byte in chroma -- a chroma row of 36 samples allows no
// more) are moved in whole chunks of 8 luma / 4 chroma samples, one vector access per lane, consecutive lanes on consecutive chunks of a row.  The packed side starts its
// rows wherever w puts them -- 2-byte boundaries, 1-byte for 8-bit chroma rows of odd length -- and is accessed by the widest units the chunk's address allows: the
// alignment of a chunk depends on its row only (chunks of a row are a whole chunk apart), so the choice is uniform over the lanes of a row.  Nothing is read or written
// outside the rows described; a chunk that the packed row ends inside is handled sample by sample.  All addressing is 64-bit (the stacked planes pass 2^32 samples); the
// picture index is blockIdx.y, the plane of a chroma launch blockIdx.z.
#include "xh_common.h"

namespace {
constexpr int FL_THREADS = 256;
constexpr int FL_TURNS = 4; // chunks per thread

// B contiguous bytes (4, 8 or 16) at p, whatever p's alignment, as B / 4 little-endian dwords -- by the widest loads p allows
template <int B> __device__ __forceinline__ void fl_read(const uint8_t *__restrict__ p, unsigned (&d)[B / 4])
{
    const unsigned a = (unsigned)reinterpret_cast<uintptr_t>(p);
    if constexpr(B == 16) {
        if(!(a & 15)) {
            const uint4 v = *reinterpret_cast<const uint4 *>(p);
            d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
            return;
        }
    }
    if constexpr(B >= 8) {
        if(!(a & 7)) {
#pragma unroll
            for(int i = 0; i < B / 8; i++) {
                const uint2 v = reinterpret_cast<const uint2 *>(p)[i];
                d[2 * i] = v.x, d[2 * i + 1] = v.y;
            }
            return;
        }
    }
    if(!(a & 3)) {
#pragma unroll
        for(int i = 0; i < B / 4; i++) d[i] = reinterpret_cast<const unsigned *>(p)[i];
    }
    else if(!(a & 1)) {
#pragma unroll
        for(int i = 0; i < B / 4; i++) d[i] = (unsigned)reinterpret_cast<const uint16_t *>(p)[2 * i] | ((unsigned)reinterpret_cast<const uint16_t *>(p)[2 * i + 1] << 16);
    }
    else {
#pragma unroll
        for(int i = 0; i < B / 4; i++) d[i] = (unsigned)p[4 * i] | ((unsigned)p[4 * i + 1] << 8) | ((unsigned)p[4 * i + 2] << 16) | ((unsigned)p[4 * i + 3] << 24);
    }
}
// the same for stores; p is at least 2-byte aligned
template <int B> __device__ __forceinline__ void fl_write(uint8_t *__restrict__ p, const unsigned (&d)[B / 4])
{
    const unsigned a = (unsigned)reinterpret_cast<uintptr_t>(p);
    if constexpr(B == 16) {
        if(!(a & 15)) {
            *reinterpret_cast<uint4 *>(p) = make_uint4(d[0], d[1], d[2], d[3]);
            return;
        }
    }
    if constexpr(B >= 8) {
        if(!(a & 7)) {
#pragma unroll
            for(int i = 0; i < B / 8; i++) reinterpret_cast<uint2 *>(p)[i] = make_uint2(d[2 * i], d[2 * i + 1]);
            return;
        }
    }
    if(!(a & 3)) {
#pragma unroll
        for(int i = 0; i < B / 4; i++) reinterpret_cast<unsigned *>(p)[i] = d[i];
    }
    else {
#pragma unroll
        for(int i = 0; i < B / 4; i++) reinterpret_cast<uint16_t *>(p)[2 * i] = (uint16_t)d[i], reinterpret_cast<uint16_t *>(p)[2 * i + 1] = (uint16_t)(d[i] >> 16);
    }
}
// N 16-bit samples in N / 2 dwords to / from an aligned plane: one 16-byte (N = 8) or 8-byte (N = 4) access
template <int N> __device__ __forceinline__ void fl_store_chunk(uint16_t *__restrict__ p, const unsigned (&o)[N / 2])
{
    if constexpr(N == 8) *reinterpret_cast<uint4 *>(p) = make_uint4(o[0], o[1], o[2], o[3]);
    else *reinterpret_cast<uint2 *>(p) = make_uint2(o[0], o[1]);
}
template <int N> __device__ __forceinline__ void fl_load_chunk(const uint16_t *__restrict__ p, unsigned (&o)[N / 2])
{
    if constexpr(N == 8) {
        const uint4 v = *reinterpret_cast<const uint4 *>(p);
        o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
    }
    else {
        const uint2 v = *reinterpret_cast<const uint2 *>(p);
        o[0] = v.x, o[1] = v.y;
    }
}

struct FlArgs {
    const uint8_t *frames;
    long long      frame_dist;   // bytes between the frames of consecutive pictures
    long long      src_off[2];   // bytes from a frame's first byte to the launch's planes (blockIdx.z)
    uint16_t      *dst[2];
    long long      dst_pic;      // samples between consecutive pictures' planes
    int            src_wp, src_hp, wp, hp, s_dst; // the plane's input size, its coded size, the output stride (samples)
};
// SB: bytes per input sample; SHIFT: up to the codec's 10 bits; N: samples per chunk (8 luma, 4 chroma).  grid: (chunks of a plane / (FL_THREADS * FL_TURNS), pictures,
// planes of the launch)
template <int SB, int SHIFT, int N> __global__ void __launch_bounds__(FL_THREADS) k_frames_load(FlArgs A)
{
    const long long pic = blockIdx.y;
    const uint8_t  *src = A.frames + pic * A.frame_dist + A.src_off[blockIdx.z];
    uint16_t       *dst = A.dst[blockIdx.z] + pic * A.dst_pic;
    const int       cpr = A.wp / N, n = cpr * A.hp; // chunks per row / per plane (at most 8192 * 4320 / 8)
    for(int t = 0, i = blockIdx.x * FL_THREADS + threadIdx.x; t < FL_TURNS && i < n; t++, i += gridDim.x * FL_THREADS) {
        const int row = i / cpr, col = (i - row * cpr) * N;
        unsigned  o[N / 2];
#pragma unroll
        for(int k = 0; k < N / 2; k++) o[k] = 0;
        if(row < A.src_hp && col < A.src_wp) {
            const uint8_t *p = src + ((long long)row * A.src_wp + col) * SB;
            if(col + N <= A.src_wp) {
                unsigned d[N * SB / 4];
                fl_read<N * SB>(p, d);
                if constexpr(SB == 2) { // (handed to the codec as they are: the plain copy of the application's imgb_cpy)
                    static_assert(SHIFT == 0, "16-bit input is not shifted");
#pragma unroll
                    for(int k = 0; k < N / 2; k++) o[k] = d[k];
                }
                else {
#pragma unroll
                    for(int k = 0; k < N / 2; k++) { // samples 2k, 2k + 1: bytes 2k, 2k + 1 of the chunk
                        const unsigned w2 = d[k / 2] >> (16 * (k & 1));
                        o[k] = ((w2 & 0xFFu) << SHIFT) | (((w2 >> 8) & 0xFFu) << (16 + SHIFT));
                    }
                }
            }
            else { // the input row ends inside this chunk: sample by sample, the rest stays 0
                const int left = A.src_wp - col;
#pragma unroll
                for(int k = 0; k < N; k++) // (unrolled: the chunk stays in registers)
                    if(k < left) {
                        const unsigned v = SB == 2 ? (unsigned)reinterpret_cast<const uint16_t *>(p)[k] : (unsigned)p[k];
                        o[k >> 1] |= ((v << SHIFT) & 0xFFFFu) << (16 * (k & 1));
                    }
            }
        }
        fl_store_chunk<N>(dst + (long long)row * A.s_dst + col, o);
    }
}

struct RcArgs {
    const uint16_t *rec[2]; // blockIdx.z
    long long       out_off[2], rec_pic, out_pic;
    int             s_rec, cwp, chp; // the plane's stride and its window
};
template <int N> __global__ void __launch_bounds__(FL_THREADS) k_recon_crop(RcArgs A, uint16_t *__restrict__ out)
{
    const long long pic = blockIdx.y;
    const uint16_t *rec = A.rec[blockIdx.z] + pic * A.rec_pic;
    uint16_t       *dst = out + pic * A.out_pic + A.out_off[blockIdx.z];
    const int       cpr = (A.cwp + N - 1) / N, n = cpr * A.chp;
    for(int t = 0, i = blockIdx.x * FL_THREADS + threadIdx.x; t < FL_TURNS && i < n; t++, i += gridDim.x * FL_THREADS) {
        const int row = i / cpr, col = (i - row * cpr) * N;
        unsigned  o[N / 2];
        fl_load_chunk<N>(rec + (long long)row * A.s_rec + col, o); // (whole: the row's stride holds the chunk the window ends inside)
        uint16_t *q = dst + (long long)row * A.cwp + col;
        if(col + N <= A.cwp) fl_write<N * 2>(reinterpret_cast<uint8_t *>(q), o);
        else {
            const int left = A.cwp - col;
#pragma unroll
            for(int k = 0; k < N; k++)
                if(k < left) q[k] = (uint16_t)(o[k >> 1] >> (16 * (k & 1)));
        }
    }
}

bool fl_aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
dim3 fl_grid(int chunks_per_row, int rows, int npics, int nplanes)
{
    const long chunks = (long)chunks_per_row * rows;
    return dim3((unsigned)((chunks + FL_THREADS * FL_TURNS - 1) / (FL_THREADS * FL_TURNS)), (unsigned)npics, (unsigned)nplanes);
}
} // namespace

extern "C" int xeve_hip_frames_load(const uint8_t *frames, int64_t frame_dist, int depth, int src_w, int src_h, int w, int h, uint16_t *const org[3], int s_org_l, int s_org_c,
                                    int64_t org_pic_l, int64_t org_pic_c, int npics, void *stream)
{
    XH_ENTER();
    XH_REQUIRE(frames && org && org[0] && org[1] && org[2] && (depth == 8 || depth == 10) && npics >= 1 && npics <= 65535);
    XH_REQUIRE(src_w >= 2 && src_h >= 2 && (src_w & 1) == 0 && (src_h & 1) == 0 && src_w <= w && src_h <= h);
    XH_REQUIRE(w >= 8 && h >= 8 && (w & 7) == 0 && (h & 7) == 0 && w <= 8192 && h <= 4320);
    const int       sb = depth > 8 ? 2 : 1;
    const long long nl = (long long)src_w * src_h, nc = nl / 4;
    XH_REQUIRE(fl_aligned(frames, sb) && (frame_dist & (sb - 1)) == 0 && (npics == 1 || frame_dist >= (nl + 2 * nc) * sb));
    XH_REQUIRE(s_org_l >= w && s_org_c >= w / 2 && (s_org_l & 7) == 0 && (s_org_c & 3) == 0 && (org_pic_l & 7) == 0 && (org_pic_c & 3) == 0);
    XH_REQUIRE(npics == 1 || (org_pic_l >= (int64_t)s_org_l * (h - 1) + w && org_pic_c >= (int64_t)s_org_c * (h / 2 - 1) + w / 2));
    XH_REQUIRE(fl_aligned(org[0], 16) && fl_aligned(org[1], 8) && fl_aligned(org[2], 8));
    hipStream_t st = static_cast<hipStream_t>(stream);
    FlArgs      A = {};
    A.frames = frames, A.frame_dist = frame_dist;
    A.src_off[0] = 0, A.dst[0] = org[0], A.dst_pic = org_pic_l, A.src_wp = src_w, A.src_hp = src_h, A.wp = w, A.hp = h, A.s_dst = s_org_l;
    if(sb == 2) k_frames_load<2, 0, 8><<<fl_grid(w / 8, h, npics, 1), FL_THREADS, 0, st>>>(A);
    else k_frames_load<1, 2, 8><<<fl_grid(w / 8, h, npics, 1), FL_THREADS, 0, st>>>(A);
    A.src_off[0] = nl * sb, A.src_off[1] = (nl + nc) * sb, A.dst[0] = org[1], A.dst[1] = org[2], A.dst_pic = org_pic_c;
    A.src_wp = src_w / 2, A.src_hp = src_h / 2, A.wp = w / 2, A.hp = h / 2, A.s_dst = s_org_c;
    if(sb == 2) k_frames_load<2, 0, 4><<<fl_grid(w / 8, h / 2, npics, 2), FL_THREADS, 0, st>>>(A);
    else k_frames_load<1, 2, 4><<<fl_grid(w / 8, h / 2, npics, 2), FL_THREADS, 0, st>>>(A);
    XH_HIP(hipGetLastError());
    return XEVE_HIP_OK;
}

extern "C" int xeve_hip_recon_crop(const uint16_t *const rec[3], int s_rec_l, int s_rec_c, int64_t rec_pic_l, int64_t rec_pic_c, int cw, int ch, int npics, uint16_t *out,
                                   int64_t out_pic, void *stream)
{
    XH_ENTER();
    XH_REQUIRE(rec && rec[0] && rec[1] && rec[2] && out && npics >= 1 && npics <= 65535);
    XH_REQUIRE(cw >= 2 && ch >= 2 && (cw & 1) == 0 && (ch & 1) == 0 && cw <= 8192 && ch <= 4320);
    XH_REQUIRE(s_rec_l >= ((cw + 7) & ~7) && s_rec_c >= ((cw / 2 + 3) & ~3) && (s_rec_l & 7) == 0 && (s_rec_c & 3) == 0 && (rec_pic_l & 7) == 0 && (rec_pic_c & 3) == 0);
    XH_REQUIRE(fl_aligned(rec[0], 16) && fl_aligned(rec[1], 8) && fl_aligned(rec[2], 8) && fl_aligned(out, 2));
    XH_REQUIRE(out_pic >= (int64_t)cw * ch * 3 / 2);
    hipStream_t     st = static_cast<hipStream_t>(stream);
    const long long nl = (long long)cw * ch, nc = nl / 4;
    RcArgs          A = {};
    A.rec[0] = rec[0], A.out_off[0] = 0, A.rec_pic = rec_pic_l, A.out_pic = out_pic, A.s_rec = s_rec_l, A.cwp = cw, A.chp = ch;
    k_recon_crop<8><<<fl_grid((cw + 7) / 8, ch, npics, 1), FL_THREADS, 0, st>>>(A, out);
    A.rec[0] = rec[1], A.rec[1] = rec[2], A.out_off[0] = nl, A.out_off[1] = nl + nc, A.rec_pic = rec_pic_c, A.s_rec = s_rec_c, A.cwp = cw / 2, A.chp = ch / 2;
    k_recon_crop<4><<<fl_grid((cw / 2 + 3) / 4, ch / 2, npics, 2), FL_THREADS, 0, st>>>(A, out);
    XH_HIP(hipGetLastError());
    return XEVE_HIP_OK;
}
