// xeve_amd/csrc/recon.hip -- what the reference hands out beside the bitstream, taken from the resident pictures: the reconstructed picture's w x h interior packed as
// the application's -r file holds it (planar Y, U, V, 16-bit samples, no padding) and the sum of squared differences against the original per plane (find_psnr_16bit,
// app/xeve_app_util.h:660-681; the PSNR itself is a host division and a logarithm).  A bandwidth kernel: every sample of the two inputs is read once, every sample of the
// output written once.
//
// One launch for the luma planes and one for both chroma planes of all `npics` stacked pictures.  A thread moves CHUNKS of one plane's interior: 8 samples (16 bytes) of a
// luma row, 4 samples (8 bytes) of a chroma row -- w and h are multiples of 8, so a row is a whole number of chunks and, with the strides of the padded stores
// (w + 288 / w / 2 + 144 samples) and of the originals (w / w / 2), every luma chunk lies on a 16-byte and every chroma chunk on an 8-byte boundary (a chroma row of
// 36 samples or a stride of 156 allows no more).  Consecutive lanes take consecutive chunks of a row: a wave's access is one contiguous run per row it touches.
// All addressing is 64-bit (the stacked stores pass 2^32 samples); the picture index is blockIdx.y.
#include "xh_common.h"

namespace {
constexpr int RM_THREADS = 256;
constexpr int RM_TURNS = 8; // chunks per thread: 64 squared differences (each below 2^20 at the codec's 10 bits) in a lane's 32-bit partial, far inside its 4095
static_assert(RM_TURNS * 8 <= 4095, "a lane's 32-bit partial holds at most 4095 squared differences of 10-bit samples");

struct RmPlane {
    const uint16_t *rec, *org;
    long long       out_off; // samples from a picture's first output sample to this plane's
};
struct RmArgs {
    RmPlane   pl[2]; // blockIdx.z
    int       s_rec, s_org, wp, hp;
    long long rec_pic, org_pic, out_pic;
    int       sse_at; // the first of the launch's planes in sse[pic][3]
};

template <class V> struct RmWords;
template <> struct RmWords<uint4> { static constexpr int N = 4; __device__ static unsigned get(const uint4 &v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; } };
template <> struct RmWords<uint2> { static constexpr int N = 2; __device__ static unsigned get(const uint2 &v, int i) { return i == 0 ? v.x : v.y; } };

// V: uint4 (luma) / uint2 (chroma).  grid: (chunks of a plane / (RM_THREADS * RM_TURNS), pictures, planes of the launch)
template <class V, bool COPY, bool MEASURE>
__global__ void __launch_bounds__(RM_THREADS) k_recon_measure(RmArgs A, uint16_t *__restrict__ out, unsigned long long *__restrict__ sse)
{
    constexpr int   SAMPLES = RmWords<V>::N * 2;
    const RmPlane   pl = A.pl[blockIdx.z];
    const long long pic = blockIdx.y;
    const int       cpr = A.wp / SAMPLES, n = cpr * A.hp; // chunks per row / per plane (at most 8192 * 4320 / 8)
    const uint16_t *rec = pl.rec + pic * A.rec_pic;
    const uint16_t *org = MEASURE ? pl.org + pic * A.org_pic : nullptr;
    uint16_t       *dst = COPY ? out + pic * A.out_pic + pl.out_off : nullptr;
    unsigned        part = 0;
    for(int t = 0, i = blockIdx.x * RM_THREADS + threadIdx.x; t < RM_TURNS && i < n; t++, i += gridDim.x * RM_THREADS) {
        const int       row = i / cpr, col = (i - row * cpr) * SAMPLES;
        const V         r = *reinterpret_cast<const V *>(rec + (long long)row * A.s_rec + col);
        if(COPY) *reinterpret_cast<V *>(dst + (long long)row * A.wp + col) = r;
        if(MEASURE) {
            const V o = *reinterpret_cast<const V *>(org + (long long)row * A.s_org + col);
#pragma unroll
            for(int k = 0; k < RmWords<V>::N; k++) {
                const unsigned a = RmWords<V>::get(r, k), b = RmWords<V>::get(o, k);
                const int      d0 = (int)(a & 0xFFFFu) - (int)(b & 0xFFFFu), d1 = (int)(a >> 16) - (int)(b >> 16);
                part += (unsigned)(d0 * d0) + (unsigned)(d1 * d1);
            }
        }
    }
    if(MEASURE) {
        // integer sums: exact whatever the order of the adds.  The wave's total of 64 partials needs more than 32 bits, so the halves are summed apart (DPP, xh_common.h)
        const unsigned long long wave = (unsigned long long)(unsigned)xh_group_sum<64>((int)(part & 0xFFFFu)) +
                                        ((unsigned long long)(unsigned)xh_group_sum<64>((int)(part >> 16)) << 16);
        __shared__ unsigned long long wsum[RM_THREADS / XH_WAVE];
        if((threadIdx.x & (XH_WAVE - 1)) == 0) wsum[threadIdx.x / XH_WAVE] = wave;
        __syncthreads();
        if(threadIdx.x == 0) {
            unsigned long long s = 0;
            for(int k = 0; k < RM_THREADS / XH_WAVE; k++) s += wsum[k];
            if(s) atomicAdd(sse + pic * 3 + A.sse_at + blockIdx.z, s); // one 64-bit add per workgroup
        }
    }
}

template <class V> void rm_launch(const RmArgs &A, int nplanes, int npics, uint16_t *out, uint64_t *sse, hipStream_t st)
{
    const long chunks = (long)(A.wp / (int)(sizeof(V) / 2)) * A.hp;
    const dim3 grid((unsigned)((chunks + RM_THREADS * RM_TURNS - 1) / (RM_THREADS * RM_TURNS)), (unsigned)npics, (unsigned)nplanes);
    unsigned long long *s = reinterpret_cast<unsigned long long *>(sse);
    if(out && sse) k_recon_measure<V, true, true><<<grid, RM_THREADS, 0, st>>>(A, out, s);
    else if(out) k_recon_measure<V, true, false><<<grid, RM_THREADS, 0, st>>>(A, out, s);
    else k_recon_measure<V, false, true><<<grid, RM_THREADS, 0, st>>>(A, out, s);
}
bool rm_aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
} // namespace

extern "C" int xeve_hip_recon_measure(const uint16_t *const rec[3], int s_rec_l, int s_rec_c, int64_t rec_pic_l, int64_t rec_pic_c, const uint16_t *const org[3], int s_org_l,
                                      int s_org_c, int64_t org_pic_l, int64_t org_pic_c, int w, int h, int npics, uint16_t *out, int64_t out_pic, uint64_t *sse, void *stream)
{
    XH_ENTER();
    XH_REQUIRE(rec && rec[0] && rec[1] && rec[2] && (out || sse));
    XH_REQUIRE(w >= 8 && h >= 8 && (w & 7) == 0 && (h & 7) == 0 && w <= 8192 && h <= 4320 && npics >= 1 && npics <= 65535);
    XH_REQUIRE(s_rec_l >= w && s_rec_c >= w / 2 && (s_rec_l & 7) == 0 && (s_rec_c & 3) == 0 && (rec_pic_l & 7) == 0 && (rec_pic_c & 3) == 0);
    XH_REQUIRE(rm_aligned(rec[0], 16) && rm_aligned(rec[1], 8) && rm_aligned(rec[2], 8));
    if(sse) {
        XH_REQUIRE(org && org[0] && org[1] && org[2] && s_org_l >= w && s_org_c >= w / 2 && (s_org_l & 7) == 0 && (s_org_c & 3) == 0 && (org_pic_l & 7) == 0 && (org_pic_c & 3) == 0);
        XH_REQUIRE(rm_aligned(org[0], 16) && rm_aligned(org[1], 8) && rm_aligned(org[2], 8) && rm_aligned(sse, 8));
    }
    if(out) XH_REQUIRE(rm_aligned(out, 16) && (out_pic & 7) == 0 && out_pic >= (int64_t)w * h * 3 / 2);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if(sse) XH_HIP(hipMemsetAsync(sse, 0, (size_t)npics * 3 * sizeof(uint64_t), st)); // the sums are SET by the call
    RmArgs A = {};
    A.pl[0] = {rec[0], sse ? org[0] : nullptr, 0};
    A.s_rec = s_rec_l, A.s_org = s_org_l, A.wp = w, A.hp = h, A.rec_pic = rec_pic_l, A.org_pic = org_pic_l, A.out_pic = out_pic, A.sse_at = 0;
    rm_launch<uint4>(A, 1, npics, out, sse, st);
    const long long nl = (long long)w * h, nc = nl / 4;
    A.pl[0] = {rec[1], sse ? org[1] : nullptr, nl}, A.pl[1] = {rec[2], sse ? org[2] : nullptr, nl + nc};
    A.s_rec = s_rec_c, A.s_org = s_org_c, A.wp = w / 2, A.hp = h / 2, A.rec_pic = rec_pic_c, A.org_pic = org_pic_c, A.sse_at = 1;
    rm_launch<uint2>(A, 2, npics, out, sse, st);
    XH_HIP(hipGetLastError());
    return XEVE_HIP_OK;
}
