// xeve_amd/csrc/ssim.hip -- the structural similarity of the reconstructed picture and the original, per picture and plane, as the exact integer sum include/xeve_hip.h
// defines (ssim_core.h holds the arithmetic; the reference has no counterpart).  A bandwidth kernel beside recon.hip's: every sample of the two inputs is read once, but
// for the halo of a tile.
//
// One launch for the luma planes and one for both chroma planes of all `npics` stacked pictures.  A plane is cut into 4x4 BLOCKS and a window is 2x2 adjacent blocks, so a
// workgroup takes a TILE of SS_TX x SS_TY blocks -- (SS_TX - 1) x (SS_TY - 1) windows and the halo row and column of blocks they share with the tiles right and below
// (1 / 32 + 1 / 16 of the tile read twice, by workgroups next to each other in the grid: the second read comes from L2).  Pass one: a lane loads the 8-byte rows of its
// blocks in both planes -- consecutive lanes take consecutive blocks of a block row, a wave's access is one contiguous run per sample row; luma and chroma rows alike are
// 8-byte aligned at every block -- and leaves each block's record (12 bytes: s1 | s2 << 16, ss, s12) in LDS, one array per word, so neighbouring lanes hit neighbouring
// banks in both passes.  Pass two: a lane forms the window whose top left block is its own from the four records and computes q -- one f64 division per 64 sample pairs
// (a few dozen f64 instructions per window beside the ~100 integer ones of its block's sums).  The workgroup's int64 total goes out in one 64-bit atomic add: integer sums, the
// same whichever workgroup adds first.  Blocks past the plane's last are read CLAMPED (the last block again: no branch around the loads) and their windows left out.
// All addressing is 64-bit; the picture index is blockIdx.y.
#include "ssim_core.h"
#include "xh_common.h"

namespace {
constexpr int SS_THREADS = 256;
constexpr int SS_TX = 32, SS_TY = 16;                     // a tile, in blocks (128 x 64 samples; tests/test_ssim_gpu.py names it)
constexpr int SS_TURNS = SS_TX * SS_TY / SS_THREADS;      // blocks (and windows) per lane
constexpr int SS_ROWS = SS_THREADS / SS_TX;               // block rows per turn
static_assert(SS_TX * SS_TY % SS_THREADS == 0 && SS_THREADS % SS_TX == 0 && SS_TX * SS_ROWS == SS_THREADS, "a turn is whole block rows of the tile");

struct SsPlane {
    const uint16_t *rec, *org;
};
struct SsArgs {
    SsPlane   pl[2]; // blockIdx.z
    int       s_rec, s_org, bx, by, tiles_x;
    long long rec_pic, org_pic;
    int       sum_at; // the first of the launch's planes in sums[pic][3]
};

__device__ __forceinline__ uint64_t ss_row(const uint16_t *p)
{
    const uint2 v = *reinterpret_cast<const uint2 *>(p);
    return (uint64_t)v.x | ((uint64_t)v.y << 32);
}

// grid: (tiles of a plane, pictures, planes of the launch)
__global__ void __launch_bounds__(SS_THREADS) k_ssim(SsArgs A, unsigned long long *__restrict__ sums)
{
    __shared__ uint32_t           l_s[SS_TY][SS_TX], l_ss[SS_TY][SS_TX], l_s12[SS_TY][SS_TX];
    __shared__ unsigned long long wsum[SS_THREADS / XH_WAVE];
    const SsPlane   pl = A.pl[blockIdx.z];
    const long long pic = blockIdx.y;
    const int       ty = blockIdx.x / A.tiles_x, tx = blockIdx.x - ty * A.tiles_x;
    const int       bx0 = tx * (SS_TX - 1), by0 = ty * (SS_TY - 1); // the tile's first block: tiles share their last block row / column with the next tile's first
    const int       lx = threadIdx.x % SS_TX, ly = threadIdx.x / SS_TX;
    const uint16_t *rec = pl.rec + pic * A.rec_pic, *org = pl.org + pic * A.org_pic;
    const int       gx = min(bx0 + lx, A.bx - 1);
#pragma unroll
    for(int t = 0; t < SS_TURNS; t++) {
        const int       y = ly + t * SS_ROWS, gy = min(by0 + y, A.by - 1);
        const uint16_t *r = rec + (long long)(4 * gy) * A.s_rec + 4 * gx, *o = org + (long long)(4 * gy) * A.s_org + 4 * gx;
        uint64_t        a[4], b[4];
#pragma unroll
        for(int k = 0; k < 4; k++) a[k] = ss_row(r + (long long)k * A.s_rec), b[k] = ss_row(o + (long long)k * A.s_org);
        const xssim::Block B = xssim::block_sums(a, b);
        l_s[y][lx] = B.s, l_ss[y][lx] = B.ss, l_s12[y][lx] = B.s12;
    }
    __syncthreads();
    long long part = 0;
#pragma unroll
    for(int t = 0; t < SS_TURNS; t++) {
        const int y = ly + t * SS_ROWS;
        if(lx < SS_TX - 1 && y < SS_TY - 1 && bx0 + lx + 1 < A.bx && by0 + y + 1 < A.by) {
            const xssim::Block tl = {l_s[y][lx], l_ss[y][lx], l_s12[y][lx]}, tr = {l_s[y][lx + 1], l_ss[y][lx + 1], l_s12[y][lx + 1]};
            const xssim::Block bl = {l_s[y + 1][lx], l_ss[y + 1][lx], l_s12[y + 1][lx]}, br = {l_s[y + 1][lx + 1], l_ss[y + 1][lx + 1], l_s12[y + 1][lx + 1]};
            part += xssim::window_q(tl, tr, bl, br);
        }
    }
    // integer sums modulo 2^64 (a negative q as its two's complement): exact whatever the order of the adds.  A lane's partial goes through the wave in 16-bit pieces, whose
    // 64-lane totals fit the 32-bit exchange (DPP, xh_common.h)
    const unsigned long long u = (unsigned long long)part;
    unsigned long long       wave = 0;
#pragma unroll
    for(int k = 0; k < 4; k++) wave += (unsigned long long)(unsigned)xh_group_sum<64>((int)((u >> (16 * k)) & 0xFFFFu)) << (16 * k);
    if((threadIdx.x & (XH_WAVE - 1)) == 0) wsum[threadIdx.x / XH_WAVE] = wave;
    __syncthreads();
    if(threadIdx.x == 0) {
        unsigned long long s = 0;
        for(int k = 0; k < SS_THREADS / XH_WAVE; k++) s += wsum[k];
        if(s) atomicAdd(sums + pic * 3 + A.sum_at + blockIdx.z, s); // one 64-bit add per workgroup
    }
}

bool ss_aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
bool ss_on_device(const void *p)
{
    hipPointerAttribute_t a;
    if(hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeDevice;
}
// the first and the last sample the call reads of a plane whose window is pw x ph
bool ss_plane_on_device(const uint16_t *p, int stride, int64_t pic, int pw, int ph, int npics)
{
    return ss_on_device(p) && ss_on_device(p + (int64_t)(npics - 1) * pic + (int64_t)(ph - 1) * stride + pw - 1);
}
void ss_launch(SsArgs &A, int pw, int ph, int nplanes, int npics, int64_t *sums, hipStream_t st)
{
    A.bx = pw >> 2, A.by = ph >> 2, A.tiles_x = (A.bx - 1 + SS_TX - 2) / (SS_TX - 1);
    const int tiles_y = (A.by - 1 + SS_TY - 2) / (SS_TY - 1);
    k_ssim<<<dim3((unsigned)(A.tiles_x * tiles_y), (unsigned)npics, (unsigned)nplanes), SS_THREADS, 0, st>>>(A, reinterpret_cast<unsigned long long *>(sums));
}
} // namespace

extern "C" int xeve_hip_ssim_planes(const uint16_t *const rec[3], int s_rec_l, int s_rec_c, int64_t rec_pic_l, int64_t rec_pic_c, const uint16_t *const org[3], int s_org_l,
                                    int s_org_c, int64_t org_pic_l, int64_t org_pic_c, int w, int h, int npics, int64_t *sums, void *stream)
{
    XH_ENTER();
    XH_REQUIRE(rec && rec[0] && rec[1] && rec[2] && org && org[0] && org[1] && org[2] && sums);
    XH_REQUIRE(w >= 16 && h >= 16 && (w & 1) == 0 && (h & 1) == 0 && w <= 8192 && h <= 4320 && npics >= 1 && npics <= 65535);
    const int wl = (w + 7) & ~7, wc = (w / 2 + 3) & ~3; // the rows' chunks of 8 (4) samples the window touches
    XH_REQUIRE(s_rec_l >= wl && s_rec_c >= wc && (s_rec_l & 7) == 0 && (s_rec_c & 3) == 0 && (rec_pic_l & 7) == 0 && (rec_pic_c & 3) == 0 && rec_pic_l >= 0 && rec_pic_c >= 0);
    XH_REQUIRE(s_org_l >= wl && s_org_c >= wc && (s_org_l & 7) == 0 && (s_org_c & 3) == 0 && (org_pic_l & 7) == 0 && (org_pic_c & 3) == 0 && org_pic_l >= 0 && org_pic_c >= 0);
    XH_REQUIRE(ss_aligned(rec[0], 16) && ss_aligned(rec[1], 8) && ss_aligned(rec[2], 8) && ss_aligned(org[0], 16) && ss_aligned(org[1], 8) && ss_aligned(org[2], 8) && ss_aligned(sums, 8));
    for(int c = 0; c < 3; c++)
        XH_REQUIRE(ss_plane_on_device(rec[c], c ? s_rec_c : s_rec_l, c ? rec_pic_c : rec_pic_l, c ? w / 2 : w, c ? h / 2 : h, npics) &&
                   ss_plane_on_device(org[c], c ? s_org_c : s_org_l, c ? org_pic_c : org_pic_l, c ? w / 2 : w, c ? h / 2 : h, npics));
    XH_REQUIRE(ss_on_device(sums) && ss_on_device(sums + (size_t)npics * 3 - 1));
    hipStream_t st = static_cast<hipStream_t>(stream);
    XH_HIP(hipMemsetAsync(sums, 0, (size_t)npics * 3 * sizeof(int64_t), st)); // the sums are SET by the call
    SsArgs A = {};
    A.pl[0] = {rec[0], org[0]};
    A.s_rec = s_rec_l, A.s_org = s_org_l, A.rec_pic = rec_pic_l, A.org_pic = org_pic_l, A.sum_at = 0;
    ss_launch(A, w, h, 1, npics, sums, st);
    A.pl[0] = {rec[1], org[1]}, A.pl[1] = {rec[2], org[2]};
    A.s_rec = s_rec_c, A.s_org = s_org_c, A.rec_pic = rec_pic_c, A.org_pic = org_pic_c, A.sum_at = 1;
    ss_launch(A, w / 2, h / 2, 2, npics, sums, st);
    XH_HIP(hipGetLastError());
    return XEVE_HIP_OK;
}
