// xeve_amd/csrc/host_cu.cpp -- host-memory forms of the CU and CTU analyses: ctx->fn_pintra_analyze_cu, ctx->fn_pinter_analyze_cu, ctx->fn_mode_analyze_lcu
// (tests/test_integration_ref.py binds them through shim/xeve_hip_shim.c).  Host code on the C-ABI's batched entry points (intra.hip, inter.hip,
// tree.hip); which form owns a stream, pinned memory or an arena is host_stage.h's table.
#include <cstdlib>
#include <vector>
#include "host_stage.h"

// ---- host-memory form of ONE call of ctx->fn_pintra_analyze_cu (the table layer's style: stage, launch, synchronise) ---------------------------------------------
// Every pointer is HOST memory: org / mod = sample (0, 0) of the original picture's planes and of the picture being reconstructed (pi->o, pi->m), the maps =
// ctx->map_scu / map_ipm / map_tidx.  Only what the analysis reads is moved: the CU's block of the original, the line above and the column left of the CU in the
// mode picture (cuw + cuh samples each, clipped to the picture), the map entries of the 4x4 units those samples lie in.  They are laid out as a small local
// picture (the CU at unit (1, 1), or on the edge where the real CU is on the picture's edge) so that the batched entry point runs unchanged on it.
extern "C" int xeve_hip_pintra_analyze_cu_host(const xeve_hip_pel *const org[3], int s_org_l, int s_org_c, const xeve_hip_pel *const mod[3], int s_mod_l, int s_mod_c,
                                               const uint32_t *map_scu, const int8_t *map_ipm, const uint8_t *map_tidx, const xeve_hip_sbac *state,
                                               const xeve_hip_intra_params *p, const xeve_hip_intra_job *job, xeve_hip_intra_result *result, int16_t *coef_y,
                                               int16_t *coef_u, int16_t *coef_v, xeve_hip_pel *rec_y, xeve_hip_pel *rec_u, xeve_hip_pel *rec_v, xeve_hip_sbac *best)
{
    XH_ENTER();
    XH_REQUIRE(org && mod && map_scu && map_ipm && map_tidx && state && job && result && coef_y && rec_y && best && intra_params_ok(p));
    const int idc = p->chroma_format_idc, ws = idc <= 2, hs = idc <= 1, ncomp = idc ? 3 : 1, lw = p->log2_cuw;
    XH_REQUIRE(org[0] && mod[0] && (!idc || (org[1] && org[2] && mod[1] && mod[2] && coef_u && coef_v && rec_u && rec_v)));
    const int cu = 1 << lw, n = cu >> 2, x_scu = job->x >> 2, y_scu = job->y >> 2, scup = y_scu * p->w_scu + x_scu;
    XH_REQUIRE(job->x >= 0 && job->y >= 0 && (job->x & 3) == 0 && (job->y & 3) == 0 && x_scu + n <= p->w_scu && y_scu + n <= p->h_scu);
    const XhWindow V(job->x, job->y, 2 * n, 2 * n, n, p->w_scu, p->h_scu);
    const int      lx = V.lx, ly = V.ly, nw = V.nw, nh = V.nh, Wl = V.Wl, Hl = V.Hl;
    const size_t n0 = (size_t)cu * cu, n1 = idc ? n0 >> (ws + hs) : 0, nmap = (size_t)Wl * Hl;
    // staging layout (identical in the pinned buffer and in the device arena)
    const int    pw[3] = {Wl * 4, Wl * (4 >> ws), Wl * (4 >> ws)}, ph[3] = {Hl * 4, Hl * (4 >> hs), Hl * (4 >> hs)};
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 63) & ~(size_t)63; return at; };
    const size_t o_job = take(sizeof(*job)), o_st = take(sizeof(*state)), o_scu = take(nmap * 4), o_ipm = take(nmap), o_tidx = take(nmap);
    size_t o_org[3] = {0, 0, 0}, o_mod[3] = {0, 0, 0};
    for(int c = 0; c < ncomp; c++) o_org[c] = take((size_t)pw[c] * ph[c] * 2), o_mod[c] = take((size_t)pw[c] * ph[c] * 2);
    const size_t in_bytes = o;
    const size_t o_res = take(sizeof(*result)), o_best = take(sizeof(*best)), o_coef = take((n0 + 2 * n1) * 2), o_rec = take((n0 + 2 * n1) * 2);
    const size_t io_bytes = o;
    xeve_hip_intra_params pl = *p;
    pl.w_scu = Wl, pl.h_scu = Hl;
    const size_t wsb = xeve_hip_pintra_analyze_cu_workspace(1, 1, &pl);
    static thread_local XhHostArena C;
    int rc = C.ensure(io_bytes, wsb);
    if(rc != XEVE_HIP_OK) return rc;
    char *H = C.pin, *D = C.dev;
    // the job in local coordinates, the entry state, the maps
    xeve_hip_intra_job jl = *job;
    jl.x = 4 * lx, jl.y = 4 * ly, jl.sbac = 0, jl.pic = 0;
    memcpy(H + o_job, &jl, sizeof(jl)), memcpy(H + o_st, state, sizeof(*state));
    memset(H + o_scu, 0, o_org[0] - o_scu);
    auto *ls = (uint32_t *)(H + o_scu);
    auto *li = (int8_t *)(H + o_ipm);
    auto *lt = (uint8_t *)(H + o_tidx);
    auto unit = [&](int lu, int gu) { ls[lu] = map_scu[gu], li[lu] = map_ipm[gu], lt[lu] = map_tidx[gu]; };
    unit(ly * Wl + lx, scup);
    if(ly) for(int i = -lx; i < nw; i++) unit((ly - 1) * Wl + lx + i, scup - p->w_scu + i);
    if(lx) for(int i = 0; i < nh; i++) unit((ly + i) * Wl + lx - 1, scup - 1 + i * p->w_scu);
    // the planes: the original's block; the line above and the column to the left of the mode picture
    for(int c = 0; c < ncomp; c++) {
        const int sx = c ? ws : 0, sy = c ? hs : 0, uw = 4 >> sx, uh = 4 >> sy, bw = cu >> sx, bh = cu >> sy;
        const int so = c ? s_org_c : s_org_l, sm = c ? s_mod_c : s_mod_l, x = job->x >> sx, y = job->y >> sy, xl = lx * uw, yl = ly * uh;
        pel *lo = (pel *)(H + o_org[c]), *lm = (pel *)(H + o_mod[c]);
        memset(lo, 0, (size_t)pw[c] * ph[c] * 2), memset(lm, 0, (size_t)pw[c] * ph[c] * 2);
        for(int r = 0; r < bh; r++) memcpy(lo + (size_t)(yl + r) * pw[c] + xl, org[c] + (size_t)(y + r) * so + x, sizeof(pel) * bw);
        if(ly) memcpy(lm + (size_t)(yl - 1) * pw[c], mod[c] + (size_t)(y - 1) * sm + (x - xl), sizeof(pel) * (size_t)(xl + nw * uw));
        if(lx) for(int r = 0; r < nh * uh; r++) lm[(size_t)(yl + r) * pw[c] + xl - 1] = mod[c][(size_t)(y + r) * sm + x - 1];
    }
    XH_HIP(hipMemcpyAsync(D, H, in_bytes, hipMemcpyHostToDevice, C.st));
    const pel *d_org[3] = {(const pel *)(D + o_org[0]), idc ? (const pel *)(D + o_org[1]) : nullptr, idc ? (const pel *)(D + o_org[2]) : nullptr};
    const pel *d_mod[3] = {(const pel *)(D + o_mod[0]), idc ? (const pel *)(D + o_mod[1]) : nullptr, idc ? (const pel *)(D + o_mod[2]) : nullptr};
    char *d_ws = D + ((io_bytes + 255) & ~(size_t)255);
    rc = xeve_hip_pintra_analyze_cu_jobs(d_org, pw[0], pw[1], d_mod, pw[0], pw[1], (const uint32_t *)(D + o_scu), (const int8_t *)(D + o_ipm), (const uint8_t *)(D + o_tidx),
                                         nullptr, (const xeve_hip_sbac *)(D + o_st), 1, &pl, (const xeve_hip_intra_job *)(D + o_job), 1,
                                         (xeve_hip_intra_result *)(D + o_res), (int16_t *)(D + o_coef), (pel *)(D + o_rec), (xeve_hip_sbac *)(D + o_best), d_ws,
                                         C.dev_bytes - (size_t)(d_ws - D), C.st);
    if(rc != XEVE_HIP_OK) return rc;
    XH_HIP(hipMemcpyAsync(H + o_res, D + o_res, io_bytes - o_res, hipMemcpyDeviceToHost, C.st));
    XH_HIP(hipStreamSynchronize(C.st));
    memcpy(result, H + o_res, sizeof(*result)), memcpy(best, H + o_best, sizeof(*best));
    const int16_t *hc = (const int16_t *)(H + o_coef);
    const pel     *hr = (const pel *)(H + o_rec);
    memcpy(coef_y, hc, n0 * 2), memcpy(rec_y, hr, n0 * 2);
    if(idc) {
        memcpy(coef_u, hc + n0, n1 * 2), memcpy(coef_v, hc + n0 + n1, n1 * 2);
        memcpy(rec_u, hr + n0, n1 * 2), memcpy(rec_v, hr + n0 + n1, n1 * 2);
    }
    return XEVE_HIP_OK;
}

// ---- host-memory form of ONE call of ctx->fn_mode_analyze_lcu in an I slice (stage, launch, synchronise: one exchange per CTU) --------------------------------
// Every pointer is HOST memory: org / mod = sample (0, 0) of the original picture's planes and of the picture being reconstructed, the maps = ctx->map_scu / map_ipm /
// map_tidx / map_cu_mode.  What the walk reads is moved as a small LOCAL PICTURE: the CTU, one unit to its left and above (none on the picture's edge), and the
// CTU's width again to the right (the samples up-right of its CUs); the picture's own right / bottom edge stays an edge, so a CTU the picture cuts is cut the
// same way.  The CTU's part of the reconstruction and of the maps is written back.
extern "C" int xeve_hip_mode_analyze_ctu_intra_host(const xeve_hip_pel *const org[3], int s_org_l, int s_org_c, xeve_hip_pel *const mod[3], int s_mod_l, int s_mod_c,
                                                    uint32_t *map_scu, int8_t *map_ipm, const uint8_t *map_tidx, uint32_t *map_cu_mode, const xeve_hip_sbac *entry,
                                                    const xeve_hip_tree_params *p, int x0, int y0, xeve_hip_ctu_data *out, xeve_hip_sbac *next_best, double *cost)
{
    XH_ENTER();
    XH_REQUIRE(org && mod && map_scu && map_ipm && map_tidx && map_cu_mode && entry && out && next_best && cost && tree_params_ok(p));
    const int idc = p->ip.chroma_format_idc, ws = idc <= 2, hs = idc <= 1, ncomp = idc ? 3 : 1, ctu = 1 << p->log2_ctu, n = ctu >> 2;
    XH_REQUIRE(org[0] && mod[0] && (!idc || (org[1] && org[2] && mod[1] && mod[2])));
    XH_REQUIRE(x0 >= 0 && y0 >= 0 && x0 < p->pic_w && y0 < p->pic_h && (x0 & (ctu - 1)) == 0 && (y0 & (ctu - 1)) == 0);
    const XhWindow V(x0, y0, 2 * n, n, n, p->ip.w_scu, p->ip.h_scu); // cw x nh units: the CTU's part inside the picture
    const int      x_scu = V.x_scu, y_scu = V.y_scu, lx = V.lx, ly = V.ly, nh = V.nh, Wl = V.Wl, Hl = V.Hl, cw = V.cw;
    const size_t nmap = (size_t)Wl * Hl;
    const int    pw[3] = {Wl * 4, Wl * (4 >> ws), Wl * (4 >> ws)}, ph[3] = {Hl * 4, Hl * (4 >> hs), Hl * (4 >> hs)};
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 63) & ~(size_t)63; return at; };
    xeve_hip_ctu_job jl;
    jl.x = 4 * lx, jl.y = 4 * ly, jl.sbac = 0, jl.pic = 0;
    const size_t o_job = take(sizeof(jl)), o_st = take(sizeof(*entry)), o_tidx = take(nmap);
    size_t o_org[3] = {0, 0, 0};
    for(int c = 0; c < ncomp; c++) o_org[c] = take((size_t)pw[c] * ph[c] * 2);
    const size_t o_scu = take(nmap * 4), o_ipm = take(nmap), o_cum = take(nmap * 4); // from here on the buffers come back too
    size_t o_mod[3] = {0, 0, 0};
    for(int c = 0; c < ncomp; c++) o_mod[c] = take((size_t)pw[c] * ph[c] * 2);
    const size_t in_bytes = o;
    const size_t o_out = take(sizeof(*out)), o_next = take(sizeof(*next_best)), o_cost = take(sizeof(double));
    const size_t io_bytes = o;
    xeve_hip_tree_params pl = *p;
    pl.ip.w_scu = Wl, pl.ip.h_scu = Hl, pl.pic_w = Wl * 4, pl.pic_h = Hl * 4;
    const size_t wsb = xeve_hip_mode_analyze_ctu_intra_workspace(1, &pl);
    XH_REQUIRE(wsb > 0);
    static thread_local XhHostArena C;
    int rc = C.ensure(io_bytes, wsb);
    if(rc != XEVE_HIP_OK) return rc;
    char *H = C.pin, *D = C.dev;
    memcpy(H + o_job, &jl, sizeof(jl)), memcpy(H + o_st, entry, sizeof(*entry));
    const int gu0 = (y_scu - ly) * p->ip.w_scu + x_scu - lx; // the window's first unit in the picture's maps
    for(int j = 0; j < Hl; j++) {
        const size_t g = (size_t)gu0 + (size_t)j * p->ip.w_scu, l = (size_t)j * Wl;
        memcpy(H + o_scu + 4 * l, map_scu + g, 4 * (size_t)Wl), memcpy(H + o_cum + 4 * l, map_cu_mode + g, 4 * (size_t)Wl);
        memcpy(H + o_ipm + l, map_ipm + g, Wl), memcpy(H + o_tidx + l, map_tidx + g, Wl);
    }
    for(int c = 0; c < ncomp; c++) {
        const int sx = c ? ws : 0, sy = c ? hs : 0, so = c ? s_org_c : s_org_l, sm = c ? s_mod_c : s_mod_l;
        const int xw = (x0 >> sx) - lx * (4 >> sx), yw = (y0 >> sy) - ly * (4 >> sy); // the window's first sample in the plane
        pel *lo = (pel *)(H + o_org[c]), *lm = (pel *)(H + o_mod[c]);
        for(int r = 0; r < ph[c]; r++) {
            memcpy(lo + (size_t)r * pw[c], org[c] + (size_t)(yw + r) * so + xw, sizeof(pel) * pw[c]);
            memcpy(lm + (size_t)r * pw[c], mod[c] + (size_t)(yw + r) * sm + xw, sizeof(pel) * pw[c]);
        }
    }
    XH_HIP(hipMemcpyAsync(D, H, in_bytes, hipMemcpyHostToDevice, C.st));
    const pel *d_org[3] = {(const pel *)(D + o_org[0]), idc ? (const pel *)(D + o_org[1]) : nullptr, idc ? (const pel *)(D + o_org[2]) : nullptr};
    pel       *d_mod[3] = {(pel *)(D + o_mod[0]), idc ? (pel *)(D + o_mod[1]) : nullptr, idc ? (pel *)(D + o_mod[2]) : nullptr};
    char *d_ws = D + ((io_bytes + 255) & ~(size_t)255);
    rc = xeve_hip_mode_analyze_ctu_intra_jobs(d_org, pw[0], pw[1], d_mod, pw[0], pw[1], (uint32_t *)(D + o_scu), (int8_t *)(D + o_ipm), (const uint8_t *)(D + o_tidx),
                                              (uint32_t *)(D + o_cum), nullptr, (const xeve_hip_sbac *)(D + o_st), 1, &pl, (const xeve_hip_ctu_job *)(D + o_job), 1,
                                              (xeve_hip_ctu_data *)(D + o_out), (xeve_hip_sbac *)(D + o_next), (double *)(D + o_cost), d_ws,
                                              C.dev_bytes - (size_t)(d_ws - D), C.st);
    if(rc != XEVE_HIP_OK) return rc;
    XH_HIP(hipMemcpyAsync(H + o_scu, D + o_scu, io_bytes - o_scu, hipMemcpyDeviceToHost, C.st));
    XH_HIP(hipStreamSynchronize(C.st));
    memcpy(out, H + o_out, sizeof(*out)), memcpy(next_best, H + o_next, sizeof(*next_best)), memcpy(cost, H + o_cost, sizeof(double));
    for(int j = 0; j < nh; j++) { // the CTU's units
        const size_t g = (size_t)(y_scu + j) * p->ip.w_scu + x_scu, l = (size_t)(ly + j) * Wl + lx;
        memcpy(map_scu + g, H + o_scu + 4 * l, 4 * (size_t)cw), memcpy(map_cu_mode + g, H + o_cum + 4 * l, 4 * (size_t)cw), memcpy(map_ipm + g, H + o_ipm + l, cw);
    }
    for(int c = 0; c < ncomp; c++) { // the CTU's samples
        const int sx = c ? ws : 0, sy = c ? hs : 0, sm = c ? s_mod_c : s_mod_l, bw = (cw * 4) >> sx, bh = (nh * 4) >> sy, xl = lx * (4 >> sx), yl = ly * (4 >> sy);
        const pel *lm = (const pel *)(H + o_mod[c]);
        for(int r = 0; r < bh; r++) memcpy(mod[c] + (size_t)((y0 >> sy) + r) * sm + (x0 >> sx), lm + (size_t)(yl + r) * pw[c] + xl, sizeof(pel) * bw);
    }
    return XEVE_HIP_OK;
}

// ---- host-memory form for every slice type (P / B: needs resident pictures, xeve_hip_picture_begin) -------------------------------------------------------------
// The inter analysis addresses the reference pictures with the CU's position in the picture, so a P / B CTU is walked in PICTURE coordinates: the original, the
// reference pictures, the collocated motion maps and the tile map are resident copies (one upload per picture); the picture being reconstructed and the maps the
// walk updates live in per-thread device buffers of picture size, of which only the CTU's neighbourhood is current -- it is uploaded before the walk (the CTU, one
// unit to its left and above, the CTU's width again to the right) and the CTU's own part is read back after it.
namespace {
struct TreePicCtx {
    uint32_t    gen = 0;
    hipStream_t st  = nullptr;
    char       *buf[12] = {};
    size_t      cap[12] = {};
    void release()
    {
        if(st) (void)hipStreamDestroy(st);
        for(int i = 0; i < 12; i++) {
            if(buf[i]) (void)hipFree(buf[i]);
            buf[i] = nullptr, cap[i] = 0;
        }
        st = nullptr;
    }
    int ensure(int i, size_t bytes)
    {
        if(cap[i] >= bytes) return XEVE_HIP_OK;
        if(buf[i]) {
            XH_HIP(hipStreamSynchronize(st));
            (void)hipFree(buf[i]);
            buf[i] = nullptr, cap[i] = 0;
        }
        XH_HIP(hipMalloc((void **)&buf[i], bytes + (bytes >> 3)));
        XH_HIP(hipMemsetAsync(buf[i], 0, bytes + (bytes >> 3), st));
        cap[i] = bytes + (bytes >> 3);
        return XEVE_HIP_OK;
    }
    int begin()
    {
        if(gen != xh_generation()) release(), gen = xh_generation();
        if(!st) XH_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        return XEVE_HIP_OK;
    }
    ~TreePicCtx() { release(); }
};
enum { B_MOD0 = 0, B_MOD1 = 1, B_MOD2 = 2, B_SCU = 3, B_IPM = 4, B_CUM = 5, B_MV = 6, B_REFI = 7, B_IO = 8, B_WS = 9 };
} // namespace

extern "C" int xeve_hip_mode_analyze_ctu_host(const xeve_hip_pel *const org[3], int s_org_l, int s_org_c, xeve_hip_pel *const mod[3], int s_mod_l, int s_mod_c,
                                              uint32_t *map_scu, int8_t *map_ipm, const uint8_t *map_tidx, uint32_t *map_cu_mode, const xeve_hip_sbac *entry,
                                              const xeve_hip_tree_params *p, const xeve_hip_tree_inter *I, int pad_l, int pad_c, int x0, int y0,
                                              xeve_hip_ctu_data *out, xeve_hip_sbac *next_best, double *cost)
{
    XH_ENTER();
    XH_REQUIRE(p);
    if(p->ip.slice_type == 2)
        return xeve_hip_mode_analyze_ctu_intra_host(org, s_org_l, s_org_c, mod, s_mod_l, s_mod_c, map_scu, map_ipm, map_tidx, map_cu_mode, entry, p, x0, y0, out, next_best, cost);
    XH_REQUIRE(org && mod && map_scu && map_ipm && map_tidx && map_cu_mode && entry && out && next_best && cost && tree_params_ok(p) && tree_inter_ok(p, I) && pad_l >= 0 && pad_c >= 0);
    if(!xh_resident_on()) {
        xh_set_error("xeve_hip_mode_analyze_ctu_host: a P / B CTU needs resident pictures (announce each picture with xeve_hip_picture_begin)");
        return XEVE_HIP_ERR_ARG;
    }
    const int idc = p->ip.chroma_format_idc, ws = idc <= 2, hs = idc <= 1, ncomp = idc ? 3 : 1, ctu = 1 << p->log2_ctu, n = ctu >> 2, isb = p->ip.slice_type == 0;
    XH_REQUIRE(org[0] && mod[0] && (!idc || (org[1] && org[2] && mod[1] && mod[2])));
    XH_REQUIRE(x0 >= 0 && y0 >= 0 && x0 < p->pic_w && y0 < p->pic_h && (x0 & (ctu - 1)) == 0 && (y0 & (ctu - 1)) == 0);
    const int w_scu = p->ip.w_scu, h_scu = p->ip.h_scu, nscu = w_scu * h_scu, hc = p->pic_h >> hs;
    const XhWindow V(x0, y0, 2 * n, n, n, w_scu, h_scu);
    const int      x_scu = V.x_scu, y_scu = V.y_scu, lx = V.lx, ly = V.ly, nh = V.nh, Wl = V.Wl, Hl = V.Hl, cw = V.cw;
    static thread_local TreePicCtx C;
    int rc = C.begin();
    if(rc != XEVE_HIP_OK) return rc;
    // resident: the original, the reference pictures of both lists, the collocated maps, the tile map
    const XhPlaneExtents E(s_org_l, s_org_c, I->s_ref_l, I->s_ref_c, pad_l, pad_c, p->pic_h, hs);
    const pel *dorg[3] = {nullptr, nullptr, nullptr};
    for(int c = 0; c < ncomp; c++)
        if(!(dorg[c] = (const pel *)xh_resident(org[c], E.org[c] * sizeof(pel)))) return XEVE_HIP_ERR_DEVICE;
    xeve_hip_refpic tab[2 * XEVE_HIP_MAX_REFP];
    const int nr[2] = {I->ipar.rdo.num_refp[0], isb ? I->ipar.rdo.num_refp[1] : 0};
    XH_REQUIRE(nr[0] >= 1 && nr[0] <= XEVE_HIP_MAX_REFP && nr[1] <= XEVE_HIP_MAX_REFP);
    if((rc = xh_resident_reftab(tab, I->refp, nr[0], nr[1], ncomp, E)) != XEVE_HIP_OK) return rc;
    const int16_t *dcol0 = (const int16_t *)xh_resident(I->col_mv0, (size_t)nscu * 8), *dcol1 = isb ? (const int16_t *)xh_resident(I->col_mv1, (size_t)nscu * 8) : dcol0;
    const uint8_t *dtidx = (const uint8_t *)xh_resident(map_tidx, (size_t)nscu);
    if(!dcol0 || !dcol1 || !dtidx) return XEVE_HIP_ERR_DEVICE;
    // per-thread picture-sized buffers + the call's small records + the workspace
    xeve_hip_tree_inter Id = *I;
    const size_t wsb = xeve_hip_mode_analyze_ctu_workspace(1, p, I, s_org_l, s_org_c);
    XH_REQUIRE(wsb > 0);
    const size_t o_job = 0, o_st = 256, o_out = 512, o_next = o_out + xh_al(sizeof(*out)), o_cost = o_next + 256, io_bytes = o_cost + 256;
    const size_t need[10] = {(size_t)s_mod_l * p->pic_h * 2, (size_t)s_mod_c * hc * 2, (size_t)s_mod_c * hc * 2, (size_t)nscu * 4, (size_t)nscu, (size_t)nscu * 4, (size_t)nscu * 8,
                             (size_t)nscu * 2, io_bytes, wsb};
    for(int i = 0; i < 10; i++)
        if((i == B_MOD1 || i == B_MOD2) && !idc) continue;
        else if((rc = C.ensure(i, need[i])) != XEVE_HIP_OK) return rc;
    pel *dmod[3] = {(pel *)C.buf[B_MOD0], (pel *)C.buf[B_MOD1], (pel *)C.buf[B_MOD2]};
    Id.refp = tab, Id.map_mv = (int16_t *)C.buf[B_MV], Id.map_refi = (int8_t *)C.buf[B_REFI], Id.col_mv0 = dcol0, Id.col_mv1 = dcol1;
    // the neighbourhood in: rows [y_scu - ly, y_scu + nh) x columns [x_scu - lx, x_scu + nw) of every map, the same window of the planes
    const size_t u0 = (size_t)(y_scu - ly) * w_scu + (x_scu - lx);
    auto copy2d = [&](void *dst, const void *src, size_t pitch, size_t width, size_t height, hipMemcpyKind kind) {
        return width && height ? hipMemcpy2DAsync(dst, pitch, src, pitch, width, height, kind, C.st) : hipSuccess;
    };
    XH_HIP(copy2d(C.buf[B_SCU] + u0 * 4, map_scu + u0, (size_t)w_scu * 4, (size_t)Wl * 4, Hl, hipMemcpyHostToDevice));
    if(y_scu + nh < h_scu) { // the units BELOW the CTU and its left margin: the left neighbours of a CU reach as far below it as it is high, i.e. out of the CTU's bottom row
                             // into units that are not coded yet -- their flags must say so here too (the buffers keep what earlier pictures left)
        const size_t b0 = (size_t)(y_scu + nh) * w_scu + (x_scu - lx);
        XH_HIP(copy2d(C.buf[B_SCU] + b0 * 4, map_scu + b0, (size_t)w_scu * 4, (size_t)(lx + cw) * 4, std::min(n, h_scu - (y_scu + nh)), hipMemcpyHostToDevice));
    }
    XH_HIP(copy2d(C.buf[B_CUM] + u0 * 4, map_cu_mode + u0, (size_t)w_scu * 4, (size_t)Wl * 4, Hl, hipMemcpyHostToDevice));
    XH_HIP(copy2d(C.buf[B_IPM] + u0, map_ipm + u0, (size_t)w_scu, (size_t)Wl, Hl, hipMemcpyHostToDevice));
    XH_HIP(copy2d(C.buf[B_MV] + u0 * 8, I->map_mv + u0 * 4, (size_t)w_scu * 8, (size_t)Wl * 8, Hl, hipMemcpyHostToDevice));
    XH_HIP(copy2d(C.buf[B_REFI] + u0 * 2, I->map_refi + u0 * 2, (size_t)w_scu * 2, (size_t)Wl * 2, Hl, hipMemcpyHostToDevice));
    for(int c = 0; c < ncomp; c++) {
        const int    sx = c ? ws : 0, sy = c ? hs : 0, sm = c ? s_mod_c : s_mod_l;
        const size_t s0 = (size_t)((y0 >> sy) - ly * (4 >> sy)) * sm + ((x0 >> sx) - lx * (4 >> sx));
        XH_HIP(copy2d(dmod[c] + s0, mod[c] + s0, (size_t)sm * 2, (size_t)(Wl * (4 >> sx)) * 2, (size_t)Hl * (4 >> sy), hipMemcpyHostToDevice));
    }
    xeve_hip_ctu_job jl;
    jl.x = x0, jl.y = y0, jl.sbac = 0, jl.pic = 0;
    XH_HIP(hipMemcpyAsync(C.buf[B_IO] + o_job, &jl, sizeof(jl), hipMemcpyHostToDevice, C.st));
    XH_HIP(hipMemcpyAsync(C.buf[B_IO] + o_st, entry, sizeof(*entry), hipMemcpyHostToDevice, C.st));
    rc = xeve_hip_mode_analyze_ctu_jobs(dorg, s_org_l, s_org_c, dmod, s_mod_l, s_mod_c, (uint32_t *)C.buf[B_SCU], (int8_t *)C.buf[B_IPM], dtidx, (uint32_t *)C.buf[B_CUM], nullptr,
                                        (const xeve_hip_sbac *)(C.buf[B_IO] + o_st), 1, p, &Id, (const xeve_hip_ctu_job *)(C.buf[B_IO] + o_job), 1,
                                        (xeve_hip_ctu_data *)(C.buf[B_IO] + o_out), (xeve_hip_sbac *)(C.buf[B_IO] + o_next), (double *)(C.buf[B_IO] + o_cost), C.buf[B_WS],
                                        C.cap[B_WS], C.st);
    if(rc != XEVE_HIP_OK) return rc;
    // the CTU's part out
    const size_t c0 = (size_t)y_scu * w_scu + x_scu;
    XH_HIP(hipMemcpyAsync(out, C.buf[B_IO] + o_out, sizeof(*out), hipMemcpyDeviceToHost, C.st));
    XH_HIP(hipMemcpyAsync(next_best, C.buf[B_IO] + o_next, sizeof(*next_best), hipMemcpyDeviceToHost, C.st));
    XH_HIP(hipMemcpyAsync(cost, C.buf[B_IO] + o_cost, sizeof(double), hipMemcpyDeviceToHost, C.st));
    XH_HIP(copy2d(map_scu + c0, C.buf[B_SCU] + c0 * 4, (size_t)w_scu * 4, (size_t)cw * 4, nh, hipMemcpyDeviceToHost));
    XH_HIP(copy2d(map_cu_mode + c0, C.buf[B_CUM] + c0 * 4, (size_t)w_scu * 4, (size_t)cw * 4, nh, hipMemcpyDeviceToHost));
    XH_HIP(copy2d(map_ipm + c0, C.buf[B_IPM] + c0, (size_t)w_scu, (size_t)cw, nh, hipMemcpyDeviceToHost));
    XH_HIP(copy2d(I->map_mv + c0 * 4, C.buf[B_MV] + c0 * 8, (size_t)w_scu * 8, (size_t)cw * 8, nh, hipMemcpyDeviceToHost));
    XH_HIP(copy2d(I->map_refi + c0 * 2, C.buf[B_REFI] + c0 * 2, (size_t)w_scu * 2, (size_t)cw * 2, nh, hipMemcpyDeviceToHost));
    for(int c = 0; c < ncomp; c++) {
        const int    sx = c ? ws : 0, sy = c ? hs : 0, sm = c ? s_mod_c : s_mod_l;
        const size_t s0 = (size_t)(y0 >> sy) * sm + (x0 >> sx);
        XH_HIP(copy2d(mod[c] + s0, dmod[c] + s0, (size_t)sm * 2, (size_t)((cw * 4) >> sx) * 2, (size_t)((nh * 4) >> sy), hipMemcpyDeviceToHost));
    }
    XH_HIP(hipStreamSynchronize(C.st));
    return XEVE_HIP_OK;
}

// ---- host-memory form of one xeve_pinter_analyze_cu call with RESIDENT pictures: per-thread device state ------------------------------------------------------------
// One stream, one device arena (job | state | result | coefficients | reconstruction | prediction | exit state | workspace) and one pinned host mirror of the small
// records per encoder thread: a call is one upload of (job, state), the launches, one download of the outputs.
namespace {
// One CU's call is ~200 small dependent launches: issued one by one they cost the host 5-7 ms per CU (measured, 1280x720 and 1920x1080 encodes); the
// whole call -- upload of (job, state), every launch, download of the results -- is therefore captured ONCE per (CU size, picture parameters) into a HIP
// graph and replayed for every further CU of that size in the picture (all operands sit at fixed addresses of the per-thread arena; the planes are the
// picture's resident copies).  The key is everything the launches bake in: the parameter record, the plane table, strides, the coefficient tables.
struct HostGraph {
    std::vector<char> key;
    hipGraph_t        graph = nullptr;
    hipGraphExec_t    exec  = nullptr;
};
struct InterHostCtx { // the arena plus the graphs, which hold its device AND pinned addresses: the pinned request is constant, so that buffer never moves after the first call
    XhHostArena            A;
    std::vector<HostGraph> graphs;
    static constexpr size_t IN_BYTES = 512, OUT_BYTES = 64 << 10; // in: job + state; out: result, exit state, coef, rec, pred (64x64: 12 + 12.1 + 8 KB)
    void drop_graphs()
    {
        for(auto &g : graphs) {
            if(g.exec) (void)hipGraphExecDestroy(g.exec);
            if(g.graph) (void)hipGraphDestroy(g.graph);
        }
        graphs.clear();
    }
    int ensure(size_t ws_bytes)
    {
        const int rc = A.ensure(IN_BYTES + OUT_BYTES, ws_bytes);
        if(A.moved) drop_graphs(), A.moved = false; // (they hold the old arena's addresses)
        return rc;
    }
    ~InterHostCtx() { drop_graphs(); }
};
} // namespace

static int inter_host_resident(const xeve_hip_pel *const org[3], int s_org_l, int s_org_c, const xeve_hip_refpic *refp, int s_l, int s_c, const XhPlaneExtents &E,
                               const xeve_hip_sbac *state, const xeve_hip_inter_params *p, const xeve_hip_inter_job *job, const int16_t (*coef_l)[8],
                               const int16_t (*coef_c)[4], xeve_hip_inter_result *result, int16_t *coef_y, int16_t *coef_u, int16_t *coef_v, xeve_hip_pel *rec_y,
                               xeve_hip_pel *rec_u, xeve_hip_pel *rec_v, xeve_hip_pel *pred_y, xeve_hip_sbac *next_best)
{
    static thread_local InterHostCtx C;
    const xeve_hip_rdo_params &rp = p->rdo;
    const int idc = rp.chroma_format_idc, ws = idc <= 2, hs = idc <= 1, ncomp = idc ? 3 : 1, isb = rp.slice_type == 0;
    const size_t n0 = (size_t)1 << (2 * rp.log2_cuw), n1 = idc ? n0 >> (ws + hs) : 0;
    const size_t wsb = xeve_hip_pinter_analyze_cu_workspace(1, 1, p, s_org_l, s_org_c);
    int rc = C.ensure(wsb);
    if(rc != XEVE_HIP_OK) return rc;
    const hipStream_t st = C.A.st;
    // planes: the picture's resident copies (uploaded on first sight)
    const pel *dorg[3] = {nullptr, nullptr, nullptr};
    for(int c = 0; c < ncomp; c++) {
        dorg[c] = (const pel *)xh_resident(org[c], E.org[c] * sizeof(pel));
        if(!dorg[c]) return XEVE_HIP_ERR_DEVICE;
    }
    xeve_hip_refpic tab[2 * XEVE_HIP_MAX_REFP];
    if((rc = xh_resident_reftab(tab, refp, rp.num_refp[0], isb ? rp.num_refp[1] : 0, ncomp, E)) != XEVE_HIP_OK) return rc;
    // arena layout
    char *d = C.A.dev, *h = C.A.pin;
    const size_t o_job = 0, o_state = 256;                                                                       // in
    const size_t o_res = InterHostCtx::IN_BYTES, o_nb = o_res + 256, o_coef = o_nb + 256, o_rec = o_coef + xh_al((n0 + 2 * n1) * 2),
                 o_pred = o_rec + xh_al((n0 + 2 * n1 + 16) * 2), o_end = o_pred + n0 * 2;                        // out
    XH_REQUIRE(o_end <= InterHostCtx::IN_BYTES + InterHostCtx::OUT_BYTES);
    const size_t o_ws = xh_al(InterHostCtx::IN_BYTES + InterHostCtx::OUT_BYTES);
    xeve_hip_inter_job j0 = *job;
    j0.sbac = 0;
    memcpy(h + o_job, &j0, sizeof(j0)), memcpy(h + o_state, state, sizeof(*state));
    pel *drec = (pel *)(d + o_rec);
    auto enqueue = [&]() -> int { // the whole call on the arena's stream
        XH_HIP(hipMemcpyAsync(d, h, InterHostCtx::IN_BYTES, hipMemcpyHostToDevice, st));
        int r = xeve_hip_pinter_analyze_cu_jobs(dorg, s_org_l, s_org_c, tab, s_l, s_c, (const xeve_hip_sbac *)(d + o_state), 1, p, (const xeve_hip_inter_job *)(d + o_job), 1,
                                                coef_l, coef_c, (xeve_hip_inter_result *)(d + o_res), (int16_t *)(d + o_coef), drec, drec + n0 + 8, drec + n0 + n1 + 16,
                                                (pel *)(d + o_pred), (xeve_hip_sbac *)(d + o_nb), d + o_ws, wsb, st);
        if(r != XEVE_HIP_OK) return r;
        XH_HIP(hipMemcpyAsync(h + o_res, d + o_res, o_end - o_res, hipMemcpyDeviceToHost, st));
        return XEVE_HIP_OK;
    };
    static const int use_graph = getenv("XEVE_HIP_HOST_GRAPH") ? atoi(getenv("XEVE_HIP_HOST_GRAPH")) : 1; // developer switch (measurement)
    if(use_graph && !xh_prof_on(XH_PROF_SEARCH) && !xh_prof_on(XH_PROF_CU_BITS)) {
        std::vector<char> key(sizeof(*p) + sizeof(tab) + sizeof(dorg) + 4 * sizeof(int) + 2 * sizeof(void *));
        char *k = key.data();
        memcpy(k, p, sizeof(*p)), k += sizeof(*p);
        memcpy(k, tab, sizeof(tab)), k += sizeof(tab);
        memcpy(k, dorg, sizeof(dorg)), k += sizeof(dorg);
        const int strides[4] = {s_org_l, s_org_c, s_l, s_c};
        memcpy(k, strides, sizeof(strides)), k += sizeof(strides);
        const void *ct[2] = {(const void *)coef_l, (const void *)coef_c};
        memcpy(k, ct, sizeof(ct));
        HostGraph *g = nullptr;
        for(auto &c : C.graphs)
            if(c.key == key) {
                g = &c;
                break;
            }
        if(!g) {
            if(C.graphs.size() >= 64) C.drop_graphs();
            HostGraph ng;
            XH_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
            rc = enqueue();
            const hipError_t ec = hipStreamEndCapture(st, &ng.graph);
            if(rc != XEVE_HIP_OK) {
                if(ng.graph) (void)hipGraphDestroy(ng.graph);
                return rc;
            }
            XH_HIP(ec);
            XH_HIP(hipGraphInstantiate(&ng.exec, ng.graph, nullptr, nullptr, 0));
            ng.key = key;
            C.graphs.push_back(std::move(ng));
            g = &C.graphs.back();
        }
        XH_HIP(hipGraphLaunch(g->exec, st));
    }
    else {
        rc = enqueue();
        if(rc != XEVE_HIP_OK) return rc;
    }
    XH_HIP(hipStreamSynchronize(st));
    memcpy(result, h + o_res, sizeof(*result)), memcpy(next_best, h + o_nb, sizeof(*next_best));
    memcpy(coef_y, h + o_coef, n0 * 2), memcpy(rec_y, h + o_rec, n0 * 2);
    if(pred_y) memcpy(pred_y, h + o_pred, n0 * 2);
    if(idc) {
        memcpy(coef_u, h + o_coef + n0 * 2, n1 * 2), memcpy(coef_v, h + o_coef + (n0 + n1) * 2, n1 * 2);
        memcpy(rec_u, h + o_rec + (n0 + 8) * 2, n1 * 2), memcpy(rec_v, h + o_rec + (n0 + n1 + 16) * 2, n1 * 2);
    }
    return XEVE_HIP_OK;
}

// ---- host-memory form of one xeve_pinter_analyze_cu call (the table layer's style: synchronous, every plane staged per call) ----------
// What ctx->fn_pinter_analyze_cu can be pointed at (tests/test_integration_ref.py does, through shim/xeve_hip_shim.c).  org / refp: HOST pointers to
// sample (0, 0); the reference planes extend pad_l / pad_c samples around the picture.
extern "C" int xeve_hip_pinter_analyze_cu_host(const xeve_hip_pel *const org[3], int s_org_l, int s_org_c, const xeve_hip_refpic *refp, int s_l, int s_c, int pad_l,
                                               int pad_c, const xeve_hip_sbac *state, const xeve_hip_inter_params *p, const xeve_hip_inter_job *job,
                                               const int16_t (*coef_l)[8], const int16_t (*coef_c)[4], xeve_hip_inter_result *result, int16_t *coef_y,
                                               int16_t *coef_u, int16_t *coef_v, xeve_hip_pel *rec_y, xeve_hip_pel *rec_u, xeve_hip_pel *rec_v,
                                               xeve_hip_pel *pred_y, xeve_hip_sbac *next_best)
{
    XH_ENTER();
    XH_REQUIRE(org && org[0] && refp && state && p && job && result && coef_y && rec_y && next_best && inter_params_ok(p) && pad_l >= 0 && pad_c >= 0);
    const xeve_hip_rdo_params &rp = p->rdo;
    const int idc = rp.chroma_format_idc, ws = idc <= 2, hs = idc <= 1, ncomp = idc ? 3 : 1, isb = rp.slice_type == 0;
    XH_REQUIRE(idc == 0 || (org[1] && org[2] && coef_u && coef_v && rec_u && rec_v));
    const XhPlaneExtents E(s_org_l, s_org_c, s_l, s_c, pad_l, pad_c, rp.pic_h, hs);
    if(xh_resident_on()) // the caller announces its pictures: planes are resident, the call moves a job and a CU's worth of results
        return inter_host_resident(org, s_org_l, s_org_c, refp, s_l, s_c, E, state, p, job, coef_l, coef_c, result, coef_y, coef_u, coef_v, rec_y, rec_u, rec_v, pred_y, next_best);
    const size_t n0 = (size_t)1 << (2 * rp.log2_cuw), n1 = idc ? n0 >> (ws + hs) : 0;
    // the pictures both lists hold (a picture may sit in both: staged once)
    constexpr int MAXR = XEVE_HIP_MAX_REFP;
    const int nr[2] = {rp.num_refp[0], isb ? rp.num_refp[1] : 0};
    const xeve_hip_pel *uniq[2 * MAXR];
    int nu = 0, which[2 * MAXR];
    for(int l = 0; l < 2; l++)
        for(int r = 0; r < nr[l]; r++) {
            const xeve_hip_refpic &e = refp[r * 2 + l];
            XH_REQUIRE(e.y && (idc == 0 || (e.u && e.v)));
            int k = 0;
            while(k < nu && uniq[k] != e.y) k++;
            if(k == nu) uniq[nu++] = e.y;
            which[r * 2 + l] = k;
        }
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += xh_al(bytes); return r; };
    size_t o_org[3], o_ref[2 * MAXR][3];
    for(int c = 0; c < ncomp; c++) o_org[c] = take(E.org[c] * sizeof(pel));
    for(int k = 0; k < nu; k++)
        for(int c = 0; c < ncomp; c++) o_ref[k][c] = take(E.ref[c] * sizeof(pel));
    const size_t o_state = take(sizeof(xeve_hip_sbac)), o_job = take(sizeof(xeve_hip_inter_job)), o_res = take(sizeof(xeve_hip_inter_result));
    const size_t o_coef = take((n0 + 2 * n1) * 2), o_rec = take((n0 + 2 * n1 + 16) * 2), o_pred = take(n0 * 2), o_nb = take(sizeof(xeve_hip_sbac));
    const size_t wsb = xeve_hip_pinter_analyze_cu_workspace(1, 1, p, s_org_l, s_org_c), o_ws = take(wsb);
    XhScratch S("xeve_hip_pinter_analyze_cu_host");
    char *d = S.alloc(o);
    if(!S.ok()) return S.rc;
    for(int c = 0; c < ncomp; c++) S.up(d + o_org[c], org[c], E.org[c] * sizeof(pel));
    xeve_hip_refpic tab[2 * MAXR];
    memset(tab, 0, sizeof(tab));
    bool done[2 * MAXR] = {};
    for(int l = 0; l < 2; l++)
        for(int r = 0; r < nr[l]; r++) {
            const xeve_hip_refpic &e = refp[r * 2 + l];
            const int k = which[r * 2 + l];
            const xeve_hip_pel *hp[3] = {e.y, e.u, e.v};
            if(!done[k])
                for(int c = 0; c < ncomp; c++) S.up(d + o_ref[k][c], hp[c] - E.ref0[c], E.ref[c] * sizeof(pel));
            done[k] = true;
            xeve_hip_refpic &t = tab[r * 2 + l];
            t.y = (pel *)(d + o_ref[k][0]) + E.ref0[0], t.poc = e.poc;
            if(idc) t.u = (pel *)(d + o_ref[k][1]) + E.ref0[1], t.v = (pel *)(d + o_ref[k][2]) + E.ref0[2];
        }
    if(!isb) tab[0 * 2 + 1] = tab[0 * 2 + 0]; // (P slices never read list 1; keep the table addressable)
    xeve_hip_inter_job j0 = *job;
    j0.sbac = 0;
    S.up(d + o_state, state, sizeof(*state)), S.up(d + o_job, &j0, sizeof(j0));
    if(S.ok()) {
        const pel *dorg[3] = {(pel *)(d + o_org[0]), idc ? (pel *)(d + o_org[1]) : nullptr, idc ? (pel *)(d + o_org[2]) : nullptr};
        pel *drec = (pel *)(d + o_rec);
        S.run(xeve_hip_pinter_analyze_cu_jobs(dorg, s_org_l, s_org_c, tab, s_l, s_c, (const xeve_hip_sbac *)(d + o_state), 1, p, (const xeve_hip_inter_job *)(d + o_job), 1,
                                              coef_l, coef_c, (xeve_hip_inter_result *)(d + o_res), (int16_t *)(d + o_coef), drec, drec + n0 + 8, drec + n0 + n1 + 16,
                                              (pel *)(d + o_pred), (xeve_hip_sbac *)(d + o_nb), d + o_ws, wsb, nullptr));
        if(S.ok()) S.check(hipStreamSynchronize(nullptr), "the analysis");
    }
    S.down(result, d + o_res, sizeof(*result)), S.down(coef_y, d + o_coef, n0 * 2), S.down(rec_y, d + o_rec, n0 * 2), S.down(next_best, d + o_nb, sizeof(*next_best));
    if(pred_y) S.down(pred_y, d + o_pred, n0 * 2);
    if(idc) {
        S.down(coef_u, d + o_coef + n0 * 2, n1 * 2), S.down(coef_v, d + o_coef + (n0 + n1) * 2, n1 * 2);
        S.down(rec_u, d + o_rec + (n0 + 8) * 2, n1 * 2), S.down(rec_v, d + o_rec + (n0 + n1 + 16) * 2, n1 * 2);
    }
    return S.rc;
}
