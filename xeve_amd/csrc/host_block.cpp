// xeve_amd/csrc/host_block.cpp -- host-memory forms in the table layer's style: ONE block, CU or picture per call, staged per call on the null stream (XhScratch,
// host_stage.h: no stream, no pinned memory), synchronous.  What pi->fn_me, pi->fn_mc, ctx->fn_eco_coef, the per-component loops of ctx->fn_tq / ctx->fn_itdp,
// ctx->fn_loop_filter and ctx->fn_picbuf_expand can be pointed at (tests/test_integration_ref.py does, through shim/xeve_hip_shim.c).
#include "host_stage.h"

// ---- one pinter_me_epzs call.  org0 / ref0: sample (0, 0) of the original luma plane (rows 0 .. pic_h - 1 are read) and of the padded reference luma plane (pad
// samples around the picture).
extern "C" int xeve_hip_me_epzs_host(const pel *org0, int s_org, const pel *org_bi, const pel *ref0, int s_ref, int pad, int pic_h,
                                     const xeve_hip_epzs_job *job, int log2w, int log2h, int bit_depth, const int16_t (*coef)[8],
                                     const xeve_hip_epzs_params *params, xeve_hip_me_result *result)
{
    XH_ENTER();
    XH_REQUIRE(org0 && ref0 && job && params && result && pad >= 0 && pic_h > 0);
    const size_t eo = (size_t)s_org * pic_h, er = (size_t)s_ref * (pic_h + 2 * pad), ro = (size_t)pad * s_ref + pad, nb = (size_t)1 << (log2w + log2h);
    const size_t wsb = xeve_hip_me_epzs_workspace(1);
    XhScratch S("xeve_hip_me_epzs_host");
    pel  *d_org = S.stage<pel>(org0, eo * sizeof(pel)), *d_ref = S.stage<pel>(ref0 - ro, er * sizeof(pel)), *d_bi = org_bi ? S.stage<pel>(org_bi, nb * sizeof(pel)) : nullptr;
    char *d_misc = S.alloc(512 + wsb); // job | result | workspace
    xeve_hip_epzs_job j0 = *job;
    j0.org_off = 0; // one job: its org_bi block is the whole buffer
    S.up(d_misc, &j0, sizeof(j0));
    if(S.ok())
        S.run(xeve_hip_me_epzs_jobs(d_org, s_org, d_bi, d_ref + ro, s_ref, (const xeve_hip_epzs_job *)d_misc, 1, log2w, log2h, bit_depth, coef, params,
                                    (xeve_hip_me_result *)(d_misc + 256), d_misc + 512, wsb, nullptr));
    S.down(result, d_misc + 256, sizeof(*result));
    return S.rc;
}

// ---- one xeve_mc call (pinter_mc, xeve_pinter.c:2058-2085).  refp: table [refi * 2 + list] of HOST plane pointers (sample (0, 0)); the planes extend pad_l / pad_c
// samples around the picture.  Only the (at most two) pictures the job uses are staged.
extern "C" int xeve_hip_mc_cu_host(const xeve_hip_refpic *refp, int num_refp0, int num_refp1, int s_l, int s_c, int pad_l, int pad_c, int pic_w, int pic_h,
                                   const xeve_hip_cu_mc_job *job, int w, int h, int bit_depth_luma, int bit_depth_chroma, int chroma_format_idc,
                                   const int16_t (*coef_l)[8], const int16_t (*coef_c)[4], pel *pred_y, pel *pred_u, pel *pred_v)
{
    XH_ENTER();
    XH_REQUIRE(refp && job && pred_y && num_refp0 >= 0 && num_refp0 <= XEVE_HIP_MAX_REFP && num_refp1 >= 0 && num_refp1 <= XEVE_HIP_MAX_REFP);
    const int idc = chroma_format_idc, ws = idc <= 2, hs = idc <= 1, nmax = num_refp0 > num_refp1 ? num_refp0 : num_refp1;
    const size_t el = (size_t)s_l * (pic_h + 2 * pad_l), ec = idc ? (size_t)s_c * ((pic_h >> hs) + 2 * pad_c) : 0;
    const size_t ol = (size_t)pad_l * s_l + pad_l, oc = (size_t)pad_c * s_c + pad_c;
    const size_t n0 = (size_t)w * h, n1 = idc ? n0 >> (ws + hs) : 0;
    xeve_hip_refpic tab[2 * XEVE_HIP_MAX_REFP];
    memset(tab, 0, sizeof(tab));
    XhScratch S("xeve_hip_mc_cu_host");
    for(int r = 0; r < nmax; r++)
        for(int l = 0; l < 2; l++) tab[r * 2 + l].poc = refp[r * 2 + l].poc;
    for(int l = 0; l < 2 && S.ok(); l++) {
        const int ri = job->refi[l];
        if(ri < 0) continue;
        XH_REQUIRE(ri < (l ? num_refp1 : num_refp0));
        const xeve_hip_refpic &src = refp[ri * 2 + l];
        const pel *hp[3] = {src.y, src.u, src.v};
        pel       *staged[3] = {nullptr, nullptr, nullptr};
        for(int c = 0; c < (idc ? 3 : 1); c++) staged[c] = S.stage<pel>(hp[c] - (c ? oc : ol), (c ? ec : el) * sizeof(pel));
        // every picture a list holds must be addressable for the per-picture launches; unused ones alias the staged one (their jobs are switched off)
        for(int r = 0; r < (l ? num_refp1 : num_refp0); r++)
            tab[r * 2 + l].y = staged[0] + ol, tab[r * 2 + l].u = idc ? staged[1] + oc : nullptr, tab[r * 2 + l].v = idc ? staged[2] + oc : nullptr;
    }
    // a list the job does not use still needs valid pointers for its (switched-off) launches: borrow the other list's planes
    for(int l = 0; l < 2; l++)
        if(job->refi[l] < 0)
            for(int r = 0; r < (l ? num_refp1 : num_refp0); r++) tab[r * 2 + l].y = tab[(job->refi[1 - l]) * 2 + (1 - l)].y, tab[r * 2 + l].u = tab[(job->refi[1 - l]) * 2 + (1 - l)].u, tab[r * 2 + l].v = tab[(job->refi[1 - l]) * 2 + (1 - l)].v;
    const size_t wsb = xeve_hip_mc_cu_workspace(1, w, h, num_refp0, num_refp1), o_pred = 256, o_ws = xh_al(o_pred + (n0 + 2 * n1) * sizeof(pel));
    char *d = S.alloc(o_ws + wsb);
    S.up(d, job, sizeof(*job));
    pel *dp = (pel *)(d + o_pred);
    if(S.ok())
        S.run(xeve_hip_mc_cu_jobs(tab, num_refp0, num_refp1, s_l, s_c, pic_w, pic_h, (const xeve_hip_cu_mc_job *)d, 1, w, h, bit_depth_luma, bit_depth_chroma, idc, coef_l,
                                  coef_c, dp, dp + n0, dp + n0 + n1, d + o_ws, wsb, nullptr));
    S.down(pred_y, dp, n0 * sizeof(pel));
    if(idc) S.down(pred_u, dp + n0, n1 * sizeof(pel)), S.down(pred_v, dp + n0 + n1, n1 * sizeof(pel));
    return S.rc;
}

// ---- one xeve_eco_coef call in bit-count mode (sbac->is_bitcount): the cbf flags and the coefficients of one CU go through the GPU coder, continuing from *state
// exactly where it stands, and *state is left as the reference's coder would leave it.
extern "C" int xeve_hip_eco_coef_host(xeve_hip_sbac *state, const int16_t *coef_y, const int16_t *coef_u, const int16_t *coef_v, int log2_cuw, int log2_cuh,
                                      const int32_t nnz[3], int flags, int chroma_format_idc, int cm_init)
{
    XH_ENTER();
    XH_REQUIRE(state && coef_y && nnz && log2_cuw >= 2 && log2_cuw <= 6 && log2_cuh >= 2 && log2_cuh <= 6 && chroma_format_idc >= 0 && chroma_format_idc <= 3);
    XH_REQUIRE(chroma_format_idc == 0 || (coef_u && coef_v));
    const int ws = chroma_format_idc <= 2, hs = chroma_format_idc <= 1;
    const size_t n0 = (size_t)1 << (log2_cuw + log2_cuh), n1 = chroma_format_idc ? n0 >> (ws + hs) : 0, ne = n0 + 2 * n1;
    xeve_hip_cu_bits_params p;
    p.log2_cuw = log2_cuw, p.log2_cuh = log2_cuh, p.slice_type = 0, p.num_refp[0] = p.num_refp[1] = 0, p.cm_init = cm_init, p.chroma_format_idc = chroma_format_idc;
    xeve_hip_cu_bits_job j;
    memset(&j, 0, sizeof(j));
    j.coef_off[0] = 0, j.coef_off[1] = (int)n0, j.coef_off[2] = (int)(n0 + n1), j.nnz[0] = nnz[0], j.nnz[1] = nnz[1], j.nnz[2] = nnz[2];
    j.mode = XEVE_HIP_BITS_ECO_COEF, j.dir_flag = (uint8_t)(flags | XEVE_HIP_ECO_NO_RESET);
    const size_t o_job = xh_al(ne * 2), o_st = o_job + 256, o_bits = o_st + 2 * 256, o_ws = o_bits + 256;
    const size_t wsb = xeve_hip_cu_bits_workspace(1, ne);
    XhScratch S("xeve_hip_eco_coef_host");
    char *d = S.alloc(o_ws + wsb);
    S.up(d, coef_y, n0 * 2);
    if(n1) S.up(d + n0 * 2, coef_u, n1 * 2), S.up(d + (n0 + n1) * 2, coef_v, n1 * 2);
    S.up(d + o_job, &j, sizeof(j)), S.up(d + o_st, state, sizeof(*state));
    if(S.ok())
        S.run(xeve_hip_cu_bits_jobs((const int16_t *)d, ne, (const xeve_hip_sbac *)(d + o_st), (const xeve_hip_cu_bits_job *)(d + o_job), 1, &p, d + o_ws, wsb,
                                    (uint32_t *)(d + o_bits), (xeve_hip_sbac *)(d + o_st + 256), nullptr));
    S.down(state, d + o_st + 256, sizeof(*state));
    return S.rc;
}

// ---- one transform block: xeve_tq_nnz (xeve_tq.c:729-748) = xeve_trans + xeve_quant_nnz, and itdq_cu (xeve_itdq.c:454-497) = xeve_dquant + xeve_itrans, on a
// dense block in HOST memory: what the per-component loops of ctx->fn_tq (xeve_sub_block_tq) / ctx->fn_itdp (xeve_itdq) call.
extern "C" int xeve_hip_tq_nnz_host(int16_t *coef, int log2w, int log2h, int qp, double lambda, int ch_type, int is_intra_cu, int is_intra_slice,
                                    int bit_depth, int tool_iqt, const xeve_hip_rdoq_est_full *est, int use_rdoq, int32_t *nnz)
{
    XH_ENTER();
    XH_REQUIRE(coef && nnz && (est || !use_rdoq) && log2w >= 1 && log2w <= 6 && log2h >= 1 && log2h <= 6 && qp >= 0 && qp <= 87);
    const size_t n = (size_t)1 << (log2w + log2h), off_nnz = (n * 2 + 15) & ~(size_t)15, off_est = off_nnz + 16;
    XhScratch S("xeve_hip_tq_nnz_host");
    char *d = S.alloc(off_est + sizeof(*est));
    S.up(d, coef, n * 2);
    if(use_rdoq) S.up(d + off_est, est, sizeof(*est));
    if(S.ok()) S.run(xeve_hip_trans((int16_t *)d, 1, log2w, log2h, bit_depth, nullptr));
    if(S.ok())
        S.run(use_rdoq ? xeve_hip_rdoq_dev((int16_t *)d, 1, log2w, log2h, qp, lambda, ch_type, bit_depth, tool_iqt, (const xeve_hip_rdoq_est_full *)(d + off_est), nullptr,
                                           1, is_intra_slice, is_intra_cu, (int32_t *)(d + off_nnz), nullptr)
                       : xeve_hip_quant((int16_t *)d, 1, log2w, log2h, qp, k_quant_scale[tool_iqt][qp % 6], is_intra_slice, bit_depth, (int32_t *)(d + off_nnz), nullptr));
    S.down(coef, d, n * 2), S.down(nnz, d + off_nnz, 4);
    return S.rc;
}

extern "C" int xeve_hip_itdq_host(int16_t *coef, int log2w, int log2h, int qp, int bit_depth)
{
    XH_ENTER();
    XH_REQUIRE(coef && log2w >= 1 && log2w <= 6 && log2h >= 1 && log2h <= 6 && qp >= 0 && qp <= 87);
    static const int dq[6] = {40, 45, 51, 57, 64, 71}; // xeve_tbl_dq_scale_b (xeve_tbl.c:237), scale << (qp / 6) (xeve_itdq.c:549)
    const size_t n = (size_t)1 << (log2w + log2h);
    XhScratch S("xeve_hip_itdq_host");
    int16_t  *d = S.stage<int16_t>(coef, n * 2);
    if(S.ok()) S.run(xeve_hip_dquant(d, 1, log2w, log2h, dq[qp % 6] << (qp / 6), bit_depth, nullptr));
    if(S.ok()) S.run(xeve_hip_itrans(d, 1, log2w, log2h, bit_depth, nullptr));
    S.down(coef, d, n * 2);
    return S.rc;
}

// ---- ctx->fn_loop_filter / ctx->fn_picbuf_expand: whole padded planes are staged per call -- a correctness path, like the other table entries -------------------
extern "C" int xeve_hip_deblock_host(xeve_hip_pel *y, xeve_hip_pel *u, xeve_hip_pel *v, int s_l, int s_c, int pad_l, int pad_c, const uint32_t *map_scu,
                                     const uint32_t *map_cu_mode, const uint8_t *map_tidx, const int8_t *map_refi, const int16_t *map_mv,
                                     const xeve_hip_deblock_params *p)
{
    XH_ENTER();
    XH_REQUIRE(p && y && map_scu && map_cu_mode && map_refi && map_mv && pad_l >= 0 && pad_c >= 0);
    const int idc = p->chroma_format_idc, hs = idc <= 1;
    const size_t n = (size_t)p->w_scu * p->h_scu;
    const size_t el = (size_t)s_l * (p->h + 2 * pad_l) * sizeof(pel), ec = idc ? (size_t)s_c * ((p->h >> hs) + 2 * pad_c) * sizeof(pel) : 0; // bytes
    const size_t ol = (size_t)pad_l * s_l + pad_l, oc = (size_t)pad_c * s_c + pad_c;
    const void  *hm[5] = {map_scu, map_cu_mode, map_refi, map_mv, map_tidx};
    const size_t ms[5] = {n * 4, n * 4, n * 2, n * 8, n};
    XhScratch S("xeve_hip_deblock_host");
    pel  *d[3] = {S.stage<pel>(y - ol, el), idc ? S.stage<pel>(u - oc, ec) : nullptr, idc ? S.stage<pel>(v - oc, ec) : nullptr};
    void *m[5];
    for(int i = 0; i < 5; i++) m[i] = hm[i] ? S.stage(hm[i], ms[i]) : nullptr; // (map_tidx == NULL: one tile)
    if(S.ok())
        S.run(xeve_hip_deblock(d[0] + ol, idc ? d[1] + oc : nullptr, idc ? d[2] + oc : nullptr, s_l, s_c, (const uint32_t *)m[0], (const uint32_t *)m[1],
                               (const uint8_t *)m[4], (const int8_t *)m[2], (const int16_t *)m[3], p, nullptr));
    S.down(y - ol, d[0], el);
    if(idc) S.down(u - oc, d[1], ec), S.down(v - oc, d[2], ec);
    return S.rc;
}

extern "C" int xeve_hip_picbuf_expand_host(xeve_hip_pel *y, xeve_hip_pel *u, xeve_hip_pel *v, int s_l, int s_c, int w_l, int h_l, int w_c, int h_c,
                                           int exp_l, int exp_c, int chroma_format_idc)
{
    XH_ENTER();
    XH_REQUIRE(y && exp_l > 0 && (chroma_format_idc == 0 || (u && v && exp_c > 0)));
    const int    idc = chroma_format_idc;
    const size_t el = (size_t)s_l * (h_l + 2 * exp_l) * sizeof(pel), ec = idc ? (size_t)s_c * (h_c + 2 * exp_c) * sizeof(pel) : 0; // bytes
    const size_t ol = (size_t)exp_l * s_l + exp_l, oc = (size_t)exp_c * s_c + exp_c;
    XhScratch S("xeve_hip_picbuf_expand_host");
    pel *d[3] = {S.stage<pel>(y - ol, el), idc ? S.stage<pel>(u - oc, ec) : nullptr, idc ? S.stage<pel>(v - oc, ec) : nullptr};
    if(S.ok()) S.run(xeve_hip_picbuf_expand(d[0] + ol, idc ? d[1] + oc : nullptr, idc ? d[2] + oc : nullptr, s_l, s_c, w_l, h_l, w_c, h_c, exp_l, exp_c, idc, nullptr));
    S.down(y - ol, d[0], el);
    if(idc) S.down(u - oc, d[1], ec), S.down(v - oc, d[2], ec);
    return S.rc;
}
