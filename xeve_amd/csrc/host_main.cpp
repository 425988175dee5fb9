// xeve_amd/csrc/host_main.cpp -- host-memory forms of the Main profile's tools: affine motion compensation and the affine gradient search (per-thread arena), the
// adaptive loop filter's sample functions with the reference's signatures (staged per call, no status channel).  Host code on the batched entry points of affine.hip and
// alf.hip; who owns a stream or pinned memory is host_stage.h's table.
#include <vector>
#include "host_stage.h"

// ---- host-memory form of ONE xeve_affine_mc call (src_main/xevem_mc.c:2236-2339): what the Main-profile encoder's by-name calls can be routed to (the affine merge
// analysis, every round of the affine gradient search, the affine bi-prediction: xevem_pinter.c:1947, 4659, 4918 -- oracle/ref_shim_affine.c does).
// refp: table [refi * 2 + list] of HOST plane pointers (sample (0, 0)) of the pictures the CU uses; the planes extend pad_l / pad_c samples around the picture; pred_y /
// pred_u / pred_v: HOST blocks of w * h and (w / 2) * (h / 2) samples, what the reference leaves in pred[0][Y_C / U_C / V_C].  Per calling thread one stream and one device
// arena (grow-only): a call is the upload of the (at most two) pictures it uses, one launch, the download of three blocks.
extern "C" int xeve_hip_affine_mc_host(int x, int y, int pic_w, int pic_h, int w, int h, const int8_t refi[2], const int16_t mv[2][3][2], const xeve_hip_refpic *refp,
                                       int num_refp0, int num_refp1, int s_l, int s_c, int pad_l, int pad_c, xeve_hip_pel *pred_y, xeve_hip_pel *pred_u, xeve_hip_pel *pred_v,
                                       int vertex_num, int bit_depth)
{
    constexpr int MAXREF = XEVE_HIP_MAX_REFP;
    XH_ENTER();
    XH_REQUIRE(refi && mv && refp && pred_y && pred_u && pred_v && (vertex_num == 2 || vertex_num == 3) && pad_l >= 0 && pad_c >= 0 && s_l > 0 && s_c > 0 && pic_w > 0 && pic_h > 0);
    XH_REQUIRE(num_refp0 >= 0 && num_refp1 >= 0 && num_refp0 <= MAXREF && num_refp1 <= MAXREF && (refi[0] < 0 || refi[0] < num_refp0) && (refi[1] < 0 || refi[1] < num_refp1) &&
               (refi[0] >= 0 || refi[1] >= 0));
    const size_t el = (size_t)s_l * (pic_h + 2 * pad_l), ec = (size_t)s_c * ((pic_h >> 1) + 2 * pad_c), ol = (size_t)pad_l * s_l + pad_l, oc = (size_t)pad_c * s_c + pad_c;
    const size_t n0 = (size_t)w * h, n1 = n0 >> 2, plane = (el + 2 * ec) * sizeof(pel), o_planes = 256, o_pred = o_planes + 2 * xh_al(plane);
    static thread_local XhHostArena A;
    const int rc0 = A.ensure(o_pred + (n0 + 2 * n1) * sizeof(pel), 0);
    if(rc0 != XEVE_HIP_OK) return rc0;
    xeve_hip_affine_job J;
    memset(&J, 0, sizeof(J));
    J.x = x, J.y = y, J.vertex_num = (int8_t)vertex_num;
    xeve_hip_refpic tab[2 * MAXREF];
    memset(tab, 0, sizeof(tab));
    pel *first = nullptr;
    for(int l = 0; l < 2; l++) {
        J.refi[l] = refi[l];
        for(int v = 0; v < 3; v++) J.mv[l][v][0] = mv[l][v][0], J.mv[l][v][1] = mv[l][v][1];
        if(refi[l] < 0) continue;
        const xeve_hip_refpic &src = refp[refi[l] * 2 + l];
        XH_REQUIRE(src.y && src.u && src.v);
        pel *d = (pel *)(A.dev + o_planes + (size_t)l * xh_al(plane));
        XH_HIP(hipMemcpyAsync(d, src.y - ol, el * sizeof(pel), hipMemcpyHostToDevice, A.st));
        XH_HIP(hipMemcpyAsync(d + el, src.u - oc, ec * sizeof(pel), hipMemcpyHostToDevice, A.st));
        XH_HIP(hipMemcpyAsync(d + el + ec, src.v - oc, ec * sizeof(pel), hipMemcpyHostToDevice, A.st));
        if(!first) first = d;
        // every picture index a list is asked to hold must be addressable: all of them alias the staged one (the job names refi[l] alone)
        for(int r = 0; r < (l ? num_refp1 : num_refp0); r++) tab[r * 2 + l].y = d + ol, tab[r * 2 + l].u = d + el + oc, tab[r * 2 + l].v = d + el + ec + oc, tab[r * 2 + l].poc = src.poc;
    }
    for(int l = 0; l < 2; l++) // (a list the CU does not use: valid pointers for the table's check, never read)
        if(refi[l] < 0)
            for(int r = 0; r < (l ? num_refp1 : num_refp0); r++) tab[r * 2 + l].y = first + ol, tab[r * 2 + l].u = first + el + oc, tab[r * 2 + l].v = first + el + ec + oc;
    XH_HIP(hipMemcpyAsync(A.dev, &J, sizeof(J), hipMemcpyHostToDevice, A.st));
    pel *dp = (pel *)(A.dev + o_pred);
    const int rc = xeve_hip_affine_mc_jobs(tab, num_refp0, num_refp1, s_l, s_c, pic_w, pic_h, (const xeve_hip_affine_job *)A.dev, 1, w, h, bit_depth, dp, dp + n0, dp + n0 + n1, A.st);
    if(rc != XEVE_HIP_OK) return rc;
    XH_HIP(hipMemcpyAsync(pred_y, dp, n0 * sizeof(pel), hipMemcpyDeviceToHost, A.st));
    XH_HIP(hipMemcpyAsync(pred_u, dp + n0, n1 * sizeof(pel), hipMemcpyDeviceToHost, A.st));
    XH_HIP(hipMemcpyAsync(pred_v, dp + n0 + n1, n1 * sizeof(pel), hipMemcpyDeviceToHost, A.st));
    XH_HIP(hipStreamSynchronize(A.st));
    return XEVE_HIP_OK;
}

// ---- host-memory form of ONE pinter_affine_me_gradient call (src_main/xevem_pinter.c:4290-4501): what the Main-profile encoder's pi->fn_affine_me can be bound to
// (oracle/ref_shim_affine.c does).  ref_y: HOST luma plane (sample (0, 0)) of refp[refi][list].pic, extending pad_l samples around the picture; org: the CU's
// first original sample with its pitch (bi: pi->org_bi, pitch w); mv: in the start vectors, out the best ones (vertex_num of them); *cost: the function's value.  Per calling
// thread one stream and one device arena (grow-only): a call is the upload of the picture and of the CU's original, two launches, the download of the job record.
extern "C" int xeve_hip_affine_me_host(int x, int y, int pic_w, int pic_h, int w, int h, int refi, int list, const int16_t mvp[3][2], int16_t mv[3][2], int bi, int vertex_num,
                                       const xeve_hip_pel *ref_y, int s_l, int pad_l, const int16_t *org, int s_org, int bit_depth, uint32_t lambda_mv, int num_refp,
                                       int mot_bits_other, uint32_t *cost)
{
    XH_ENTER();
    XH_REQUIRE(mvp && mv && ref_y && org && cost && (vertex_num == 2 || vertex_num == 3) && pad_l >= 0 && s_l > 0 && s_org > 0 && pic_w > 0 && pic_h > 0);
    XH_REQUIRE(refi >= 0 && refi < XEVE_HIP_MAX_REFP && (list == 0 || list == 1) && num_refp > refi && num_refp <= 16 && xh_pow2(w) && xh_pow2(h) && w >= 16 && h >= 16 && w <= 128 &&
               h <= 128);
    const size_t el = (size_t)s_l * (pic_h + 2 * pad_l), ol = (size_t)pad_l * s_l + pad_l, n = (size_t)w * h;
    const size_t o_plane = 256, o_org = o_plane + xh_al(el * sizeof(pel)), total = o_org + n * sizeof(int16_t);
    static thread_local XhHostArena A;
    const int rc0 = A.ensure(total, 0);
    if(rc0 != XEVE_HIP_OK) return rc0;
    xeve_hip_affine_me_job *J = reinterpret_cast<xeve_hip_affine_me_job *>(A.pin);
    memset(J, 0, sizeof(*J));
    J->x = x, J->y = y, J->refi = (int8_t)refi, J->list = (int8_t)list, J->bi = (int8_t)(bi != 0), J->vertex_num = (int8_t)vertex_num, J->mot_bits_other = mot_bits_other;
    for(int v = 0; v < 3; v++)
        for(int c = 0; c < 2; c++) J->mvp[v][c] = v < vertex_num ? mvp[v][c] : (int16_t)0, J->mv[v][c] = v < vertex_num ? mv[v][c] : (int16_t)0;
    int16_t *ho = reinterpret_cast<int16_t *>(A.pin + o_org);
    for(int r = 0; r < h; r++) memcpy(ho + (size_t)r * w, org + (size_t)r * s_org, (size_t)w * sizeof(int16_t));
    XH_HIP(hipMemcpyAsync(A.dev, J, sizeof(*J), hipMemcpyHostToDevice, A.st));
    XH_HIP(hipMemcpyAsync(A.dev + o_org, ho, n * sizeof(int16_t), hipMemcpyHostToDevice, A.st));
    XH_HIP(hipMemcpyAsync(A.dev + o_plane, ref_y - ol, el * sizeof(pel), hipMemcpyHostToDevice, A.st));
    const int rc = xh_affine_me_dense(reinterpret_cast<const pel *>(A.dev + o_plane) + ol, refi, list, s_l, pic_w, pic_h, reinterpret_cast<const int16_t *>(A.dev + o_org),
                                      reinterpret_cast<xeve_hip_affine_me_job *>(A.dev), w, h, bit_depth, lambda_mv, num_refp, A.st);
    if(rc != XEVE_HIP_OK) return rc;
    XH_HIP(hipMemcpyAsync(J, A.dev, sizeof(*J), hipMemcpyDeviceToHost, A.st));
    XH_HIP(hipStreamSynchronize(A.st));
    for(int v = 0; v < vertex_num; v++) mv[v][0] = J->mv[v][0], mv[v][1] = J->mv[v][1];
    *cost = J->cost;
    return XEVE_HIP_OK;
}

// ---- the adaptive loop filter: host-memory forms with the reference's signatures (the ADAPTIVE_LOOP_FILTER object's function pointers).  No status channel: a refused
// call or a failed step ends the process (xh_die) -----------------------------------------------------------------------------------------------------------------------
namespace {
void alf_enter(const XhScratch &S, bool args_ok)
{
    if(!xh_ready()) xh_set_error("xeve_hip_init() has not been called"), xh_die(S.form);
    if(!args_ok) xh_set_error("invalid argument"), xh_die(S.form);
}
// rows [y0, y0 + rows) x columns [x0, x0 + cols) of a host plane (pointer at its sample (0, 0), either sign of offsets) -> a dense device buffer
void rows_up(XhScratch &S, pel *dev, const pel *host00, long stride, int y0, int x0, int rows, int cols)
{
    S.copy2d(dev, (size_t)cols * sizeof(pel), host00 + (long)y0 * stride + x0, (size_t)stride * sizeof(pel), (size_t)cols * sizeof(pel), rows, hipMemcpyHostToDevice);
}
// the classifier is a table of row pointers, indexed with the picture's coordinates: the area at (x, y) as a dense device block of pitch w
void cls_up(XhScratch &S, uint8_t *dev, uint8_t **classifier, int x, int y, int w, int h)
{
    std::vector<uint8_t> c((size_t)w * h);
    for(int i = 0; i < h; i++) memcpy(c.data() + (size_t)i * w, classifier[y + i] + x, (size_t)w);
    S.up(dev, c.data(), c.size());
}
void filter_host(int taps, uint8_t **classifier, pel *rec_dst, int dst_stride, const pel *rec_src, int src_stride, const xeve_hip_alf_area *blk, short *filter_set,
                 const xeve_hip_alf_clip_range *cr, const char *what)
{
    XhScratch S(what);
    alf_enter(S, rec_dst && rec_src && blk && filter_set && cr && blk->w > 0 && blk->h > 0 && ((blk->w | blk->h) & 3) == 0 && (taps == 5 || classifier));
    const int MG = xh_alf_margin(), w = blk->w, h = blk->h, sw = w + 2 * MG;
    pel     *src = S.alloc<pel>((size_t)sw * (h + 2 * MG) * sizeof(pel)), *dst = S.alloc<pel>((size_t)w * h * sizeof(pel));
    uint8_t *cls = S.alloc<uint8_t>((size_t)w * h);
    rows_up(S, src, rec_src, src_stride, -MG, -MG, h + 2 * MG, sw);
    if(taps == 7) cls_up(S, cls, classifier, blk->x, blk->y, w, h);
    const xeve_hip_alf_filter_job jb = {0, 0, w, h, 0, (int64_t)MG * sw + MG};
    const auto *job = S.stage<xeve_hip_alf_filter_job>(&jb, sizeof(jb));
    if(S.ok()) S.run(xeve_hip_alf_filter_jobs(taps, dst, w, src, sw, cls, w, job, 1, filter_set, cr->min, cr->max, nullptr));
    S.copy2d(rec_dst, (size_t)dst_stride * sizeof(pel), dst, (size_t)w * sizeof(pel), (size_t)w * sizeof(pel), h, hipMemcpyDeviceToHost);
    if(!S.ok()) xh_die(what);
}
} // namespace

extern "C" void xeve_hip_alf_derive_classification_blk_host(uint8_t **classifier, const xeve_hip_pel *src_luma, int src_stride, const xeve_hip_alf_area *blk, int shift,
                                                            int bit_depth)
{
    (void)shift; // (unused by the reference as well, :488-493)
    XhScratch S("xeve_hip_alf_derive_classification_blk_host");
    alf_enter(S, classifier && src_luma && blk && blk->w > 0 && blk->h > 0 && ((blk->w | blk->h) & 3) == 0);
    const int MG = xh_alf_margin(), w = blk->w, h = blk->h, sw = w + 2 * MG;
    pel     *src = S.alloc<pel>((size_t)sw * (h + 2 * MG) * sizeof(pel));
    uint8_t *cls = S.alloc<uint8_t>((size_t)w * h);
    rows_up(S, src, src_luma, src_stride, blk->y - MG, blk->x - MG, h + 2 * MG, sw);
    const xeve_hip_alf_area a = {0, 0, w, h};
    if(S.ok()) S.run(xeve_hip_alf_classify(cls, w, src + (size_t)MG * sw + MG, sw, &a, bit_depth, nullptr));
    std::vector<uint8_t> c((size_t)w * h);
    S.down(c.data(), cls, c.size());
    if(!S.ok()) xh_die(S.form);
    for(int i = 0; i < h; i++) memcpy(classifier[blk->y + i] + blk->x, c.data() + (size_t)i * w, (size_t)w);
}
extern "C" void xeve_hip_alf_filter_blk_7_host(uint8_t **classifier, xeve_hip_pel *rec_dst, int dst_stride, const xeve_hip_pel *rec_src, int src_stride,
                                               const xeve_hip_alf_area *blk, uint8_t comp_id, short *filter_set, const xeve_hip_alf_clip_range *clip_range)
{
    (void)comp_id;
    filter_host(7, classifier, rec_dst, dst_stride, rec_src, src_stride, blk, filter_set, clip_range, "xeve_hip_alf_filter_blk_7_host");
}
extern "C" void xeve_hip_alf_filter_blk_5_host(uint8_t **classifier, xeve_hip_pel *rec_dst, int dst_stride, const xeve_hip_pel *rec_src, int src_stride,
                                               const xeve_hip_alf_area *blk, uint8_t comp_id, short *filter_set, const xeve_hip_alf_clip_range *clip_range)
{
    (void)comp_id;
    filter_host(5, classifier, rec_dst, dst_stride, rec_src, src_stride, blk, filter_set, clip_range, "xeve_hip_alf_filter_blk_5_host");
}
extern "C" void xeve_hip_alf_get_blk_stats_host(int taps, xeve_hip_alf_covariance *alf_cov, uint8_t **classifier, const xeve_hip_pel *org0, int org_stride,
                                                const xeve_hip_pel *rec0, int rec_stride, int x, int y, int width, int height)
{
    XhScratch S("xeve_hip_alf_get_blk_stats_host");
    alf_enter(S, (taps == 5 || taps == 7) && alf_cov && org0 && rec0 && width > 0 && height > 0 && ((width | height) & 3) == 0);
    const int MG = xh_alf_margin(), w = width, h = height, sw = w + 2 * MG, nclasses = classifier ? 25 : 1, ncoef = taps * taps / 4 + 1;
    for(int c = 0; c < nclasses; c++)
        if(alf_cov[c].num_coef < ncoef || !alf_cov[c].E || !alf_cov[c].y) xh_set_error("a covariance record smaller than the filter shape"), xh_die(S.form);
    pel     *rec = S.alloc<pel>((size_t)sw * (h + 2 * MG) * sizeof(pel)), *org = S.alloc<pel>((size_t)w * h * sizeof(pel));
    uint8_t *cls = S.alloc<uint8_t>((size_t)w * h);
    std::vector<double> r((size_t)nclasses * (169 + 13 + 1));
    double *dE = S.alloc<double>(r.size() * sizeof(double)), *dy = dE + (size_t)nclasses * 169, *dp = dy + (size_t)nclasses * 13;
    rows_up(S, rec, rec0, rec_stride, y - MG, x - MG, h + 2 * MG, sw);
    rows_up(S, org, org0, org_stride, y, x, h, w);
    if(classifier) cls_up(S, cls, classifier, x, y, w, h);
    const xeve_hip_alf_area a = {0, 0, w, h};
    const auto *job = S.stage<xeve_hip_alf_area>(&a, sizeof(a));
    if(S.ok()) S.run(xeve_hip_alf_blk_stats_jobs(taps, classifier ? cls : nullptr, w, org, w, rec + (size_t)MG * sw + MG, sw, job, 1, dE, dy, dp, nullptr));
    S.down(r.data(), dE, r.size() * sizeof(double));
    if(!S.ok()) xh_die(S.form);
    const double *E = r.data(), *yv = E + (size_t)nclasses * 169, *pp = yv + (size_t)nclasses * 13;
    for(int c = 0; c < nclasses; c++) {
        for(int k = 0; k < ncoef; k++) {
            for(int l = k; l < ncoef; l++) alf_cov[c].E[k][l] += E[(c * 13 + k) * 13 + l];
            alf_cov[c].y[k] += yv[c * 13 + k];
        }
        alf_cov[c].pix_acc += pp[c];
        for(int k = 1; k < ncoef; k++)
            for(int l = 0; l < k; l++) alf_cov[c].E[k][l] = alf_cov[c].E[l][k];
    }
}
