// xeve_amd/csrc/host_stage.h -- the staging of the HOST-MEMORY FORMS (xeve_hip_*_host: INTEGRATION.md's drop-in route).  Included by host_block.cpp, host_cu.cpp,
// host_main.cpp and abi.cpp only; plain C++, no kernel.  A host-memory form takes the reference encoder's host pointers, stages ONE CU, CTU or block, calls a batched
// entry point of the C-ABI and copies the result back.
//
// WHO OWNS WHAT.  A live non-blocking stream that has moved pinned memory makes every later launch of the process ~1.5 us slower (cause open), so a
// form stages on an arena only where it did when that was measured, and a thread owns no more such streams than the rows below:
//   form                                         file             stream (non-blocking, per thread)   pinned memory       device memory
//   xeve_hip_pintra_analyze_cu_host              host_cu.cpp      XhHostArena                         XhHostArena         XhHostArena
//   xeve_hip_mode_analyze_ctu_intra_host         host_cu.cpp      XhHostArena                         XhHostArena         XhHostArena
//   xeve_hip_mode_analyze_ctu_host (P / B)       host_cu.cpp      TreePicCtx                          none (pageable)     TreePicCtx (picture-sized) + resident pictures
//   xeve_hip_pinter_analyze_cu_host, resident    host_cu.cpp      InterHostCtx = XhHostArena + graphs  XhHostArena, fixed  XhHostArena + resident pictures
//   xeve_hip_affine_mc_host                      host_main.cpp    XhHostArena                         XhHostArena         XhHostArena
//   xeve_hip_affine_me_host                      host_main.cpp    XhHostArena                         XhHostArena         XhHostArena
//   xeve_hip_pinter_analyze_cu_host, per call    host_cu.cpp      null stream                         none                XhScratch
//   xeve_hip_me_epzs_host, _mc_cu_host, _eco_coef_host, _tq_nnz_host, _itdq_host, _deblock_host, _picbuf_expand_host
//                                                host_block.cpp   null stream                         none                XhScratch
//   xeve_hip_alf_*_host (four)                   host_main.cpp    null stream                         none                XhScratch; a failure ends the process (xh_die)
//   (the dispatch tables: abi.cpp's Stage, one mapped pinned buffer and one stream per thread)
#pragma once
#include <algorithm>
#include <cstring>
#include "xh_common.h"

// ---- what the forms need from the kernel translation units ----------------------------------------------------------------------------------------------------------
XH_LOCAL bool intra_params_ok(const xeve_hip_intra_params *p);                             // intra.hip
XH_LOCAL bool inter_params_ok(const xeve_hip_inter_params *p);                             // inter.hip
XH_LOCAL bool tree_params_ok(const xeve_hip_tree_params *p);                               // tree.hip
XH_LOCAL bool tree_inter_ok(const xeve_hip_tree_params *p, const xeve_hip_tree_inter *I);  // tree.hip
XH_LOCAL extern const int k_quant_scale[2][6];                                             // rdoq.hip: xeve_quant_scale[tool_iqt][qp % 6]
XH_LOCAL int xh_alf_margin();                                                              // alf.hip: the samples its kernels read around an area
// one search on a dense original (org_block: w x h, pitch w) in the picture ref_y, all device memory: the launches of xeve_hip_affine_me_host (affine.hip)
XH_LOCAL int xh_affine_me_dense(const pel *ref_y, int refi, int list, int s_l, int pic_w, int pic_h, const int16_t *org_block, xeve_hip_affine_me_job *job, int w, int h,
                                int bit_depth, uint32_t lambda_mv, int num_refp, hipStream_t st);
// the end of an entry point that has no status channel (the dispatch tables, the ALF forms: their callers check nothing, a failure must not pass for a result): prints
// `what` with xeve_hip_last_error() in the caller's wording and aborts (abi.cpp)
[[noreturn]] XH_LOCAL void xh_die(const char *what, bool table_call = false);

static inline size_t xh_al(size_t v) { return (v + 255) & ~(size_t)255; }

// ---- per-thread staging of a form that runs a batched entry point on ONE unit: a stream, a pinned host buffer and a device arena that grow on demand and re-create
// themselves after xeve_hip_shutdown / _init.  `moved` is raised whenever the device arena or the pinned buffer is (re)allocated or released: an owner that keeps
// their addresses (InterHostCtx's graphs) drops what it keeps and clears it.
struct XhHostArena {
    uint32_t    gen = 0;
    hipStream_t st  = nullptr;
    char       *dev = nullptr, *pin = nullptr;
    size_t      dev_bytes = 0, pin_bytes = 0;
    bool        moved = false;
    void release()
    { // (errors ignored: at exit or after a shutdown the runtime may be gone already)
        if(st) (void)hipStreamDestroy(st);
        if(dev) (void)hipFree(dev);
        if(pin) (void)hipHostFree(pin);
        st = nullptr, dev = pin = nullptr, dev_bytes = pin_bytes = 0, moved = true;
    }
    int ensure(size_t io_bytes, size_t ws_bytes)
    {
        if(gen != xh_generation()) release(), gen = xh_generation(); // the library was shut down or re-bound since
        if(!st) XH_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        if(pin_bytes < io_bytes) {
            if(pin) (void)hipHostFree(pin);
            pin = nullptr, pin_bytes = 0, moved = true;
            XH_HIP(hipHostMalloc((void **)&pin, io_bytes + (io_bytes >> 1), hipHostMallocDefault));
            pin_bytes = io_bytes + (io_bytes >> 1);
        }
        const size_t need = io_bytes + 256 + ws_bytes;
        if(dev_bytes < need) {
            moved = true;
            if(dev) {
                XH_HIP(hipStreamSynchronize(st));
                (void)hipFree(dev);
                dev = nullptr, dev_bytes = 0;
            }
            XH_HIP(hipMalloc((void **)&dev, need + (need >> 2)));
            dev_bytes = need + (need >> 2);
        }
        return XEVE_HIP_OK;
    }
    ~XhHostArena() { release(); }
};

// ---- scoped staging of ONE call on the null stream: device blocks that are freed on scope exit, synchronous copies.  The first failure sets the error text with the
// form's name and the status; every later step is a no-op, so a form stages, checks ok() once, launches through run() and copies back.
namespace {
struct XhScratch {
    const char *form;
    int         rc = XEVE_HIP_OK, n = 0;
    void       *blk[12];
    explicit XhScratch(const char *form_name) : form(form_name) {}
    XhScratch(const XhScratch &) = delete;
    ~XhScratch() { while(n) (void)hipFree(blk[--n]); }
    bool ok() const { return rc == XEVE_HIP_OK; }
    void check(hipError_t e, const char *step)
    {
        if(e != hipSuccess && ok()) xh_set_error("%s: %s failed: %s", form, step, hipGetErrorString(e)), rc = XEVE_HIP_ERR_DEVICE;
    }
    template <typename T = char> T *alloc(size_t bytes)
    {
        void *p = nullptr;
        if(ok() && n == 12) xh_set_error("%s: too many device blocks", form), rc = XEVE_HIP_ERR_DEVICE;
        if(ok()) check(hipMalloc(&p, bytes ? bytes : 1), "device allocation");
        if(ok()) blk[n++] = p;
        return (T *)p;
    }
    template <typename T = char> T *stage(const void *host, size_t bytes) // a block holding host[0 .. bytes)
    {
        T *p = alloc<T>(bytes);
        up(p, host, bytes);
        return p;
    }
    void up(void *dev, const void *host, size_t bytes) { if(ok()) check(hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice), "copy to the device"); }
    void down(void *host, const void *dev, size_t bytes) { if(ok()) check(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost), "copy from the device"); }
    void copy2d(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t rows, hipMemcpyKind kind)
    {
        if(ok()) check(hipMemcpy2D(dst, dpitch, src, spitch, width, rows, kind), kind == hipMemcpyHostToDevice ? "copy to the device" : "copy from the device");
    }
    void run(int status) { if(ok()) rc = status; } // a batched entry point's status (it has set the error text itself)
};
} // namespace

// ---- arithmetic the forms share -------------------------------------------------------------------------------------------------------------------------------------
// the planes of a picture in elements: an original plane (org), a reference plane with its padding (ref), and sample (0, 0)'s offset in the latter (ref0)
struct XhPlaneExtents {
    size_t org[3], ref[3], ref0[3];
    XhPlaneExtents(int s_org_l, int s_org_c, int s_ref_l, int s_ref_c, int pad_l, int pad_c, int pic_h, int hs)
    {
        for(int c = 0; c < 3; c++) {
            const size_t so = c ? s_org_c : s_org_l, sr = c ? s_ref_c : s_ref_l, pad = c ? pad_c : pad_l, h = c ? pic_h >> hs : pic_h;
            org[c] = so * h, ref[c] = sr * (h + 2 * pad), ref0[c] = pad * sr + pad;
        }
    }
};
// the device reference table [refi * 2 + list] of a slice whose pictures (host planes at sample (0, 0)) are resident copies, uploaded on first sight
static inline int xh_resident_reftab(xeve_hip_refpic *tab, const xeve_hip_refpic *refp, int num_refp0, int num_refp1, int ncomp, const XhPlaneExtents &E)
{
    memset(tab, 0, 2 * XEVE_HIP_MAX_REFP * sizeof(*tab));
    const int nr[2] = {num_refp0, num_refp1}; // (num_refp1 == 0: a P slice)
    for(int l = 0; l < 2; l++)
        for(int r = 0; r < nr[l]; r++) {
            const xeve_hip_refpic &e = refp[r * 2 + l];
            XH_REQUIRE(e.y && (ncomp == 1 || (e.u && e.v)));
            const xeve_hip_pel *hp[3] = {e.y, e.u, e.v};
            const pel *dp[3] = {nullptr, nullptr, nullptr};
            for(int c = 0; c < ncomp; c++) {
                const pel *d = (const pel *)xh_resident(hp[c] - E.ref0[c], E.ref[c] * sizeof(pel));
                if(!d) return XEVE_HIP_ERR_DEVICE;
                dp[c] = d + E.ref0[c];
            }
            xeve_hip_refpic &t = tab[r * 2 + l];
            t.y = dp[0], t.u = dp[1], t.v = dp[2], t.poc = e.poc;
        }
    if(!nr[1]) tab[0 * 2 + 1] = tab[0 * 2 + 0]; // (P slices never read list 1; keep the table addressable)
    return XEVE_HIP_OK;
}
// the window of 4x4 units a CU or CTU at (x, y) is analysed in: one unit to its left and above (none on the picture's edge), right_max x down_max units from its own
// first unit on, cut by the picture.  Wl x Hl units in all; the unit's own part inside the picture is cw units wide (own_max at most)
struct XhWindow {
    int x_scu, y_scu, lx, ly, nw, nh, Wl, Hl, cw;
    XhWindow(int x, int y, int right_max, int down_max, int own_max, int w_scu, int h_scu)
        : x_scu(x >> 2), y_scu(y >> 2), lx(x_scu > 0), ly(y_scu > 0), nw(std::min(right_max, w_scu - x_scu)), nh(std::min(down_max, h_scu - y_scu)), Wl(lx + nw), Hl(ly + nh),
          cw(std::min(own_max, w_scu - x_scu))
    {
    }
};
