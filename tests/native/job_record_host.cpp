// tests/native/job_record_host.cpp -- TEST INFRASTRUCTURE: the job-record makers and decoders of xeve_amd/csrc/xh_common.h (xh_make_job / xh_job, xh_make_pred_off /
// xh_pred_off, xh_u, and the guards xh_job_ok / xh_dense_ok the host entry points require) compiled for the host -- they are __host__ __device__, every consumer kernel
// decodes through them -- so that the CPU suite can walk the edges of their domain (2^31, 2^32, 2^33 samples, bit 30 of off2) without a GPU.  Nothing of this is linked
// into the product library.
#include "../../xeve_amd/csrc/xh_common.h"

extern "C" {
void jr_make_job(uint64_t o, int32_t off2, int32_t *rec)
{
    const xeve_hip_job j = xh_make_job((size_t)o, off2);
    rec[0] = j.off1, rec[1] = j.off2;
}
// the (y, stride, x) form the kernels call
void jr_make_job_yx(int64_t y, int64_t stride, int64_t x, int32_t off2, int32_t *rec)
{
    const xeve_hip_job j = xh_make_job((long)y, (long)stride, (long)x, off2);
    rec[0] = j.off1, rec[1] = j.off2;
}
void jr_job(int32_t off1, int32_t off2, uint64_t *o, int32_t *o2)
{
    xeve_hip_job j;
    j.off1 = off1, j.off2 = off2;
    const XhJob r = xh_job(j);
    *o = (uint64_t)xh_u(r.off1), *o2 = r.off2;
}
uint64_t jr_u(int32_t off) { return (uint64_t)xh_u(off); }
int      jr_job_ok(uint64_t o, int32_t off2) { return xh_job_ok((size_t)o, off2); }
int      jr_dense_ok(int64_t nblocks, int64_t n) { return xh_dense_ok((long)nblocks, (long)n); }
void     jr_make_pred_off(uint64_t o, int32_t *rec)
{
    const XhPredOff r = xh_make_pred_off((size_t)o);
    rec[0] = r.pred_off, rec[1] = r.frac;
}
uint64_t jr_pred_off(int32_t pred_off, int32_t frac) { return (uint64_t)xh_pred_off(pred_off, frac); }
int      jr_off2_half() { return XH_OFF2_HALF; }
int      jr_frac_half() { return XH_FRAC_HALF; }
int      jr_frac_off() { return XH_FRAC_OFF; }
}
