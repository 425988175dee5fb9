// xeve_amd/csrc/eco_wave.h -- how the writer kernels (encode.hip, eco.hip) hold eco_lane.h's coder: ONE CHAIN PER WAVE of 64 lanes, the 72 context models in LDS
// ([model][lane]: no bank conflicts, no scratch) and, every lane function forced inline, the coder core (range, code, pending bytes) and the byte sink in registers
// (sbac_lane.h: XL, XL_CTX, XL_SINK).  The lane-serial form with the whole record in scratch (round 2: 13 ms per CTU of noise for one chain, 346 ms per step for 2048
// chains) was bound by the scratch round trip of every bin's model.  Include it once per translation unit, before any other use of the lane headers.
#pragma once
#include "xh_common.h"
#define XL_NCTX 72
static __shared__ uint16_t xl_lds_ctx[XL_NCTX * 64];
#if defined(__HIP_DEVICE_COMPILE__)
#define XL __host__ __device__ static inline __attribute__((always_inline))
#define XL_CTX(s, ci) xl_lds_ctx[(ci) * 64 + (threadIdx.x & 63)]
#define XL_SINK(o) true // (every coder of a writer's translation unit writes: see sbac_lane.h)
#endif
#include "eco_lane.h"
static_assert(sizeof(((xeve_hip_sbac *)0)->ctx) == XL_NCTX * sizeof(uint16_t), "the models' LDS image");
// a coder record in: the core into the lane's registers, the models into the lane's LDS column; and out again
__device__ static __forceinline__ void sbac_in(xl::Sbac &s, const xeve_hip_sbac *__restrict__ g)
{
    s = *g;
#pragma unroll
    for(int i = 0; i < XL_NCTX; i++) xl_lds_ctx[i * 64 + (threadIdx.x & 63)] = s.ctx[i];
}
__device__ static __forceinline__ void sbac_out(xeve_hip_sbac *__restrict__ g, xl::Sbac &s)
{
#pragma unroll
    for(int i = 0; i < XL_NCTX; i++) s.ctx[i] = xl_lds_ctx[i * 64 + (threadIdx.x & 63)];
    *g = s;
}
