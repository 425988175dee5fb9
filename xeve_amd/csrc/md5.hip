// xeve_amd/csrc/md5.hip -- the decoded-picture signatures of the application's --hash (xeve_md5_imgb, src_base/xeve_util.c:1067-1083) on the device: one MD5 per plane
// over the plane's interior as the -r file holds it.  md5_core.h is the lane's code.
//
// MD5 is a serial chain: 64 dependent steps per 64-byte block, block after block.  Nothing inside a message runs in parallel, so the parallel axis is the MESSAGES -- a lane
// each, 64 messages per wave, ONE launch for all of them (a picture end of G GOPs: 3 * G).  The lanes of a wave run in step as long as their messages have the same
// shape, and a wave is as slow as its longest lane: callers list messages of one length next to each other (the encoder: every luma plane, then every chroma plane), so
// only the wave at a boundary mixes lengths.  State, message words and the block read ahead live in registers; no LDS, no workspace.  Each lane reads whole 64-byte lines
// of its own plane (four 16-byte loads where the row allows); the lanes' lines are far apart, which costs nothing here -- the 64 steps between two loads are the time.
#include "xh_common.h"
#include "md5_core.h"

static_assert(sizeof(xeve_hip_md5_job) == 24 && offsetof(xeve_hip_md5_job, stride) == 8 && offsetof(xeve_hip_md5_job, h) == 16, "xeve_hip_md5_job: the layout xeve_amd/lib.py binds");

namespace {
__global__ void __launch_bounds__(XH_WAVE) k_md5_planes(const uint16_t *__restrict__ base, const xeve_hip_md5_job *__restrict__ jobs, int njobs, uint8_t *__restrict__ digests)
{
    const int j = blockIdx.x * XH_WAVE + threadIdx.x;
    if(j >= njobs) return;
    const xeve_hip_md5_job J = jobs[j];
    uint8_t d[16] = {0};
    if(J.w >= 1 && J.h >= 1) xmd5::digest_plane(base + J.offset, J.stride, J.w, J.h, d); // (an empty job reads nothing: sixteen zero bytes)
    for(int k = 0; k < 16; k++) digests[(size_t)j * 16 + k] = d[k]; // (byte stores: `digests` may lie anywhere)
}
} // namespace

extern "C" int xeve_hip_md5_planes(const uint16_t *base, const xeve_hip_md5_job *jobs, int njobs, uint8_t *digests, void *stream)
{
    XH_ENTER();
    XH_REQUIRE(base && jobs && digests && njobs >= 1 && njobs <= (1 << 24));
    XH_REQUIRE((reinterpret_cast<uintptr_t>(base) & 1) == 0 && (reinterpret_cast<uintptr_t>(jobs) & 7) == 0);
    k_md5_planes<<<(unsigned)((njobs + XH_WAVE - 1) / XH_WAVE), XH_WAVE, 0, static_cast<hipStream_t>(stream)>>>(base, jobs, njobs, digests);
    XH_HIP(hipGetLastError());
    return XEVE_HIP_OK;
}
