// tests/native/md5_host.cpp -- xeve_amd/csrc/md5_core.h (what a lane of md5.hip runs) compiled for the host: a stand-alone program, built with the address and
// undefined-behaviour sanitizers by tests/test_md5_core_host.py and run as a child process.
// usage: md5_host FILE -- FILE holds (little-endian) int64 njobs, int64 nsamples, njobs records of xeve_hip_md5_job (int64 offset; int32 stride, w, h, reserved), then
// nsamples 16-bit samples.  The samples are copied into a heap block of exactly their size -- a read outside what a job describes is a sanitizer report -- and every
// job's digest is printed as one line of hex.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../xeve_amd/csrc/md5_core.h"

struct Job {
    int64_t offset;
    int32_t stride, w, h, reserved;
};
static_assert(sizeof(Job) == 24, "xeve_hip_md5_job");

int main(int argc, char **argv)
{
    if(argc != 2) return fprintf(stderr, "usage: md5_host FILE\n"), 2;
    FILE *f = fopen(argv[1], "rb");
    if(!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
    int64_t head[2];
    if(fread(head, sizeof(head), 1, f) != 1 || head[0] < 0 || head[1] < 0) return fprintf(stderr, "bad header\n"), 2;
    std::vector<Job> jobs((size_t)head[0]);
    if(head[0] && fread(jobs.data(), sizeof(Job), jobs.size(), f) != jobs.size()) return fprintf(stderr, "short job list\n"), 2;
    uint16_t *samples = static_cast<uint16_t *>(malloc((size_t)head[1] * 2 + 1)); // (+ 1: never a zero-sized block)
    if(!samples || (head[1] && fread(samples, 2, (size_t)head[1], f) != (size_t)head[1])) return fprintf(stderr, "short sample list\n"), 2;
    fclose(f);
    for(const Job &j : jobs) {
        if(j.w < 1 || j.h < 1 || j.stride < j.w || j.offset < 0 || j.offset + (int64_t)(j.h - 1) * j.stride + j.w > head[1]) return fprintf(stderr, "a job outside the samples\n"), 2;
        uint8_t d[16];
        xmd5::digest_plane(samples + j.offset, j.stride, j.w, j.h, d);
        for(int k = 0; k < 16; k++) printf("%02x", d[k]);
        printf("\n");
    }
    free(samples);
    return 0;
}
