// tests/native/color_host.cpp -- xeve_amd/csrc/color_core.h (the per-lane code of color.hip: c16, the block functions, the output conversions, and the host's exact
// coefficients) compiled for the HOST and run over whole pictures.  tests/test_color_host.py builds this with the address and undefined-behaviour sanitizers and compares
// its output with the numpy / Fraction restatement (tests/_color.py).  Every buffer is a heap block of exactly its size, so a tap that is not clamped is a report.
//   color_host <jobs file> <output file>
// jobs file: int64 count, then per job 12 x int64 { direction (0 RGB -> YUV, 1 YUV -> RGB), dtype, siting, matrix, full_range, depth, w, h, stride_x, stride_y, stride_c,
// rgb elements } followed by the job's input (the RGB elements, or w * h * 3 / 2 uint16 samples).  Output per job: the frame's samples (uint8 at depth 8, uint16 at 10), or
// the whole RGB block (filled with 0xA5 bytes before the conversion).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../xeve_amd/csrc/color_core.h"

using namespace xcol;

static int elem_bytes(int dt) { return dt == DT_U8 ? 1 : dt == DT_F32 ? 4 : 2; }

template <int DT, int SIT> static void fwd(const Fwd &F, int depth, const void *rgb, const int64_t *j, void *yuv)
{
    if(depth == 8) forward_picture<DT, SIT, uint8_t>(F, rgb, j[8], j[9], j[10], (int)j[6], (int)j[7], static_cast<uint8_t *>(yuv));
    else forward_picture<DT, SIT, uint16_t>(F, rgb, j[8], j[9], j[10], (int)j[6], (int)j[7], static_cast<uint16_t *>(yuv));
}
template <int DT> static void run(const Fwd &F, const Inv &I, const int64_t *j, const void *in, void *out)
{
    const int sit = (int)j[2], w = (int)j[6], h = (int)j[7];
    if(j[0] == 0) {
        if(sit == SIT_LEFT) fwd<DT, SIT_LEFT>(F, (int)j[5], in, j, out);
        else fwd<DT, SIT_CENTRE>(F, (int)j[5], in, j, out);
    }
    else if(sit == SIT_LEFT) inverse_picture<DT, SIT_LEFT>(I, static_cast<const uint16_t *>(in), w, h, out, j[8], j[9], j[10]);
    else inverse_picture<DT, SIT_CENTRE>(I, static_cast<const uint16_t *>(in), w, h, out, j[8], j[9], j[10]);
}

int main(int argc, char **argv)
{
    if(argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    int64_t n = 0;
    if(!f || !o || fread(&n, 8, 1, f) != 1) return 2;
    for(int64_t k = 0; k < n; k++) {
        int64_t j[12];
        if(fread(j, 8, 12, f) != 12) return 3;
        const int    dt = (int)j[1], w = (int)j[6], h = (int)j[7];
        const size_t rgb_bytes = (size_t)j[11] * elem_bytes(dt), yuv_in = (size_t)w * h * 3, yuv_out = (size_t)w * h * 3 / 2 * (j[5] > 8 ? 2 : 1);
        const size_t in_bytes = j[0] == 0 ? rgb_bytes : yuv_in, out_bytes = j[0] == 0 ? yuv_out : rgb_bytes;
        void *in = malloc(in_bytes), *out = malloc(out_bytes);
        if(!in || !out || fread(in, 1, in_bytes, f) != in_bytes) return 3;
        memset(out, 0xA5, out_bytes);
        Fwd F;
        Inv I;
        if(!matrix((int)j[3], (int)j[4], (int)j[5], F, I)) return 4;
        switch(dt) {
        case DT_U8: run<DT_U8>(F, I, j, in, out); break;
        case DT_F16: run<DT_F16>(F, I, j, in, out); break;
        case DT_BF16: run<DT_BF16>(F, I, j, in, out); break;
        case DT_F32: run<DT_F32>(F, I, j, in, out); break;
        default: return 4;
        }
        if(fwrite(out, 1, out_bytes, o) != out_bytes) return 5;
        free(in), free(out);
    }
    fclose(f);
    return fclose(o) == 0 ? 0 : 5;
}
