// tests/native/scale_host.cpp -- xeve_amd/csrc/scale_core.h (the per-lane code of scale.hip: the sample, the two passes, and the host's exact tables with their bounds)
// compiled for the HOST and run over whole surfaces.  tests/test_scale_host.py builds this with the address and undefined-behaviour sanitizers and compares its output
// with the numpy / Fraction restatement (tests/_scale.py).  Every plane is a heap block of exactly (rows - 1) * pitch + the row's bytes, so a tap that is not clamped or a
// read behind the last row's end is a report.
//   scale_host <jobs file> <output file>
// jobs file: int64 count, then per job 13 x int64 { layout (0 planar, 1 semi-planar), sample_bytes, depth, shift, siting, sw, sh, w, h, pitch_l, pitch_c, luma bytes, bytes
// of a chroma block } followed by the luma block and the chroma block(s) (planar: U, then V).  Output per job: the frame's samples (uint8 at depth 8, uint16 at 10), Y, U, V.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../xeve_amd/csrc/scale_core.h"

using namespace xscl;

int main(int argc, char **argv)
{
    if(argc != 3) return 2;
    FILE   *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    int64_t n = 0;
    if(!f || !o || fread(&n, 8, 1, f) != 1) return 2;
    for(int64_t k = 0; k < n; k++) {
        int64_t j[13];
        if(fread(j, 8, 13, f) != 13) return 3;
        const int    semi = (int)j[0], sb = (int)j[1], depth = (int)j[2], shift = (int)j[3], siting = (int)j[4], sw = (int)j[5], sh = (int)j[6], w = (int)j[7], h = (int)j[8];
        const size_t nl = (size_t)j[11], nc = (size_t)j[12];
        if(nl != (size_t)(sh - 1) * j[9] + (size_t)sw * sb || nc != (size_t)(sh / 2 - 1) * j[10] + (size_t)(sw / 2) * sb * (semi ? 2 : 1)) return 4; // (exactly the described bytes)
        uint8_t *luma = static_cast<uint8_t *>(malloc(nl)), *cb = static_cast<uint8_t *>(malloc(nc)), *cr = semi ? nullptr : static_cast<uint8_t *>(malloc(nc));
        if(!luma || !cb || fread(luma, 1, nl, f) != nl || fread(cb, 1, nc, f) != nc || (cr && fread(cr, 1, nc, f) != nc)) return 3;
        Axis hl, vl, hc, vc;
        if(!filter(sw, w, KIND_PLAIN, hl) || !filter(sh, h, KIND_PLAIN, vl) || !filter(sh / 2, h / 2, KIND_PLAIN, vc)) return 5;
        if(!(siting == 0 ? filter(sw, w, KIND_LEFT, hc) : filter(sw / 2, w / 2, KIND_PLAIN, hc))) return 5;
        if(!bounds_ok(hl.sum_abs, vl.sum_abs, depth) || !bounds_ok(hc.sum_abs, vc.sum_abs, depth)) return 6;
        const size_t sl = (size_t)w * h, sc = sl / 4;
        uint16_t    *out = static_cast<uint16_t *>(malloc((sl + 2 * sc) * 2));
        if(!out) return 3;
        scale_plane(luma, sb, 1, 0, j[9], shift, depth, hl, vl, out);
        scale_plane(cb, sb, semi ? 2 : 1, 0, j[10], shift, depth, hc, vc, out + sl);
        scale_plane(semi ? cb : cr, sb, semi ? 2 : 1, semi ? 1 : 0, j[10], shift, depth, hc, vc, out + sl + sc);
        for(size_t i = 0; i < sl + 2 * sc; i++) {
            if(depth == 8) {
                const uint8_t v = (uint8_t)out[i];
                if(fwrite(&v, 1, 1, o) != 1) return 7;
            }
            else if(fwrite(&out[i], 2, 1, o) != 1) return 7;
        }
        free(luma), free(cb), free(cr), free(out);
    }
    fclose(f);
    return fclose(o) == 0 ? 0 : 7;
}
