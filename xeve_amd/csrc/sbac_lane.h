// xeve_amd/csrc/sbac_lane.h -- the arithmetic coder as ONE lane runs it on a whole coder record (xeve_hip_sbac), counting bits or writing bytes to a sink (the
// bitstream writer, eco_lane.h), with the small tables the writer's syntax needs.  Every field of XEVE_SBAC is kept exactly.  The fused walk's coder on LDS rows
// (walk.h), the branch-free count of sbac.hip and the one bin of tree.hip's split_cu_flag are forms of their own, each measured where it runs.
// Every function is __host__ __device__: tests/native builds them for the host so that `pytest -m "not gpu"` checks them bit for bit against the oracle without a
// GPU.
#pragma once
#include <stdint.h>
#include "../../include/xeve_hip.h"

// A translation unit may define XL (e.g. with always_inline) and XL_CTX (where the coder's context models live) before including this header: the bitstream
// writer's kernels (encode.hip) keep the models in LDS and the coder core in registers that way.  The defaults are the plain record.
#ifndef XL
#define XL __host__ __device__ static inline
#endif
#ifndef XL_CTX
#define XL_CTX(s, ci) (s).ctx[ci]
#endif
// XL_SINK(o): does this coder write bytes?  A writer-only translation unit defines it as true: a comparison of the sink's (private) address with null is one the
// compiler does not fold, and it keeps the sink's fields in scratch memory instead of registers.
#ifndef XL_SINK
#define XL_SINK(o) ((o) != nullptr)
#endif

namespace xl {
typedef xeve_hip_sbac Sbac;

// ---- tables ---------------------------------------------------------------------------------------------------------------------------------------------------
// zig-zag scans of xeve_tbl_scan (xeve_util.c:1301-1325)
XL int zigzag(int n, int p)
{
    static constexpr uint8_t z4[16] = {0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15};
    static constexpr uint8_t z8[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                            35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return n == 2 ? p : n == 4 ? z4[p] : z8[p];
}
// xeve_tbl_mpm (xeve_tbl.c:40-48): [left mode + 1 | 0][up mode + 1 | 0] -> rank of every mode
XL int mpm_rank(int l, int u, int m)
{
    static constexpr uint8_t t[36][5] = {{0, 2, 3, 1, 4}, {0, 2, 1, 3, 4}, {0, 2, 1, 3, 4}, {1, 2, 0, 3, 4}, {0, 2, 1, 3, 4}, {0, 1, 2, 3, 4}, {1, 0, 2, 3, 4}, {0, 1, 2, 3, 4}, {0, 1, 2, 3, 4},
                              {1, 2, 0, 3, 4}, {0, 1, 3, 2, 4}, {0, 2, 1, 4, 3}, {1, 0, 2, 3, 4}, {1, 0, 2, 3, 4}, {1, 0, 2, 3, 4}, {2, 0, 1, 3, 4}, {1, 0, 3, 2, 4}, {0, 1, 2, 4, 3},
                              {1, 0, 2, 3, 4}, {0, 2, 1, 3, 4}, {1, 0, 2, 3, 4}, {1, 2, 0, 3, 4}, {0, 1, 2, 3, 4}, {0, 2, 1, 4, 3}, {0, 1, 2, 3, 4}, {0, 3, 2, 1, 4}, {1, 0, 2, 3, 4},
                              {1, 2, 0, 3, 4}, {1, 2, 3, 0, 4}, {0, 2, 1, 4, 3}, {0, 1, 2, 3, 4}, {0, 1, 2, 4, 3}, {0, 1, 2, 4, 3}, {0, 2, 1, 4, 3}, {0, 1, 2, 3, 4}, {0, 1, 2, 4, 3}};
    return t[l * 6 + u][m];
}
// the coded and intra flags of a unit's map_scu word (MCU_GET_COD, MCU_GET_IF)
#define XL_COD(m) (((m) >> 31) & 1u)
#define XL_IF(m)  (((m) >> 15) & 1u)

// ---- the arithmetic coder in bit-count mode (xeve_eco.c:392-575, xeve_mode.c:39-55): every field of XEVE_SBAC kept exactly ---------------------------------------
// write mode (the bitstream writer's coder, is_bitcount clear): the bytes go to a sink instead of advancing the counter
struct Sink {
    uint8_t *p;
    int      cap, n;
};
XL void sb_byte(Sbac &s, unsigned b, Sink *o = nullptr)
{
    if(s.is_pending_byte) {
        if(s.pending_byte == 0) s.stacked_zero++;
        else if(XL_SINK(o)) {
            for(; s.stacked_zero; s.stacked_zero--) {
                if(o->n < o->cap) o->p[o->n] = 0;
                o->n++;
            }
            if(o->n < o->cap) o->p[o->n] = (uint8_t)s.pending_byte;
            o->n++;
        }
        else s.bitcounter += 8 * s.stacked_zero + 8, s.stacked_zero = 0;
    }
    s.pending_byte = b & 0xFF, s.is_pending_byte = 1;
}
XL void sb_shift(Sbac &s, Sink *o = nullptr)
{
    s.code <<= 1;
    if(--s.code_bits) return;
    const unsigned out = s.code >> 17;
    s.code &= (1u << 17) - 1;
    if(out < 0xFF) {
        for(; s.stacked_ff; s.stacked_ff--) sb_byte(s, 0xFF, o);
        sb_byte(s, out, o);
    }
    else if(out > 0xFF) {
        s.pending_byte++;
        for(; s.stacked_ff; s.stacked_ff--) sb_byte(s, 0, o);
        sb_byte(s, out, o);
    }
    else s.stacked_ff++;
    s.code_bits = 8;
}
// n sb_shift steps at once (a context-coded bin renormalises by 0 .. 5 bits, so at most one byte leaves): the code register reaches the byte boundary with the same
// value as bit by bit, the byte leaves there, the rest of the shift follows
XL void sb_shift_n(Sbac &s, int n, Sink *o = nullptr)
{
    while(n >= (int)s.code_bits) {
        n -= (int)s.code_bits;
        s.code <<= s.code_bits - 1, s.code_bits = 1;
        sb_shift(s, o); // the boundary step itself: byte out, code_bits = 8
    }
    s.code <<= n, s.code_bits -= n;
}
// one context-coded bin on a model the caller holds in a register (a run of bins on one model -- the tail of a unary symbol -- loads and stores it once)
XL void sb_bin_m(Sbac &s, unsigned &model, unsigned bin, Sink *o = nullptr)
{
    unsigned state = (model >> 1) & 511u, mps = model & 1;
    unsigned lps = (state * (s.range & 0xFFFFu)) >> 9; // (the masks change nothing -- 9-bit state, 16-bit range -- and let the device use its full-rate 24-bit multiply)
    if(lps < 437) lps = 437;
    s.bin_counter++;
    s.range -= lps;
    if((bin != 0) != (mps != 0)) {
        if(s.range >= lps) s.code += s.range, s.range = lps;
        state = state + ((512 - state + 16) >> 5);
        if(state > 256) mps = 1 - mps, state = 512 - state;
    }
    else state = state - ((state + 16) >> 5);
    model = (state << 1) + mps;
    if(s.range < 8192) { // (xeve_sbac_encode_bin's renormalisation loop, :559-575, in one step)
        const int n = __builtin_clz(s.range) - 18;
        s.range <<= n;
        sb_shift_n(s, n, o);
    }
}
XL void sb_bin(Sbac &s, int ci, unsigned bin, Sink *o = nullptr)
{
    unsigned model = XL_CTX(s, ci);
    sb_bin_m(s, model, bin, o);
    XL_CTX(s, ci) = (uint16_t)model;
}
XL void sb_bin_ep(Sbac &s, unsigned bin, Sink *o = nullptr)
{   // (the range loses its LSB, xeve_eco.c:455-472)
    s.bin_counter++;
    s.range >>= 1;
    if(bin) s.code += s.range;
    s.range <<= 1;
    sb_shift(s, o);
}
XL void sb_unary2(Sbac &s, unsigned sym, int ci, Sink *o = nullptr)
{   // sbac_write_unary_sym with two models (xeve_eco.c:474-490)
    sb_bin(s, ci, sym ? 1 : 0, o);
    if(!sym) return;
    unsigned model = XL_CTX(s, ci + 1);
    while(sym) {
        sym--;
        sb_bin_m(s, model, sym ? 1 : 0, o);
    }
    XL_CTX(s, ci + 1) = (uint16_t)model;
}
} // namespace xl
