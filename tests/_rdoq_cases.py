"""Seeded RDOQ cases: transformed residual blocks + plausible CABAC bit-estimate tables (entropy_bits values,
xeve_mode.c:304-325: -32768 * (log2(p) - 9) for a 9-bit probability state)."""
import math

import numpy as np

from _libs import RdoqEst, oracle, ptr


def entropy_bits(state):  # xeve_init_bits_est, i = state << 1
    p = (512 * ((state << 1) + 0.5)) / 1024
    return int(-32768 * (math.log(p) / math.log(2.0) - 9))


def make_est(r):
    e = RdoqEst()

    def pair():
        st = int(r.integers(1, 511))  # probability state of the context model
        return entropy_bits(st), entropy_bits(512 - st)

    e.cbf[0], e.cbf[1] = pair()
    for i in range(24):
        e.run[i][0], e.run[i][1] = pair()
        e.level[i][0], e.level[i][1] = pair()
    for i in range(2):
        e.last[i][0], e.last[i][1] = pair()
    return e


def make_coef(r, lw, lh, bd, kind):
    """forward-transformed residual of a plausible prediction error (through the oracle's DCT)"""
    n = 1 << (lw + lh)
    if kind == 0:
        resid = r.integers(-(1 << bd) + 1, 1 << bd, size=n)
    elif kind == 1:
        resid = r.integers(-40, 41, size=n)
    elif kind == 2:
        resid = r.integers(-6, 7, size=n)
    else:
        resid = np.zeros(n, np.int64)
        resid[r.integers(0, n, size=max(1, n // 16))] = r.integers(-300, 301, size=max(1, n // 16))
    c = resid.astype(np.int16)
    oracle().xo_trans(ptr(c), lw, lh, bd)
    return c


# ---- the 16-bit wrap zone -------------------------------------------------------------------------------------------------------------------------------------------
# The reference stores quantised levels through plain (s16) casts (xeve_tq.c:34, 558, 608, 723-724): a level above 32767 wraps, changes sign and magnitude, and flows on
# into the rate, the decision and the output.  level = |coef| * q_value >> q_bits with q_bits = 14 + (15 - bit_depth - log2_size) + qp / 6: at 10 bits a full-scale
# coefficient passes 32767 on 32-point blocks at QP 0 .. 3 and on 64-point blocks at QP 0 .. 9.
QUANT_SCALE = (26214, 23302, 20560, 18396, 16384, 14764)  # xeve_quant_scale[0] (tool_iqt off)
SATURATED_SIZES = [(1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (6, 6), (3, 4), (4, 5), (6, 5), (2, 6)]  # the sizes of test_hip_rdoq_batches_vs_oracle
SATURATED_GOLDEN_QPS = (1, 3, 4, 9)
S32_MAX = 2 ** 31 - 1


def quant_numbers(lw, lh, qp, bd):
    odd = (lw + lh) & 1
    q_value = (QUANT_SCALE[qp % 6] * 181 + 64) >> 7 if odd else QUANT_SCALE[qp % 6]
    return q_value, 14 + (15 - bd - ((lw + lh) >> 1)) + qp // 6


def unwrapped_levels(coef, lw, lh, qp, bd):
    """the level of every coefficient BEFORE the (s16) cast (xeve_rdoq_run_length_cc's max_abs_level, xeve_tq.c:540-558)"""
    q_value, q_bits = quant_numbers(lw, lh, qp, bd)
    ld = np.minimum(np.abs(coef.astype(np.int64)) * q_value, S32_MAX - (1 << (q_bits - 1)))
    return (ld + (1 << (q_bits - 1))) >> q_bits


def coef_for_level(level, lw, lh, qp, bd):
    """the smallest coefficient whose unwrapped level is at least `level`, or 32767 where no 16-bit coefficient gets there"""
    q_value, q_bits = quant_numbers(lw, lh, qp, bd)
    v = min(32767, max(1, ((level << q_bits) - (1 << (q_bits - 1)) + q_value - 1) // q_value))
    assert v == 32767 or (int(unwrapped_levels(np.array([v]), lw, lh, qp, bd)[0]) >= level > int(unwrapped_levels(np.array([v - 1]), lw, lh, qp, bd)[0]))
    return v


def saturated_blocks(r, lw, lh, qp, bd):
    """nine blocks: the transforms of a full-scale flat residual +-(2^bd - 1) in both signs and as a half-and-half step, of a full-scale one-sample checkerboard and of
    full-scale stripes in both directions; a DC coefficient whose level lands exactly on 32767, one on 32768 and one beyond 65535 (each over light noise in the
    other coefficients; where no 16-bit coefficient reaches the level, the largest one)"""
    w, h, full = 1 << lw, 1 << lh, (1 << bd) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for resid in (np.full((h, w), full), np.full((h, w), -full), np.where(xx < w // 2, full, -full), np.where((xx + yy) & 1, full, -full), np.where(xx & 1, full, -full),
                  np.where(yy & 1, -full, full)):
        c = resid.astype(np.int16).reshape(-1).copy()
        oracle().xo_trans(ptr(c), lw, lh, bd)
        out.append(c)
    for k, level in enumerate((32767, 32768, 65536 + 1000)):
        c = make_coef(r, lw, lh, bd, 2)
        c[0] = coef_for_level(level, lw, lh, qp, bd) * (-1 if k == 1 else 1)
        out.append(c)
    return np.stack(out)


def rate_bound(levels):
    """the largest continue-bin estimate level[.][1] under which the s32 rate of the largest level the search visits stays below 2^31, whatever the other estimates
    (each at most entropy_bits(1) < 300 000)"""
    visited = int(np.abs(levels.astype(np.int16).astype(np.int64)).max())  # (the search visits the WRAPPED magnitude and the one below it)
    return S32_MAX if visited <= 2 else (S32_MAX - 32768 - 3 * 300000) // (visited - 2)


def cap_est(est, levels):
    """caps the continue-bin estimates of `est` in place (rate_bound) and asserts the s32 condition for every context pair"""
    visited, bound = int(np.abs(levels.astype(np.int16).astype(np.int64)).max()), rate_bound(levels)
    fixed = 32768 + max(est.run[i][0] for i in range(24))
    for c in range(24):
        est.level[c][1] = min(est.level[c][1], bound)
    for c in range(23):
        assert fixed + est.level[c][1] + est.level[c + 1][1] * max(0, visited - 2) + est.level[c + 1][0] <= S32_MAX, (visited, c)


def saturated_case(lw, lh, qp, bd):
    """-> (blocks, estimate tables, lambda, is_luma, unwrapped levels): the reference's rate is an s32 (get_rate_positionLastXY / the level's rate in
    xeve_rdoq_run_length_cc): the continue-bin estimates level[.][1] are capped so that the rate of the largest level the search visits stays below 2^31 -- beyond that
    the reference's result is signed overflow and no target"""
    r = np.random.default_rng(9000 + ((lw * 8 + lh) * 64 + qp) * 2 + (bd == 10))
    blocks = saturated_blocks(r, lw, lh, qp, bd)
    est = make_est(r)
    levels = unwrapped_levels(blocks, lw, lh, qp, bd)
    cap_est(est, levels)
    lam = 0.57 * 2.0 ** ((qp - 12) / 3.0)  # the luma lambda of slice QP qp (set_lambda, xeve_mode.c:660-679)
    return blocks, est, lam, int(r.integers(0, 2)), levels


def wraps_expected(lw, lh, qp, bd):
    """does a 16-bit coefficient reach a level above 32767 at this size, QP and bit depth?"""
    return int(unwrapped_levels(np.array([32767]), lw, lh, qp, bd)[0]) > 32767


def plain_levels(coef, lw, lh, qp, bd, intra_slice):
    """the plain quantiser's level of every coefficient BEFORE its (s16) cast (xeve_quant_nnz without RDOQ, xeve_tq.c:704-727)"""
    shift = 14 + (15 - bd - ((lw + lh) >> 1)) + qp // 6
    return (np.abs(coef.astype(np.int64)) * QUANT_SCALE[qp % 6] + ((171 if intra_slice else 85) << (shift - 9))) >> shift


_residual_memo = {}


def saturated_residuals(lw, lh, qp, bd):
    """nine RESIDUAL blocks (the leaf chains start at the difference): full-scale flat +-(2^bd - 1), the half-and-half step, the one-sample checkerboard, stripes in both
    directions, and three flat residuals whose amplitude is solved so that the plain quantiser's DC level is the first at or above 32767, 32768 and 65536 (the largest
    amplitude where none gets there).  Built once per (size, QP, depth), shared, read-only."""
    key = (lw, lh, qp, bd)
    if key not in _residual_memo:
        w, h, full = 1 << lw, 1 << lh, (1 << bd) - 1
        yy, xx = np.mgrid[0:h, 0:w]
        out = [np.full((h, w), full), np.full((h, w), -full), np.where(xx < w // 2, full, -full), np.where((xx + yy) & 1, full, -full), np.where(xx & 1, full, -full),
               np.where(yy & 1, -full, full)]

        def dc_level(a):
            c = np.full(w * h, a, np.int16)
            oracle().xo_trans(ptr(c), lw, lh, bd)
            return int(plain_levels(c[:1], lw, lh, qp, bd, 0)[0])

        for k, level in enumerate((32767, 32768, 65536)):
            lo, hi = 1, full  # the smallest amplitude whose DC level reaches `level` (the level grows with the amplitude)
            while lo < hi:
                mid = (lo + hi) // 2
                lo, hi = (lo, mid) if dc_level(mid) >= level else (mid + 1, hi)
            out.append(np.full((h, w), -lo if k == 1 else lo))
        a = np.stack([o.astype(np.int16).reshape(-1) for o in out])
        a.setflags(write=False)
        _residual_memo[key] = a
    return _residual_memo[key]


def plain_wraps_expected(lw, lh, qp, bd):
    """does a full-scale flat residual give the plain quantiser a level above 32767 at this size, QP and bit depth?"""
    c = saturated_residuals(lw, lh, qp, bd)[0].copy()
    oracle().xo_trans(ptr(c), lw, lh, bd)
    return int(plain_levels(c, lw, lh, qp, bd, 0).max()) > 32767


def wrapped_outputs(blocks, levels, out):
    """how many RDOQ outputs ARE a wrapped level: positions whose unwrapped level is above 32767 and whose nonzero output is the (s16) value of +-level -- the sign the
    reference's tmp_coef carries after its cast -- or that value one step towards zero (the two candidates of get_coded_level_rl); -32768, the level 32768, counts"""
    def s16(a):
        return ((a + 32768) % 65536) - 32768

    lv, o = levels.astype(np.int64), out.astype(np.int64)
    w = s16(np.where(blocks > 0, s16(lv), -s16(lv)))
    lower = np.where(w < 0, w + 1, w - 1)
    return int(((lv > 32767) & (o != 0) & ((o == w) | (o == s16(lower)))).sum())
