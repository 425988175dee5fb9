"""The restatement of the surface scaler's definition (include/xeve_hip.h, "DECODER SURFACES IN"): the tables of an axis in fractions.Fraction, the two passes in numpy
int64.  Nothing here is shared with the library -- tests/test_scale_host.py holds xeve_hip_scale_filter and scale_core.h to it on the CPU, tests/test_scale_gpu.py the
kernel, tests/test_enc_surface_gpu.py the encoder's end."""
import functools
from fractions import Fraction

import numpy as np

CBITS = 14
SITINGS = ("left", "centre")


def rnd(q):
    """round half away from zero of an exact rational"""
    n, d = (q.numerator, q.denominator)
    r = (2 * abs(n) + d) // (2 * d)
    return -r if n < 0 else r


def weight(t):
    a = abs(t)
    if a <= 1:
        return (3 * a ** 3 - 5 * a ** 2 + 2) / 2
    if a < 2:
        return (-a ** 3 + 5 * a ** 2 - 8 * a + 4) / 2
    return Fraction(0)


def centre(i, src_n, dst_n, kind):
    if kind == 1:
        return Fraction((4 * i + 1) * src_n - dst_n, 4 * dst_n)
    return Fraction((2 * i + 1) * src_n - dst_n, 2 * dst_n)


@functools.lru_cache(maxsize=None)
def table(src_n, dst_n, kind=0):
    """(first[rows], coef[rows][ntaps], ntaps) of one axis as xeve_hip_scale_filter hands it out: kind 0 -- src_n -> dst_n samples of a plane; kind 1 -- the left-sited
    chroma columns of a picture src_n -> dst_n luma samples wide.  Rows shorter than the longest end in zeros"""
    rows = dst_n // 2 if kind == 1 else dst_n
    stretch = min(Fraction(1), Fraction(dst_n, src_n))
    firsts, coefs = [], []
    for i in range(rows):
        p = centre(i, src_n, dst_n, kind)
        # the integers k with |(k - p) * stretch| < 2
        lo, hi = p - 2 / stretch, p + 2 / stretch
        k0 = lo.numerator // lo.denominator + 1
        k1 = -((-hi.numerator) // hi.denominator) - 1
        ks = list(range(k0, k1 + 1))
        assert all(abs((k - p) * stretch) < 2 for k in ks) and abs((k0 - 1 - p) * stretch) >= 2 and abs((k1 + 1 - p) * stretch) >= 2
        w = [weight((k - p) * stretch) for k in ks]
        total = sum(w)
        c = [rnd((1 << CBITS) * x / total) for x in w]
        c[w.index(max(w))] += (1 << CBITS) - sum(c)  # (index: the lowest k among equals)
        firsts.append(k0)
        coefs.append(c)
    ntaps = max(len(c) for c in coefs)
    coef = np.zeros((rows, ntaps), np.int64)
    for i, c in enumerate(coefs):
        coef[i, :len(c)] = c
    return np.array(firsts, np.int64), coef, ntaps


def resample(plane, h_table, v_table, depth, clamp=True):
    """a plane of samples (2-d, any integer type) through the two passes; clamp=False: the vertical sums' values before the clamp"""
    src = plane.astype(np.int64)
    sh, sw = src.shape
    hf, hc, _ = h_table
    vf, vc, _ = v_table
    idx = np.clip(hf[:, None] + np.arange(hc.shape[1])[None, :], 0, sw - 1)  # [dw][taps]
    t = ((src[:, idx] * hc[None, :, :]).sum(axis=2) + (1 << 9)) >> 10  # [sh][dw]
    idy = np.clip(vf[:, None] + np.arange(vc.shape[1])[None, :], 0, sh - 1)  # [dh][taps]
    out = ((t[idy, :] * vc[:, :, None]).sum(axis=1) + (1 << 17)) >> 18  # [dh][dw]
    return np.clip(out, 0, (1 << depth) - 1) if clamp else out


def tables(sw, sh, w, h, siting):
    """((luma columns, luma rows), (chroma columns, chroma rows)) for a picture sw x sh -> w x h"""
    hc = table(sw, w, 1) if siting == "left" else table(sw // 2, w // 2, 0)
    return (table(sw, w, 0), table(sh, h, 0)), (hc, table(sh // 2, h // 2, 0))


def scale_planes(y, u, v, w, h, siting, depth, clamp=True):
    """three planes of SAMPLES (the containers already shifted) -> the three planes of the w x h frame"""
    sh, sw = y.shape
    luma, chroma = tables(sw, sh, w, h, siting)
    return resample(y, *luma, depth, clamp), resample(u, *chroma, depth, clamp), resample(v, *chroma, depth, clamp)


def frame(y, u, v, w, h, siting, depth):
    """the frame xeve_hip_enc_push takes: Y, U, V without padding; uint8 at depth 8, little-endian uint16 at depth 10"""
    planes = scale_planes(y, u, v, w, h, siting, depth)
    return np.concatenate([p.reshape(-1) for p in planes]).astype(np.uint8 if depth == 8 else "<u2")


# ---- surfaces for the tests: samples -> containers -> pitched planes ---------------------------------------------------------------------------------------------------
FORMATS = {"u8": (1, 8, 0), "lo10": (2, 10, 0), "msb10": (2, 10, 6)}  # name -> (bytes per container, depth, shift)
CONTENTS = ("random", "max", "checker")


def content(rng, kind, sh, sw, depth):
    """three planes of samples: random, all-maximum, a one-sample checkerboard of 0 and the maximum, or ("blocks") two-sample squares of them -- plateaus next to an edge,
    what a cubic overshoots at both ends of the range even when shrinking"""
    top = (1 << depth) - 1

    def plane(h, w):
        if kind == "random":
            return rng.integers(0, top + 1, size=(h, w), dtype=np.int64)
        if kind == "max":
            return np.full((h, w), top, np.int64)
        yy, xx = np.mgrid[0:h, 0:w]
        return ((yy + xx) & 1) * top if kind == "checker" else ((yy // 2 + xx // 2) & 1) * top

    return plane(sh, sw), plane(sh // 2, sw // 2), plane(sh // 2, sw // 2)


def containers(plane, fmt, rng):
    """samples as the format's containers, with noise in every bit of a word that is not the sample's: below it in an msb-aligned word (the shift drops them), above it in
    a low-aligned one (the definition's mask drops them: a sample is (container >> shift) & (2^d - 1))"""
    sb, depth, shift = FORMATS[fmt]
    c = plane.astype(np.int64) << shift
    if shift:
        c |= rng.integers(0, 1 << shift, size=plane.shape, dtype=np.int64)
    elif 8 * sb > depth:
        c |= rng.integers(0, 1 << (8 * sb - depth), size=plane.shape, dtype=np.int64) << depth
    return c.astype(np.uint8 if sb == 1 else "<u2")


def pitched(rows, pitch, poison):
    """rows (2-d containers) `pitch` containers apart in a flat block of exactly (rows - 1) * pitch + the row's length, the gaps poisoned"""
    h, w = rows.shape
    assert pitch >= w
    buf = np.full((h - 1) * pitch + w, poison, rows.dtype)
    np.lib.stride_tricks.as_strided(buf, (h, w), (pitch * buf.itemsize, buf.itemsize))[:] = rows
    return buf


def surface(rng, sw, sh, layout, fmt, kind="random", extra=0, poison=None):
    """(the sample planes y, u, v; the flat blocks: [luma, uv] for layout "nv" or [luma, u, v] for "planar"; luma pitch; chroma pitch -- in containers).  extra: containers
    between a row's end and the next row (luma; chroma gets extra + 1 pairs or samples)"""
    sb, depth, _ = FORMATS[fmt]
    poison = (0xA5 if sb == 1 else 0xA5A5) if poison is None else poison
    y, u, v = content(rng, kind, sh, sw, depth)
    cy, cu, cv = (containers(p, fmt, rng) for p in (y, u, v))
    pl = sw + extra
    if layout == "nv":
        uv = np.stack([cu, cv], axis=2).reshape(sh // 2, sw)
        pc = sw + (2 * (extra + 1) if extra else 0)
        blocks = [pitched(cy, pl, poison), pitched(uv, pc, poison)]
    else:
        pc = sw // 2 + (extra + 1 if extra else 0)
        blocks = [pitched(cy, pl, poison), pitched(cu, pc, poison), pitched(cv, pc, poison)]
    return (y, u, v), blocks, pl, pc
