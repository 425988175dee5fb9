"""The colour conversions of include/xeve_hip.h ("RGB TENSORS IN AND OUT") restated in numpy and fractions.Fraction from the definition's text -- not from the library:
what tests/test_color_host.py, test_color_gpu.py and test_enc_rgb_gpu.py hold xeve_hip_color_matrix, color_core.h and the kernels of color.hip to, bit for bit."""
from fractions import Fraction

import numpy as np

S = 24
KRKB = {"bt601": (Fraction(299, 1000), Fraction(114, 1000)), "bt709": (Fraction(2126, 10000), Fraction(722, 10000)), "bt2020nc": (Fraction(2627, 10000), Fraction(593, 10000))}
MATRICES = ("bt601", "bt709", "bt2020nc")
SITINGS = ("left", "centre")
DTYPES = ("uint8", "float16", "bfloat16", "float32")
SHAPES = [(2, 2), (4, 2), (2, 4), (6, 10), (70, 50), (64, 64), (258, 6)]  # (w, h): every tap clamps; one block column / row; odd chroma rows; more than one workgroup along a row


def rnd(q):
    """round half away from zero of an exact rational"""
    q = Fraction(q)
    n = (abs(q) * 2 + 1) // 2
    return int(n) if q >= 0 else -int(n)


def scales(full, d):
    """(sY, sC, oY, oC)"""
    if full:
        return (1 << d) - 1, (1 << d) - 1, 0, 1 << (d - 1)
    return 219 << (d - 8), 224 << (d - 8), 16 << (d - 8), 1 << (d - 1)


def fwd_matrix(matrix, full, d):
    """([[mYR, mYG, mYB], [Cb row], [Cr row]], oY, oC)"""
    kr, kb = KRKB[matrix]
    sy, sc, oy, oc = scales(full, d)
    a, c = Fraction(sy << S, 65535), Fraction(sc << S, 65535)
    yr, yb = rnd(a * kr), rnd(a * kb)
    yg = rnd(a) - yr - yb
    ub, ur = rnd(c / 2), rnd(-c * kr / (2 * (1 - kb)))
    ug = -ub - ur
    vr, vb = rnd(c / 2), rnd(-c * kb / (2 * (1 - kr)))
    vg = -vr - vb
    return [[yr, yg, yb], [ur, ug, ub], [vr, vg, vb]], oy, oc


def inv_matrix(matrix, full):
    """(iY, rCr, gCb, gCr, bCb, oY, oC) -- d = 10"""
    kr, kb = KRKB[matrix]
    kg = 1 - kr - kb
    sy, sc, oy, oc = scales(full, 10)
    ic = Fraction(65535 << S, sc)
    return rnd(Fraction(65535 << S, sy)), rnd(2 * (1 - kr) * ic), rnd(-2 * kb * (1 - kb) / kg * ic), rnd(-2 * kr * (1 - kr) / kg * ic), rnd(2 * (1 - kb) * ic), oy, oc


def c16(a):
    """components as 16 bits: a uint8 array, or a float array (float16 / float32; bfloat16 widened to float32 by the caller, which is exact)"""
    a = np.asarray(a)
    if a.dtype == np.uint8:
        return a.astype(np.int64) * 257
    x = a.astype(np.float32)
    x = np.where(np.isnan(x), np.float32(0), x)
    x = np.minimum(np.maximum(x, np.float32(0)), np.float32(1)).astype(np.float32)
    p = (x * np.float32(65535)).astype(np.float32)  # rounded to float32
    t = (p + np.float32(0.5)).astype(np.float32)  # and again
    return np.floor(t).astype(np.int64)


def forward(c, matrix="bt709", full=False, siting="left", depth=10):
    """c: (h, w, 3) of c16 values -> (Y (h, w), U, V (h / 2, w / 2)) as int64"""
    c = np.asarray(c, np.int64)
    h, w, _ = c.shape
    m, oy, oc = fwd_matrix(matrix, full, depth)
    top = (1 << depth) - 1
    y = np.clip((c[..., 0] * m[0][0] + c[..., 1] * m[0][1] + c[..., 2] * m[0][2] + (oy << S) + (1 << (S - 1))) >> S, 0, top)
    rows = c[0::2] + c[1::2]  # rows 2j, 2j + 1, weights 1 1
    if siting == "centre":
        s, L = rows[:, 0::2] + rows[:, 1::2], 2
    else:
        i = np.arange(w // 2)
        s, L = rows[:, np.clip(2 * i - 1, 0, w - 1)] + 2 * rows[:, 2 * i] + rows[:, np.clip(2 * i + 1, 0, w - 1)], 3
    out = [y]
    for r in (1, 2):
        out.append(np.clip((s[..., 0] * m[r][0] + s[..., 1] * m[r][1] + s[..., 2] * m[r][2] + (oc << (S + L)) + (1 << (S + L - 1))) >> (S + L), 0, top))
    return out


def frame(planes, depth):
    """Y, U, V as the pushed frame: one byte per sample at depth 8, 16-bit little-endian at depth 10"""
    flat = np.concatenate([p.reshape(-1) for p in planes])
    return flat.astype(np.uint8) if depth == 8 else flat.astype("<u2")


def forward_frame(rgb, matrix="bt709", full=False, siting="left", depth=10):
    """an (h, w, 3) uint8 / float picture -> the samples of its frame (uint8 / uint16 array)"""
    return frame(forward(c16(rgb), matrix, full, siting, depth), depth)


def split(samples, w, h):
    """a frame's samples -> Y, U, V planes (int64)"""
    s = np.asarray(samples).astype(np.int64)
    n = w * h
    return s[:n].reshape(h, w), s[n:n + n // 4].reshape(h // 2, w // 2), s[n + n // 4:n + n // 2].reshape(h // 2, w // 2)


def _upsample(c, w, h, siting):
    """the chroma plane at every luma pixel as a sum of weight 16"""
    ch, cw = c.shape
    y = np.arange(h)
    cy = y >> 1
    other = np.clip(np.where(y & 1, cy + 1, cy - 1), 0, ch - 1)
    v = 3 * c[cy] + c[other]  # (h, cw)
    x = np.arange(w)
    cx = x >> 1
    if siting == "centre":
        return 3 * v[:, cx] + v[:, np.clip(np.where(x & 1, cx + 1, cx - 1), 0, cw - 1)]
    right = np.clip(cx + 1, 0, cw - 1)
    return np.where(x & 1, 2 * v[:, cx] + 2 * v[:, right], 4 * v[:, cx])


def inverse(y, u, v, matrix="bt709", full=False, siting="left"):
    """10-bit planes -> (h, w, 3) of 16-bit R, G, B (int64)"""
    iy, rcr, gcb, gcr, bcb, oy, oc = inv_matrix(matrix, full)
    h, w = y.shape
    sb, sr = _upsample(np.asarray(u, np.int64), w, h, siting) - 16 * oc, _upsample(np.asarray(v, np.int64), w, h, siting) - 16 * oc
    lum = 16 * iy * (np.asarray(y, np.int64) - oy) + (1 << (S + 3))
    r = np.clip((lum + rcr * sr) >> (S + 4), 0, 65535)
    g = np.clip((lum + gcb * sb + gcr * sr) >> (S + 4), 0, 65535)
    b = np.clip((lum + bcb * sb) >> (S + 4), 0, 65535)
    return np.stack([r, g, b], axis=-1)


def out(v16, dtype):
    """16-bit components as the output element type; bfloat16 comes back as the uint16 bit patterns (float32 rounded to nearest-even by torch on the CPU)"""
    if dtype == "uint8":
        return ((v16 + 128) // 257).astype(np.uint8)
    f = (v16.astype(np.float32) / np.float32(65535)).astype(np.float32)
    if dtype == "float32":
        return f
    if dtype == "float16":
        return f.astype(np.float16)
    import torch

    return torch.from_numpy(f).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def inverse_frame(samples, w, h, dtype, matrix="bt709", full=False, siting="left"):
    return out(inverse(*split(samples, w, h), matrix, full, siting), dtype)


def textbook(rgb01, matrix, full, depth):
    """the float64 conversion of the books, unrounded: (..., 3) in [0, 1] -> Y, Cb, Cr code values at a pixel (no subsampling)"""
    kr, kb = (float(k) for k in KRKB[matrix])
    kg = 1 - kr - kb
    sy, sc, oy, oc = scales(full, depth)
    r, g, b = rgb01[..., 0], rgb01[..., 1], rgb01[..., 2]
    e = kr * r + kg * g + kb * b
    return oy + sy * e, oc + sc * (b - e) / (2 * (1 - kb)), oc + sc * (r - e) / (2 * (1 - kr))


def special_floats(n, rng):
    """n float32 values in and around [0, 1] with what the definition singles out: NaN, +-inf, -1, 2, the ends, and x whose x * 65535 + 0.5 lies on or next to an
    integer, where one rounding more or less changes the floor"""
    fixed = np.array([np.nan, np.inf, -np.inf, -1.0, 2.0, 0.0, 1.0, -0.0, 0.5, 1e-8, 1 - 2 ** -24], np.float32)
    k = rng.integers(0, 65535, size=max(0, n // 2)).astype(np.float64)
    edge = ((k + 0.5) / 65535).astype(np.float32)  # x * 65535 is next to k + 0.5: the sum sits on the boundary
    edge = np.concatenate([edge, np.nextafter(edge, np.float32(0)), np.nextafter(edge, np.float32(1))])
    pool = np.concatenate([fixed, edge, rng.random(n).astype(np.float32)])
    got = pool[rng.permutation(pool.size)[:n]]
    got[:min(n, fixed.size)] = fixed[:min(n, fixed.size)]
    return got


def picture(rng, w, h, dtype):
    """a random (h, w, 3) picture of the element type (bfloat16: returned as float32 values that bfloat16 holds exactly, the caller narrows them), floats with the
    special values mixed in"""
    if dtype == "uint8":
        return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    x = special_floats(h * w * 3, rng).reshape(h, w, 3)
    if dtype == "float16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16)
    if dtype == "bfloat16":
        return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    return x
