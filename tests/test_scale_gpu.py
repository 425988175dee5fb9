"""xeve_hip_surface_to_yuv420 on the GPU (xeve_amd/csrc/scale.hip): decoder surfaces -- planar and semi-planar, 8 bits, 10 bits low-aligned and msb-aligned, rows and
pictures further apart than their content with poison in the gaps -- -> the frames the encoder takes at another size, EQUAL to the numpy / Fraction restatement of the
definition (tests/_scale.py).  The sizes are the smallest at which a path can go wrong: 2x2 (every tap clamps), the 8 : 1 limits either way, odd chroma lengths, shrinking
in one axis while enlarging in the other, an output of several 64 x 16 tiles whose source windows straddle them, and the widest and tallest strips.  Outputs lie inside
sentinel-filled buffers that are compared whole."""
import ctypes as C
import itertools

import numpy as np
import pytest

import _scale as K

pytestmark = [pytest.mark.gpu, pytest.mark.gpu_full]

FILL = 0xA5
# source -> destination.  300x140 -> 264x132: 5 x 9 luma tiles (3 x 5 chroma), the last ones cut in both directions
SIZES = [((2, 2), (2, 2)), ((16, 16), (2, 2)), ((2, 2), (16, 16)), ((70, 50), (62, 36)), ((202, 138), (130, 66)), ((128, 18), (34, 70)), ((300, 140), (264, 132)),
         ((8192, 2), (1024, 2)), ((2, 4320), (2, 540))]


@pytest.fixture(scope="module")
def dev():
    import torch

    import xeve_amd

    xeve_amd.init(0)
    return torch.device("cuda:0")


def _stacked(rng, n, sw, sh, layout, fmt, kind, extra, gap):
    """n surfaces: (the sample planes per picture, the flat blocks -- one per plane, the pictures `gap` containers further apart than a picture, the gaps poisoned --, luma
    and chroma pitch, luma and chroma picture distance; all in containers)"""
    pics = [K.surface(rng, sw, sh, layout, fmt, kind, extra) for _ in range(n)]
    blocks = []
    for p in range(len(pics[0][1])):
        one = pics[0][1][p]
        flat = np.full(n * (one.size + gap), 0x5A if one.itemsize == 1 else 0x5A5A, one.dtype)
        for i, pic in enumerate(pics):
            flat[i * (one.size + gap):i * (one.size + gap) + one.size] = pic[1][p]
        blocks.append(flat)
    return [p[0] for p in pics], blocks, pics[0][2], pics[0][3], pics[0][1][0].size + gap, pics[0][1][1].size + gap


def _to_dev(a, dev):
    import torch

    return torch.from_numpy(a.view(np.int16) if a.dtype.itemsize == 2 else a).to(dev)


def _desc(tensors, layout, fmt, pl, pc, dl=0, dc=0):
    from xeve_amd import lib

    sb, depth, shift = K.FORMATS[fmt]
    s = lib.Surface(1 if layout == "nv" else 0, sb, depth, shift)
    for i, t in enumerate(tensors):
        s.plane[i] = t.data_ptr()
    s.pitch_l, s.pitch_c, s.pic_l, s.pic_c = pl * sb, pc * sb, dl * sb, dc * sb
    return s


def _run(dev, rng, sw, sh, w, h, layout, fmt, siting, kind, extra, n):
    """one call into a sentinel-filled buffer; returns (the whole buffer, what it must hold, the unclamped restatement's planes)"""
    import torch

    from xeve_amd import lib

    sb, depth, _ = K.FORMATS[fmt]
    planes, blocks, pl, pc, dl, dc = _stacked(rng, n, sw, sh, layout, fmt, kind, extra, 11 if n > 1 else 0)
    tensors = [_to_dev(b, dev) for b in blocks]
    sbo = 2 if depth > 8 else 1
    per, lead, gap = w * h * 3 // 2 * sbo, 3 * sbo, (5 * sbo if n > 1 else 0)
    out = torch.full((lead + n * (per + gap) + 64,), FILL, dtype=torch.uint8, device=dev)
    want = np.full(out.numel(), FILL, np.uint8)
    for p in range(n):
        want[lead + p * (per + gap):lead + p * (per + gap) + per] = K.frame(*planes[p], w, h, siting, depth).view(np.uint8)
    s = _desc(tensors, layout, fmt, pl, pc, dl, dc)
    torch.cuda.synchronize()
    rc = lib.load().xeve_hip_surface_to_yuv420(C.byref(s), sw, sh, K.SITINGS.index(siting), w, h, depth, n, C.c_void_p(out.data_ptr() + lead), per + gap, None)
    assert rc == 0, lib.last_error()
    torch.cuda.synchronize()
    for t, b in zip(tensors, blocks):  # the input is only read
        assert np.array_equal(t.cpu().numpy().view(b.dtype), b)
    return out.cpu().numpy(), want, planes


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_the_kernel_equals_the_restatement(size, dev):
    """layout x format x siting x pitch (the row's length / larger, poison in the gap), three pictures further apart than their size on both sides, the content rotating
    through random, all-maximum and the one-sample checkerboard; every layout and format once more with a single picture"""
    (sw, sh), (w, h) = size
    rng = np.random.default_rng(sw * 7 + sh * 3 + w)
    turn = itertools.count()
    for layout, fmt, siting, extra in itertools.product(("nv", "planar"), K.FORMATS, K.SITINGS, (0, 6)):
        kind = K.CONTENTS[next(turn) % 3]
        got, want, _ = _run(dev, rng, sw, sh, w, h, layout, fmt, siting, kind, extra, 3)
        assert np.array_equal(got, want), (layout, fmt, siting, extra, kind)
    for layout, fmt in itertools.product(("nv", "planar"), K.FORMATS):
        got, want, _ = _run(dev, rng, sw, sh, w, h, layout, fmt, "left", "random", 2, 1)
        assert np.array_equal(got, want), (layout, fmt)


@pytest.mark.parametrize("fmt", K.FORMATS)
def test_overshoot_is_clamped_at_both_ends(fmt, dev):
    """two-sample squares of 0 and the maximum shrunk, random content enlarged: the restatement WITHOUT its clamp leaves 0 .. 2^d - 1 at both ends in luma and in chroma, and
    the kernel's output is the clamped one"""
    rng = np.random.default_rng(77)
    depth = K.FORMATS[fmt][1]
    for (sw, sh), (w, h), kind in (((70, 50), (62, 36), "blocks"), ((34, 18), (128, 70), "random")):
        got, want, planes = _run(dev, rng, sw, sh, w, h, "nv", fmt, "left", kind, 6, 1)
        raw = K.scale_planes(*planes[0], w, h, "left", depth, clamp=False)
        for p in raw:
            assert p.min() < 0 and p.max() > (1 << depth) - 1, (sw, sh, w, h, int(p.min()), int(p.max()))
        assert np.array_equal(got, want)


@pytest.mark.parametrize("fmt", K.FORMATS)
@pytest.mark.parametrize("layout", ("nv", "planar"))
def test_a_same_size_call_is_deinterleave_shift_and_pitch_removal(layout, fmt, dev):
    rng = np.random.default_rng(5)
    sb, depth, _ = K.FORMATS[fmt]
    for w, h in ((70, 50), (64, 16), (2, 2)):
        got, want, planes = _run(dev, rng, w, h, w, h, layout, fmt, "left", "random", 10, 1)
        sbo = 2 if depth > 8 else 1
        exact = np.concatenate([p.reshape(-1) for p in planes[0]]).astype(np.uint8 if depth == 8 else "<u2").view(np.uint8)
        assert np.array_equal(got[3 * sbo:3 * sbo + exact.size], exact) and np.array_equal(got, want)


def test_the_python_face(dev):
    """surface_to_yuv420 on tensors: NV12 as views of wider tensors (the pitch comes from stride()), P010 with msb_aligned, a planar (u, v) pair, a leading axis of pictures,
    and what is no surface"""
    import torch

    from xeve_amd import encode

    rng = np.random.default_rng(13)
    sw, sh, w, h = 70, 50, 34, 26
    (y, u, v), _, _, _ = K.surface(rng, sw, sh, "nv", "u8")
    base_y = torch.zeros((sh, sw + 10), dtype=torch.uint8, device=dev)
    base_uv = torch.zeros((sh // 2, sw // 2 + 3, 2), dtype=torch.uint8, device=dev)
    ty, tuv = base_y[:, 4:4 + sw], base_uv[:, 1:1 + sw // 2]
    ty[:] = torch.from_numpy(y.astype(np.uint8)).to(dev)
    tuv[:] = torch.from_numpy(np.stack([u, v], axis=2).astype(np.uint8)).to(dev)
    got = encode.surface_to_yuv420(ty, tuv, w, h, siting="centre")
    assert got.dtype == torch.uint8 and got.shape == (w * h * 3 // 2,)
    assert np.array_equal(got.cpu().numpy(), K.frame(y, u, v, w, h, "centre", 8))
    # P010: three pictures at once, the sample in the top bits
    pics = [K.content(rng, "random", sh, sw, 10) for _ in range(3)]
    word = lambda p: torch.from_numpy((p << 6).astype(np.uint16).view(np.int16)).to(dev)
    sy = torch.stack([word(p[0]) for p in pics])
    suv = torch.stack([word(np.stack([p[1], p[2]], axis=2)) for p in pics])
    got = encode.surface_to_yuv420(sy, suv, w, h, msb_aligned=True)
    assert got.dtype == torch.int16 and got.shape == (3, w * h * 3 // 2)
    for i, p in enumerate(pics):
        assert np.array_equal(got[i].cpu().numpy().view(np.uint16), K.frame(*p, w, h, "left", 10))
    # planar, low-aligned: a (u, v) pair cut out of one tensor
    low = lambda p: torch.from_numpy(p.astype(np.uint16).view(np.int16)).to(dev)
    y0, u0, v0 = pics[0]
    c = torch.stack([low(u0), low(v0)])
    lo = encode.surface_to_yuv420(low(y0), (c[0], c[1]), w, h)
    assert np.array_equal(lo.cpu().numpy().view(np.uint16), K.frame(y0, u0, v0, w, h, "left", 10))
    with pytest.raises(ValueError):
        encode.surface_to_yuv420(ty, tuv, w, h, siting="right")
    with pytest.raises(ValueError):
        encode.surface_to_yuv420(ty, tuv, w, h, msb_aligned=True)  # (bytes have no top bits to spare)
    with pytest.raises(ValueError):
        encode.surface_to_yuv420(ty, tuv[:, :-1], w, h)
    with pytest.raises(ValueError):
        encode.surface_to_yuv420(ty.float(), tuv.float(), w, h)
    with pytest.raises(ValueError):
        encode.surface_to_yuv420(ty[:, ::2], tuv, w, h)  # (the samples of a row must be neighbours)
    first, coef, ntaps = encode.scale_filter(sw, w, 1)
    want = K.table(sw, w, 1)
    assert first == want[0].tolist() and coef == want[1].tolist() and ntaps == want[2]


def test_arguments_outside_the_contract_are_refused(dev):
    """XEVE_HIP_ERR_ARG before any launch: odd or oversized sizes, a ratio beyond 8 on either axis either way, a frame depth that is not the surface's, an unknown layout,
    sample size, depth, shift or siting, 10 bits in bytes, 8 bits in words, no pictures or too many, host memory on either side, null pointers, misaligned pointers, pitches and distances, a
    pitch below the row, a frame distance below the frame, an output that overlaps the source"""
    import torch

    from xeve_amd import lib

    L = lib.load()
    sw, sh, w, h = 70, 50, 62, 36
    block = torch.zeros((1 << 16,), dtype=torch.int16, device=dev)  # luma at 0, chroma behind it, the output behind both
    lum, chr_, out = block.data_ptr(), block.data_ptr() + 2 * sw * sh, block.data_ptr() + 2 * (sw * sh * 3 // 2 + 64)
    host = np.zeros(sw * sh * 4, np.uint8)
    base = dict(layout=1, sb=2, sdepth=10, shift=6, y=lum, c=chr_, c2=chr_, pl=2 * sw, pc=2 * sw, dl=0, dc=0, sw=sw, sh=sh, siting=0, w=w, h=h, depth=10, n=1, out=out,
                pic=w * h * 3, desc=True)
    bad = (dict(sw=69), dict(sh=51), dict(w=61), dict(h=35), dict(sw=0), dict(w=0), dict(w=8194, sw=8194), dict(h=4322, sh=4322), dict(sw=8194), dict(sh=4322),
           dict(w=8), dict(h=6), dict(sw=6, w=62), dict(sh=4, h=36), dict(depth=8), dict(sdepth=8, depth=8, shift=6), dict(sdepth=8, depth=8, shift=0), dict(sdepth=8, depth=8, shift=8), dict(sdepth=12, depth=12), dict(layout=2), dict(layout=-1),
           dict(sb=4), dict(sb=0), dict(sb=1), dict(shift=2), dict(shift=8), dict(shift=-6), dict(siting=2), dict(n=0), dict(n=65536), dict(y=host.ctypes.data),
           dict(c=host.ctypes.data), dict(out=host.ctypes.data), dict(y=None), dict(c=None), dict(out=None), dict(desc=False), dict(layout=0, c2=None), dict(y=lum + 1), dict(c=chr_ + 1),
           dict(out=out + 1), dict(pl=2 * sw - 2), dict(pc=2 * sw - 2), dict(pl=2 * sw + 1), dict(pc=2 * sw + 1), dict(n=2, dl=1), dict(n=2, dc=-2), dict(pl=-2 * sw),
           dict(pic=w * h * 3 - 2), dict(pic=w * h * 3 + 1), dict(out=lum), dict(out=chr_ + 2 * sw * (sh // 2) - 2), dict(y=lum + 4000, out=lum),
           dict(n=3, dl=2 * sw * sh, dc=2 * sw * sh // 2, out=lum + 2 * 3 * sw * sh - 2))

    def call(k):
        s = lib.Surface(k["layout"], k["sb"], k["sdepth"], k["shift"])
        s.plane[0], s.plane[1], s.plane[2] = k["y"], k["c"], k["c2"]
        s.pitch_l, s.pitch_c, s.pic_l, s.pic_c = k["pl"], k["pc"], k["dl"], k["dc"]
        return L.xeve_hip_surface_to_yuv420(C.byref(s) if k["desc"] else None, k["sw"], k["sh"], k["siting"], k["w"], k["h"], k["depth"], k["n"], k["out"], k["pic"], None)

    block.fill_(21)
    for kw in bad:
        assert call(dict(base, **kw)) == -2 and "invalid argument" in lib.last_error(), kw
    torch.cuda.synchronize()
    assert bool((block == 21).all())
    assert call(base) == 0, lib.last_error()  # (and the base of the list is a call that runs)
    assert call(dict(base, layout=0, pc=sw, c2=chr_ + sw * (sh // 2))) == 0, lib.last_error()
    torch.cuda.synchronize()


def test_the_table_cache_turns_over_and_outlives_a_rebind(dev):
    """20 source sizes to one destination size are 80 axes, more than the 64 the cache keeps for a device: the call that would pass the limit waits for the device and
    frees its axes, and the sizes met before give the same frames again.  Then, in a process of its own (a shutdown must not pull the library from under this one's other
    tests): scale, xeve_hip_shutdown, xeve_hip_init, scale again -- the first call after the re-bind frees the old tables and derives new ones"""
    import subprocess
    import sys

    from _libs import ROOT

    for turn in range(2):
        for i in range(20):
            sw, sh = 16 + 2 * i, 12 + 2 * i
            got, want, _ = _run(dev, np.random.default_rng(100 + i), sw, sh, 16, 12, "nv", "u8", "left", "random", 2, 1)
            assert np.array_equal(got, want), (turn, sw, sh)
    code = """
import ctypes as C, sys
import numpy as np, torch
sys.path.insert(0, "tests")
import _scale as K
import xeve_amd
from xeve_amd import encode, lib
dev = torch.device("cuda:0")
(y, u, v), _, _, _ = K.surface(np.random.default_rng(3), 70, 50, "nv", "u8")
ty = torch.from_numpy(y.astype(np.uint8)).to(dev)
tuv = torch.from_numpy(np.stack([u, v], axis=2).astype(np.uint8)).to(dev)
want = K.frame(y, u, v, 34, 26, "left", 8)
for turn in range(2):
    xeve_amd.init(0)
    for _ in range(2):
        assert np.array_equal(encode.surface_to_yuv420(ty, tuv, 34, 26).cpu().numpy(), want), turn
    torch.cuda.synchronize()
    lib.load().xeve_hip_shutdown()
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
