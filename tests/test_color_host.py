"""CPU suite: the colour conversions without a GPU.  xeve_hip_color_matrix (host only) against the Fraction derivation of tests/_color.py, the properties the definition
promises (rows' sums, the grey points, the distance to the float64 textbook conversion, the clamp of full-range chroma), and xeve_amd/csrc/color_core.h -- the per-lane
code of color.hip's kernels -- compiled for the host and held to the numpy restatement bit for bit in both directions.  tests/native/color_host.cpp is a stand-alone
program built with the address and undefined-behaviour sanitizers and run as a child process: its buffers are heap blocks of exactly their size."""
import ctypes as C
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

import _color as K
from _libs import ROOT

SRC = os.path.join(ROOT, "tests", "native", "color_host.cpp")
HDR = os.path.join(ROOT, "xeve_amd", "csrc", "color_core.h")
OUT = os.path.join(ROOT, "tests", "native", "build", "color_host")
SETTINGS = list(itertools.product(K.MATRICES, (False, True), (8, 10)))


def library_matrix(matrix, full, depth, siting="left"):
    from xeve_amd import lib

    col = lib.Color(K.MATRICES.index(matrix), int(full), K.SITINGS.index(siting), depth)
    fwd, off, inv = (C.c_int64 * 9)(), (C.c_int64 * 2)(), (C.c_int64 * 5)()
    assert lib.load().xeve_hip_color_matrix(C.byref(col), fwd, off, inv) == 0, lib.last_error()
    return [list(fwd[0:3]), list(fwd[3:6]), list(fwd[6:9])], tuple(off), list(inv)


@pytest.mark.parametrize("matrix,full,depth", SETTINGS)
def test_the_librarys_coefficients_are_the_fraction_derivation(matrix, full, depth):
    fwd, off, inv = library_matrix(matrix, full, depth)
    m, oy, oc = K.fwd_matrix(matrix, full, depth)
    assert fwd == m and off == (oy, oc)
    assert inv == list(K.inv_matrix(matrix, full)[:5])


@pytest.mark.parametrize("matrix,full,depth", SETTINGS)
def test_chroma_rows_sum_to_zero_and_the_luma_row_to_rnd_a(matrix, full, depth):
    fwd, _, _ = library_matrix(matrix, full, depth)
    from fractions import Fraction

    assert sum(fwd[1]) == 0 and sum(fwd[2]) == 0
    assert sum(fwd[0]) == K.rnd(Fraction(K.scales(full, depth)[0] << K.S, 65535))


def test_a_refused_setting_is_an_error_not_a_matrix():
    from xeve_amd import lib

    out = (C.c_int64 * 9)(), (C.c_int64 * 2)(), (C.c_int64 * 5)()
    for bad in (lib.Color(3, 0, 0, 10), lib.Color(0, 2, 0, 10), lib.Color(0, 0, 0, 9), lib.Color(-1, 0, 0, 8), lib.Color(0, 0, 2, 8)):
        assert lib.load().xeve_hip_color_matrix(C.byref(bad), *out) == -2 and "invalid argument" in lib.last_error()
    assert lib.load().xeve_hip_color_matrix(None, *out) == -2


@pytest.mark.parametrize("matrix", K.MATRICES)
@pytest.mark.parametrize("siting", K.SITINGS)
def test_white_black_and_mid_grey_at_depth_10_limited_range(matrix, siting):
    for value, luma in ((255, 940), (0, 64)):
        y, u, v = K.forward(K.c16(np.full((4, 4, 3), value, np.uint8)), matrix, False, siting, 10)
        assert (y == luma).all() and (u == 512).all() and (v == 512).all()
    y, u, v = K.forward(K.c16(np.full((4, 4, 3), 0.5, np.float32)), matrix, False, siting, 10)
    assert (y == 502).all() and (u == 512).all() and (v == 512).all()


@pytest.mark.parametrize("matrix,full,depth", SETTINGS)
def test_the_forward_result_stays_within_0_506_code_values_of_the_textbook(matrix, full, depth):
    """200 000 random triples, no subsampling (flat 2x2 blocks: the chroma sum is 4 times the pixel).  The bound is the final rounding (0.5) plus the coefficients'
    rounding (three of at most half a unit of 2^-24 each, times 65535: 3 * 65535 / 2^25)"""
    rng = np.random.default_rng(K.MATRICES.index(matrix) * 4 + full * 2 + depth)
    t = rng.integers(0, 65536, size=(200000, 3), dtype=np.int64)
    t[:8] = [[0, 0, 0], [65535] * 3, [65535, 0, 0], [0, 65535, 0], [0, 0, 65535], [65535, 65535, 0], [0, 65535, 65535], [65535, 0, 65535]]
    pic = np.repeat(np.repeat(t.reshape(400, 500, 3), 2, axis=0), 2, axis=1)
    y, u, v = K.forward(pic, matrix, full, "centre", depth)
    top = (1 << depth) - 1
    want = [np.clip(p.reshape(400, 500), 0, top) for p in K.textbook(t / 65535.0, matrix, full, depth)]
    bound = 0.5 + 3 * 65535 / 2 ** 25
    worst = max(float(np.abs(got - w).max()) for got, w in zip((y[::2, ::2], u, v), want))
    print("largest distance to the float64 conversion: %.4f (bound %.4f)" % (worst, bound))
    assert worst <= bound


@pytest.mark.parametrize("matrix", K.MATRICES)
@pytest.mark.parametrize("depth", (8, 10))
def test_full_range_chroma_of_saturated_blue_and_red_is_clamped(matrix, depth):
    top = (1 << depth) - 1
    for rgb, plane in (((0, 0, 255), 1), ((255, 0, 0), 2)):
        planes = K.forward(K.c16(np.full((2, 2, 3), rgb, np.uint8)), matrix, True, "centre", depth)
        assert (planes[plane] == top).all()


# ---- color_core.h on the host ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program():
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                               "-static-libubsan", "-o", OUT, SRC])  # (the runtimes linked in: the program needs nothing preloaded)
    return OUT


def _elements(a, dtype):
    """the picture's elements as the bytes of the tensor's dtype (bfloat16: the upper halves of the float32 values, which hold them exactly)"""
    if dtype == "bfloat16":
        return (a.view(np.uint32) >> 16).astype(np.uint16)
    return a


def _layout(w, h, layout):
    """(stride_x, stride_y, stride_c, elements) of a block with rows padded by 5 pixels: hwc, or chw with padded planes as well"""
    if layout == "hwc":
        return 3, 3 * (w + 5), 1, 3 * (w + 5) * (h - 1) + 3 * w
    plane = (w + 5) * h + 7
    return 1, w + 5, plane, 2 * plane + (w + 5) * (h - 1) + w


def _place(pic, w, h, layout, fill):
    sx, sy, sc, n = _layout(w, h, layout)
    buf = np.full(n, fill, pic.dtype)
    np.lib.stride_tricks.as_strided(buf, (h, w, 3), tuple(s * buf.itemsize for s in (sy, sx, sc)))[:] = pic
    return buf


def _jobs():
    rng = np.random.default_rng(24)
    jobs = []
    for n, ((w, h), dtype, siting) in enumerate(itertools.product(K.SHAPES, K.DTYPES, K.SITINGS)):
        matrix, full, depth = SETTINGS[n % len(SETTINGS)]
        layout = ("hwc", "chw")[(n // 2) % 2]
        jobs.append(dict(direction=0, dtype=dtype, siting=siting, matrix=matrix, full=full, depth=depth, w=w, h=h, layout=layout, data=K.picture(rng, w, h, dtype)))
        yuv = rng.integers(0, 1024, size=w * h * 3 // 2).astype("<u2")
        jobs.append(dict(direction=1, dtype=dtype, siting=siting, matrix=matrix, full=full, depth=10, w=w, h=h, layout=layout, data=yuv))
    primaries = np.array([[0, 0, 255], [255, 0, 0], [0, 255, 0], [255, 255, 255]], np.uint8)[rng.integers(0, 4, size=(6, 10))]  # full range: saturated chroma meets the clamp
    for matrix, depth, siting in itertools.product(K.MATRICES, (8, 10), K.SITINGS):
        jobs.append(dict(direction=0, dtype="uint8", siting=siting, matrix=matrix, full=True, depth=depth, w=10, h=6, layout="hwc", data=primaries))
        flat = np.repeat(np.repeat(primaries[:3, :5], 2, axis=0), 2, axis=1)
        jobs.append(dict(direction=0, dtype="uint8", siting=siting, matrix=matrix, full=True, depth=depth, w=10, h=6, layout="chw", data=flat))
    return jobs


def test_the_lane_code_equals_the_restatement_in_both_directions(program, tmp_path):
    jobs = _jobs()
    src, dst = os.path.join(str(tmp_path), "jobs.bin"), os.path.join(str(tmp_path), "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<q", len(jobs)))
        for j in jobs:
            sx, sy, sc, n = _layout(j["w"], j["h"], j["layout"])
            f.write(struct.pack("<12q", j["direction"], K.DTYPES.index(j["dtype"]), K.SITINGS.index(j["siting"]), K.MATRICES.index(j["matrix"]), int(j["full"]), j["depth"], j["w"], j["h"],
                                sx, sy, sc, n))
            f.write((_place(_elements(j["data"], j["dtype"]), j["w"], j["h"], j["layout"], 0) if j["direction"] == 0 else j["data"]).tobytes())
    r = subprocess.run([program, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    got = open(dst, "rb").read()
    at = 0
    for j in jobs:
        w, h = j["w"], j["h"]
        key = {k: j[k] for k in ("direction", "dtype", "siting", "matrix", "full", "depth", "w", "h", "layout")}
        if j["direction"] == 0:
            want = K.forward_frame(j["data"], j["matrix"], j["full"], j["siting"], j["depth"])
        else:
            pic = K.inverse_frame(j["data"], w, h, j["dtype"], j["matrix"], j["full"], j["siting"])
            want = _place(pic, w, h, j["layout"], np.frombuffer(b"\xa5" * pic.itemsize, pic.dtype)[0])  # (what the program filled its block with survives between the rows)
        raw = want.tobytes()
        assert got[at:at + len(raw)] == raw, key
        at += len(raw)
    assert at == len(got)
