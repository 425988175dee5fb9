"""CPU suite: the surface scaler without a GPU.  xeve_hip_scale_filter (host only) against the Fraction derivation of tests/_scale.py for the pairs that matter -- the
identity, the 8 : 1 limits either way, the ladder's ratios, odd ratios, the widest and tallest pictures -- in both kinds; what the definition promises of a table (rows sum
to 2^14, the identity, the tap count, the sums of |c| behind the kernel's 16-bit intermediate and 32-bit sums); the refusals of the host-side checks; and
xeve_amd/csrc/scale_core.h -- the per-lane code of scale.hip's kernel -- compiled for the host and held to the numpy restatement bit for bit.  tests/native/scale_host.cpp
is a stand-alone program built with the address and undefined-behaviour sanitizers and run as a child process: its planes are heap blocks of exactly their size."""
import ctypes as C
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

import _scale as K
from _libs import ROOT

SRC = os.path.join(ROOT, "tests", "native", "scale_host.cpp")
HDR = os.path.join(ROOT, "xeve_amd", "csrc", "scale_core.h")
OUT = os.path.join(ROOT, "tests", "native", "build", "scale_host")
PAIRS = [(64, 64), (2, 2), (16, 2), (2, 16), (1080, 720), (2160, 540), (1366, 854), (70, 62), (130, 70), (202, 130), (8192, 1024), (4320, 540)]


def library_table(src_n, dst_n, kind):
    from xeve_amd import encode

    first, coef, ntaps = encode.scale_filter(src_n, dst_n, kind)
    return np.array(first, np.int64), np.array(coef, np.int64).reshape(len(first), ntaps), ntaps


@pytest.mark.parametrize("kind", (0, 1))
@pytest.mark.parametrize("src_n,dst_n", PAIRS)
def test_the_librarys_table_is_the_fraction_derivation(src_n, dst_n, kind):
    first, coef, ntaps = library_table(src_n, dst_n, kind)
    want_first, want_coef, want_ntaps = K.table(src_n, dst_n, kind)
    assert ntaps == want_ntaps and np.array_equal(first, want_first) and np.array_equal(coef, want_coef)


@pytest.mark.parametrize("kind", (0, 1))
@pytest.mark.parametrize("src_n,dst_n", PAIRS)
def test_rows_sum_to_one_and_the_narrowed_types_hold(src_n, dst_n, kind):
    """every row sums to 2^14; at most 4 taps when enlarging, 4 sn / dn + 1 when shrinking; and with A = the largest sum of |c| the kernel's types hold at both depths:
    |T| <= ((A * (2^d - 1) + 2^9) >> 10) + 1 fits 16 bits, and A * (any 16-bit T) + 2^17 fits 32 -- the bound the host checks per pair of tables before a launch"""
    first, coef, ntaps = library_table(src_n, dst_n, kind)
    assert (coef.sum(axis=1) == 1 << 14).all()
    assert ntaps <= (4 if dst_n >= src_n else 4 * src_n // dst_n + 1)
    assert np.abs(coef).max() <= 32767
    a = int(np.abs(coef).sum(axis=1).max())
    print("%d -> %d kind %d: %d taps, largest sum of |c| %d (%.4f)" % (src_n, dst_n, kind, ntaps, a, a / 16384))
    for depth in (8, 10):  # as a horizontal table: T fits 16 bits; as a vertical one: the sum fits 32 bits whatever 16-bit T it meets
        assert ((a * ((1 << depth) - 1) + 512) >> 10) + 1 <= 32767
    assert a * 32767 + (1 << 17) <= 2 ** 31 - 1
    plane_sn = src_n // 2 if kind else src_n
    assert first.min() >= -ntaps and first.max() <= plane_sn  # (taps stay next to the plane: what lies outside is read clamped)
    assert (np.diff(first) >= 0).all()  # (a tile's window runs from its first column's first tap to its last column's last)


@pytest.mark.parametrize("n", (2, 64, 70, 8192))
def test_the_identity_table_is_the_identity(n):
    for kind in (0, 1):
        first, coef, ntaps = library_table(n, n, kind)
        rows = n // 2 if kind else n
        tap = np.arange(rows)[:, None] - first[:, None] == np.arange(ntaps)[None, :]  # the tap that lands on the row's own index
        assert tap.sum(axis=1).tolist() == [1] * rows
        assert (coef[tap] == 1 << 14).all() and (coef[~tap] == 0).all()


def test_a_refused_length_is_an_error_not_a_table():
    from xeve_amd import lib

    L = lib.load()
    first, coef, ntaps = (C.c_int32 * 64)(), (C.c_int16 * (64 * 33))(), C.c_int()
    for src_n, dst_n, kind in ((0, 2, 0), (2, 0, 0), (18, 2, 0), (2, 18, 0), (8194, 8194, 0), (16, 2, 2), (16, 2, -1), (15, 2, 1), (16, 3, 1), (-4, 4, 0)):
        assert L.xeve_hip_scale_filter(src_n, dst_n, kind, first, coef, 64 * 33, C.byref(ntaps)) == -2 and "invalid argument" in lib.last_error(), (src_n, dst_n, kind)
    assert L.xeve_hip_scale_filter(16, 2, 0, None, coef, 64 * 33, C.byref(ntaps)) == -2
    assert L.xeve_hip_scale_filter(16, 2, 0, first, None, 64 * 33, C.byref(ntaps)) == -2
    assert L.xeve_hip_scale_filter(16, 2, 0, first, coef, 64 * 33, None) == -2
    assert L.xeve_hip_scale_filter(16, 2, 0, first, coef, 63, C.byref(ntaps)) == -2 and "needs room for 64 coefficients" in lib.last_error()  # (2 rows of 32)
    assert L.xeve_hip_scale_filter(16, 2, 0, first, coef, 64, C.byref(ntaps)) == 0 and ntaps.value == 32


def test_the_leaf_refuses_before_the_library_is_bound():
    """the surface entry point needs xeve_hip_init (XEVE_HIP_ERR_UNINIT); the table function does not (a fresh process, no GPU)"""
    code = ("import ctypes as C\nfrom xeve_amd import lib, encode\nL = lib.load()\ns = lib.Surface(1, 1, 8, 0)\n"
            "print(L.xeve_hip_surface_to_yuv420(C.byref(s), 4, 4, 0, 4, 4, 8, 1, None, 24, None), encode.scale_filter(4, 2, 0)[2])")
    r = subprocess.run([os.sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.split() == ["-3", "8"], (r.stdout, r.stderr[-2000:])


# ---- scale_core.h on the host ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program():
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                               "-o", OUT, SRC])  # (the runtimes linked in: the program needs nothing preloaded)
    return OUT


SIZES = [((2, 2), (2, 2)), ((16, 16), (2, 2)), ((2, 2), (16, 16)), ((70, 50), (62, 36)), ((202, 138), (130, 66)), ((128, 18), (34, 70)), ((70, 50), (70, 50))]


def _jobs():
    rng = np.random.default_rng(31)
    jobs = []
    for n, (((sw, sh), (w, h)), layout, fmt) in enumerate(itertools.product(SIZES, ("nv", "planar"), K.FORMATS)):
        kind, siting, extra = K.CONTENTS[n % 3], K.SITINGS[(n // 3) % 2], (0, 6)[(n // 2) % 2]
        planes, blocks, pl, pc = K.surface(rng, sw, sh, layout, fmt, kind, extra, poison=rng.integers(0, 256))
        jobs.append(dict(layout=layout, fmt=fmt, siting=siting, sw=sw, sh=sh, w=w, h=h, kind=kind, extra=extra, planes=planes, blocks=blocks, pl=pl, pc=pc))
    return jobs


def test_the_lane_code_equals_the_restatement(program, tmp_path):
    jobs = _jobs()
    src, dst = os.path.join(str(tmp_path), "jobs.bin"), os.path.join(str(tmp_path), "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<q", len(jobs)))
        for j in jobs:
            sb, depth, shift = K.FORMATS[j["fmt"]]
            f.write(struct.pack("<13q", int(j["layout"] == "nv"), sb, depth, shift, K.SITINGS.index(j["siting"]), j["sw"], j["sh"], j["w"], j["h"], j["pl"] * sb, j["pc"] * sb,
                                j["blocks"][0].nbytes, j["blocks"][1].nbytes))
            for b in j["blocks"]:
                f.write(b.tobytes())
    r = subprocess.run([program, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    got = open(dst, "rb").read()
    at = 0
    for j in jobs:
        key = {k: j[k] for k in ("layout", "fmt", "siting", "sw", "sh", "w", "h", "kind", "extra")}
        raw = K.frame(*j["planes"], j["w"], j["h"], j["siting"], K.FORMATS[j["fmt"]][1]).tobytes()
        assert got[at:at + len(raw)] == raw, key
        if (j["sw"], j["sh"]) == (j["w"], j["h"]):  # a same-size call is de-interleave, shift and pitch removal
            assert raw == np.concatenate([p.reshape(-1) for p in j["planes"]]).astype(np.uint8 if K.FORMATS[j["fmt"]][1] == 8 else "<u2").tobytes(), key
        at += len(raw)
    assert at == len(got)
