"""Test infrastructure: builds and loads the HOST side of xeve_amd/csrc/sbac_lane.h and eco_lane.h (the lane coder and the lane-serial bitstream writer that
libxeve_hip.so runs on the device, every function __host__ __device__) so that the CPU suite can compare it bit for bit with the oracle.  hipcc --cuda-host-only;
nothing of this is linked into the product library."""
import ctypes as C
import os
import subprocess

import numpy as np

from _libs import ROOT, c_int, c_void_p, oracle

SRC = os.path.join(ROOT, "tests", "native", "sbac_lane_host.cpp")
HDR = os.path.join(ROOT, "xeve_amd", "csrc", "sbac_lane.h")
HDR2 = os.path.join(ROOT, "xeve_amd", "csrc", "eco_lane.h")
OUT = os.path.join(ROOT, "tests", "native", "build", "libsbac_lane_host.so")
HIPCC = "/opt/rocm/bin/hipcc"


_lib = None


def available():
    return os.path.exists(HIPCC)


def lane():
    global _lib
    if _lib is None:
        if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(SRC), os.path.getmtime(HDR), os.path.getmtime(HDR2)):
            os.makedirs(os.path.dirname(OUT), exist_ok=True)
            subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-o", OUT, SRC], check=True)
        _lib = C.CDLL(OUT)
        _lib.xl_host_eco_ctu.restype = c_int
        _lib.xl_host_eco_ctu.argtypes = [c_int] * 8 + [c_void_p] * 9 + [c_int, c_int, c_void_p, c_int]
        _lib.xl_host_eco_tile_end.restype = c_int
        _lib.xl_host_eco_tile_end.argtypes = [c_void_p, c_void_p, c_int]
    return _lib


_scans = None


def scans():
    """zig-zag scans of the 16x16, 32x32, 64x64 blocks (xeve_tbl_scan) from the oracle's xo_zigzag"""
    global _scans
    if _scans is None:
        O = oracle()
        O.xo_zigzag.restype = None
        O.xo_zigzag.argtypes = [c_int, c_int, c_void_p]
        _scans = []
        for l in (4, 5, 6):
            a = np.zeros(1 << (2 * l), np.uint16)
            O.xo_zigzag(l, l, a.ctypes.data)
            _scans.append(a)
    return _scans
