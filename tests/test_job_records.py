"""The 32-bit job records that address the stacked originals of a batch (xeve_amd/csrc/xh_common.h: xh_make_job / xh_job, xh_make_pred_off / xh_pred_off), on the CPU:
the functions are __host__ __device__ and tests/native/job_record_host.cpp builds their host side.  Every consumer kernel (sad.hip, tq.hip, dct_mfma.hip, mc.hip)
decodes a record through them, so a wrong decode at 2^31, 2^32 or 2^33 samples shows here without a GPU; tests/test_hip_batched.py holds the kernels to it.

No C-ABI entry point checks its arguments before the device is initialised (XH_ENTER precedes every XH_REQUIRE and xeve_hip_init needs a GPU), so the refusal of a
dense operand of 2^30 elements or more is tested on the guard the entry points call (xh_dense_ok), and the guards' presence in the four entry points by reading them."""
import ctypes as C
import os
import re
import subprocess

import pytest

from _libs import ROOT

SRC = os.path.join(ROOT, "tests", "native", "job_record_host.cpp")
HDR = os.path.join(ROOT, "xeve_amd", "csrc", "xh_common.h")
OUT = os.path.join(ROOT, "tests", "native", "build", "libjob_record_host.so")
HIPCC = "/opt/rocm/bin/hipcc"

INT_MIN = -2 ** 31
OFFSETS = [0, 2, 1, 2 ** 31 - 2, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 2, 2 ** 33 - 2]
OFF2S = [0, 1, 2 ** 30 - 1, 2 ** 30, 2 ** 30 + 1, 2 ** 31 - 1, -1, -2 ** 30, INT_MIN]
NONE = (-1, INT_MIN)  # XH_JOB_NONE


def in_domain(o, off2):
    """the header comment's domain of xh_make_job, restated: off2 = INT_MIN + 1 .. 2^30 - 1; an even o with a non-negative off2 travels halved (below 2^33), every
    other o as it is (below 2^32)"""
    if not INT_MIN < off2 < 2 ** 30:
        return False
    return o < (2 ** 33 if o % 2 == 0 and off2 >= 0 else 2 ** 32)


@pytest.fixture(scope="module")
def jr():
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", OUT, SRC], check=True)
    L = C.CDLL(OUT)
    i32, u64, i64, p32 = C.c_int32, C.c_uint64, C.c_int64, C.POINTER(C.c_int32)
    L.jr_make_job.argtypes, L.jr_make_job.restype = [u64, i32, p32], None
    L.jr_make_job_yx.argtypes, L.jr_make_job_yx.restype = [i64, i64, i64, i32, p32], None
    L.jr_job.argtypes, L.jr_job.restype = [i32, i32, C.POINTER(u64), p32], None
    L.jr_u.argtypes, L.jr_u.restype = [i32], u64
    L.jr_job_ok.argtypes, L.jr_job_ok.restype = [u64, i32], C.c_int
    L.jr_dense_ok.argtypes, L.jr_dense_ok.restype = [i64, i64], C.c_int
    L.jr_make_pred_off.argtypes, L.jr_make_pred_off.restype = [u64, p32], None
    L.jr_pred_off.argtypes, L.jr_pred_off.restype = [i32, i32], u64

    class J:
        HALF2, HALFF, OFF = L.jr_off2_half(), L.jr_frac_half(), L.jr_frac_off()

        @staticmethod
        def make(o, off2):
            r = (i32 * 2)()
            L.jr_make_job(o, off2, r)
            return r[0], r[1]

        @staticmethod
        def make_yx(y, s, x, off2):
            r = (i32 * 2)()
            L.jr_make_job_yx(y, s, x, off2, r)
            return r[0], r[1]

        @staticmethod
        def job(off1, off2):
            o, o2 = u64(), i32()
            L.jr_job(off1, off2, C.byref(o), C.byref(o2))
            return o.value, o2.value

        @staticmethod
        def make_pred(o):
            r = (i32 * 2)()
            L.jr_make_pred_off(o, r)
            return r[0], r[1]

        u, ok, dense_ok, pred = staticmethod(L.jr_u), staticmethod(L.jr_job_ok), staticmethod(L.jr_dense_ok), staticmethod(L.jr_pred_off)

    assert (J.HALF2, J.HALFF, J.OFF) == (1 << 30, 1 << 8, 4)
    return J


def s32(v):
    """the int32 a record holds for the unsigned 32-bit value v"""
    return v - 2 ** 32 if v >= 2 ** 31 else v


def test_a_record_of_the_librarys_making_decodes_to_the_block_it_was_made_for(jr):
    made = {}
    for o in OFFSETS:
        for off2 in OFF2S:
            rec = jr.make(o, off2)
            assert bool(jr.ok(o, off2)) == in_domain(o, off2), (o, off2)
            if in_domain(o, off2):
                assert jr.job(*rec) == (o, off2), (o, off2, rec)
                assert rec != NONE
                made[rec] = (o, off2)
            else:  # refused: the one record no pair of the domain makes, so it aliases no block a launch addresses
                assert rec == NONE, (o, off2, rec)
    assert len(made) == sum(in_domain(o, off2) for o in OFFSETS for off2 in OFF2S)  # (no two pairs of the domain share a record)
    assert not in_domain(*jr.job(*NONE))
    # which pairs those are: everything below 2^32 with an off2 a caller may write, the even offsets up to 2^33 - 2 where off2 is not negative -- and no off2 of
    # 2^30 .. 2^31 - 1 (bit 30 is the mark) at any offset
    assert [o for o in OFFSETS if in_domain(o, 0)] == [o for o in OFFSETS if o % 2 == 0 or o < 2 ** 32] == OFFSETS
    assert [o for o in OFFSETS if in_domain(o, -1)] == [o for o in OFFSETS if o < 2 ** 32]
    assert not any(in_domain(o, off2) for o in OFFSETS for off2 in (2 ** 30, 2 ** 30 + 1, 2 ** 31 - 1, INT_MIN))
    # the halved form is what reaches past 2^32, and the (y, stride, x) form the kernels call does its row arithmetic in 64 bits
    assert jr.make(2 ** 33 - 2, 5) == (-1, 5 | jr.HALF2) and jr.make(2 ** 32, 0) == (s32(2 ** 31), jr.HALF2) and jr.make(2 ** 32 - 1, 7) == (-1, 7)
    s, y, x = 1312, (2 ** 33 - 2) // 1312, (2 ** 33 - 2) % 1312
    assert jr.job(*jr.make_yx(y, s, x, 9)) == (2 ** 33 - 2, 9)
    assert jr.make_yx(-1, s, 0, 0) == NONE  # (a negative offset is no offset)


def test_a_callers_record_decodes_to_itself(jr):
    """include/xeve_hip.h: any off1 of 0 .. 2^32 - 1, odd ones too, with an unmarked off2 -- negative or below 2^30"""
    for o in [o for o in OFFSETS if o < 2 ** 32] + [3, 2 ** 31 - 1, 2 ** 31 + 1, 2 ** 32 - 3]:
        for off2 in (0, 1, 2 ** 30 - 1, -1, -2 ** 30, INT_MIN + 1):
            assert jr.job(s32(o), off2) == (o, off2), (o, off2)
        assert jr.u(s32(o)) == o
    # and a marked one to twice its off1 with the mark taken off
    for h in (0, 1, 2 ** 30, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 4, 2 ** 32 - 1):
        assert jr.job(s32(h), 12345 | jr.HALF2) == (2 * h, 12345)


def test_the_fused_comparisons_pred_off_pair(jr):
    """mc.hip: k_spel_make builds (pred_off, frac) with xh_make_pred_off, the fused kernel reads it with xh_pred_off"""
    seen = {}
    for o in OFFSETS + [3, 2 ** 31 - 1, 2 ** 31 + 1, 2 ** 32 + 1, 2 ** 33 - 1, 2 ** 33, 2 ** 33 + 2, 2 ** 34, 2 ** 63]:
        po, frac = jr.make_pred(o)
        if o < (2 ** 33 if o % 2 == 0 else 2 ** 32):
            assert frac == (jr.HALFF if o % 2 == 0 else 0) and jr.pred(po, frac | 3 | (5 << 3)) == o, (o, po, frac)  # (filter and plane bits of frac do not count)
            assert (po, frac) not in seen
            seen[(po, frac)] = o
        else:  # refused: a job that is switched off reads no block at all
            assert (po, frac) == (0, jr.OFF), (o, po, frac)
    # a caller's own pred_off (include/xeve_hip.h xeve_hip_mc_job): unsigned, unmarked
    for o in (0, 1, 2, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1):
        assert jr.pred(s32(o), 3) == o
        assert jr.pred(s32(o), 3 | jr.HALFF) == 2 * o


def test_a_dense_second_operand_of_a_gigasample_is_refused(jr):
    """bit 30 of off2 is the mark, so the dense buffers whose block offsets (j * n0, t * n0, c * cu * cu) become off2 stay below 2^30 elements: xh_dense_ok is what the
    host entry points that size them require, before anything is launched"""
    for n in (16, 64, 256, 1024, 4096):
        assert jr.dense_ok(2 ** 30 // n - 1, n) and not jr.dense_ok(2 ** 30 // n, n) and not jr.dense_ok(2 ** 30 // n + 1, n)
        assert jr.job(*jr.make(2 ** 33 - 2, (2 ** 30 // n - 2) * n)) == (2 ** 33 - 2, (2 ** 30 // n - 2) * n)  # (the last block of the largest buffer accepted)
    assert jr.dense_ok(0, 4096) and jr.dense_ok(5, 0) and not jr.dense_ok(-1, 16) and not jr.dense_ok(2 ** 40, 2 ** 40)
    assert jr.dense_ok(3, 2 ** 30 // 3) and not jr.dense_ok(3, 2 ** 30 // 3 + 1)
    # every entry point whose kernels call xh_make_job with a dense offset requires it
    need = {"rdo.hip": 2, "inter.hip": 1, "intra.hip": 1, "tree.hip": 1}
    for f, n in need.items():
        src = open(os.path.join(ROOT, "xeve_amd", "csrc", f)).read()
        assert len(re.findall(r"XH_REQUIRE\(xh_dense_ok\(", src)) >= n, f
