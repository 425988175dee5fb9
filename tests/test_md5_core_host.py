"""CPU suite: xeve_amd/csrc/md5_core.h -- the per-lane code of the MD5 kernel (md5.hip: transform, the gather of a 64-byte block across row boundaries, the finish with
both padding branches) -- compiled for the host and held to hashlib over the shapes tests/test_md5_gpu.py holds the kernel to.  tests/native/md5_host.cpp is a
stand-alone program built with the address and undefined-behaviour sanitizers and run as a child process: its samples lie in a heap block of exactly their size, so a
read outside what a job describes is a report and a failed run."""
import os
import struct
import subprocess

import pytest

import _md5_cases as M
from _libs import ROOT

SRC = os.path.join(ROOT, "tests", "native", "md5_host.cpp")
HDR = os.path.join(ROOT, "xeve_amd", "csrc", "md5_core.h")
OUT = os.path.join(ROOT, "tests", "native", "build", "md5_host")


@pytest.fixture(scope="module")
def program():
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                               "-o", OUT, SRC])  # (the runtimes linked in: the program needs nothing preloaded and does not mind what its environment preloads)
    return OUT


def run(program, tmp_path, jobs, samples):
    p = os.path.join(tmp_path, "jobs.bin")
    with open(p, "wb") as f:
        f.write(struct.pack("<qq", len(jobs), len(samples)))
        f.write(M.records(jobs).tobytes())
        f.write(samples.astype("<u2").tobytes())
    r = subprocess.run([program, p], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    got = r.stdout.split()
    assert len(got) == len(jobs)
    return [bytes.fromhex(x) for x in got]


@pytest.mark.parametrize("cases", [M.small_cases, M.mixed_cases, M.luma_1080p_case], ids=lambda f: f.__name__)
def test_the_lane_code_gives_hashlibs_digests(cases, program, tmp_path):
    jobs, samples = cases()
    got = run(program, str(tmp_path), jobs, samples)
    for j, g in zip(jobs, got):
        assert g == M.expected(samples, j), j


def test_the_shapes_cover_every_branch():
    """what the lists are there for: messages of one block and of the two-block finish, an exact multiple of the block, rows shorter than a block, and each path of
    the reader (whole blocks at 16-, 4- and 2-byte alignment, blocks across a row's end)"""
    jobs, _ = M.small_cases()
    rem = {(w * h) % 32 for _, _, w, h in jobs}
    assert {0, 1, 27, 28, 31} <= rem
    assert any(w * h == 32 for _, _, w, h in jobs) and any(w * h == 64 for _, _, w, h in jobs)
    assert any(w < 32 and h > 1 for _, _, w, h in jobs)
    wide = [(2 * off, 2 * stride) for off, stride, w, h in jobs if w >= 64 and h > 1]  # byte addresses of rows that hold whole blocks
    assert any(a % 16 == 0 and s % 16 == 0 for a, s in wide) and any(a % 16 and a % 4 == 0 and s % 4 == 0 for a, s in wide) and any(a % 4 == 2 and s % 4 == 0 for a, s in wide)
    assert any(stride > w and h > 1 for _, stride, w, h in jobs)
