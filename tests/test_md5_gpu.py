"""xeve_hip_md5_planes on the GPU (xeve_amd/csrc/md5.hip, a lane per message) against hashlib, over the messages of tests/_md5_cases.py: lengths around both padding
branches, rows that straddle 64-byte blocks, rows `stride` > w apart with fill between them, a base at an odd sample offset, 130 jobs of mixed lengths in one launch,
the same launch twice, one 1920x1080 luma plane.  tests/test_md5_core_host.py holds the same lane code to the same messages on the host."""
import ctypes as C

import numpy as np
import pytest

import _md5_cases as M

# gpu_full (XEVE_GPU_FULL=1): the default GPU suite is held to the seconds recorded in tests/golden/gpu_suite_durations.json, a file this change leaves as it is
pytestmark = [pytest.mark.gpu, pytest.mark.gpu_full]


@pytest.fixture(scope="module")
def L():
    import xeve_amd
    from xeve_amd import lib

    xeve_amd.init(0)
    return lib.load()


def digests(L, jobs, samples, shift=0, guard=64):
    """the leaf's digests of `jobs` over `samples`; shift = 1: base one sample into the buffer (2-byte aligned only), offsets counted from there.  The digests lie between
    two guards the call must leave as they were"""
    import torch

    from xeve_amd import lib

    dev = torch.device("cuda:0")
    d_samples = torch.from_numpy(samples.view(np.int16)).to(dev)
    d_jobs = torch.from_numpy(M.records(jobs, shift).view(np.uint8).copy()).to(dev)
    out = torch.full((guard + 16 * len(jobs) + guard,), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    lib.check(L.xeve_hip_md5_planes(C.c_void_p(d_samples.data_ptr() + 2 * shift), C.c_void_p(d_jobs.data_ptr()), len(jobs), C.c_void_p(out.data_ptr() + guard), None))
    torch.cuda.synchronize()
    got = out.cpu().numpy().tobytes()
    assert got[:guard] == got[-guard:] == b"\xa5" * guard, "written outside digests[0 .. njobs * 16)"
    return [got[guard + 16 * i:guard + 16 * i + 16] for i in range(len(jobs))]


@pytest.fixture(scope="module")
def small():
    jobs, samples = M.small_cases()
    return jobs, samples, [M.expected(samples, j) for j in jobs]


def test_padding_branches_straddling_rows_strides_and_alignments(L, small):
    jobs, samples, want = small
    got = digests(L, jobs, samples)
    for j, g, w in zip(jobs, got, want):
        assert g == w, j
    shapes = {(w, h) for _, _, w, h in jobs}
    assert set(M.PADDING_SHAPES + M.STRADDLE_SHAPES) <= shapes


def test_a_base_at_an_odd_sample_offset(L, small):
    jobs, samples, want = small
    assert digests(L, jobs, samples, shift=1) == want


def test_each_shape_alone(L, small):
    """a launch of one job: a wave with one live lane"""
    jobs, samples, want = small
    for i in range(0, 3 * len(M.PADDING_SHAPES + M.STRADDLE_SHAPES), 3):
        assert digests(L, jobs[i:i + 1], samples) == want[i:i + 1], jobs[i]


def test_130_mixed_jobs_in_one_launch_twice(L):
    jobs, samples = M.mixed_cases(130)
    want = [M.expected(samples, j) for j in jobs]
    first = digests(L, jobs, samples)
    assert first == want
    assert digests(L, jobs, samples) == first


def test_a_1080p_luma_plane(L):
    """64800 blocks, rows of 60 whole blocks on 16-byte boundaries inside a padded store; beside it the same plane one sample further on (no 4-byte alignment: the
    sample-by-sample reader over the same length)"""
    jobs, samples = M.luma_1080p_case()
    assert len(jobs) == 2 and jobs[0][2:] == (1920, 1080)
    assert digests(L, jobs, samples) == [M.expected(samples, j) for j in jobs]


def test_arguments_are_checked(L):
    from xeve_amd import lib

    jobs, samples = M.mixed_cases(2)
    with pytest.raises(lib.XeveHipError, match="invalid argument"):
        lib.check(L.xeve_hip_md5_planes(None, None, 1, None, None))
    import torch

    d = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(lib.XeveHipError, match="invalid argument"):
        lib.check(L.xeve_hip_md5_planes(C.c_void_p(d.data_ptr()), C.c_void_p(d.data_ptr()), 0, C.c_void_p(d.data_ptr()), None))
    with pytest.raises(lib.XeveHipError, match="invalid argument"):
        lib.check(L.xeve_hip_md5_planes(C.c_void_p(d.data_ptr() + 1), C.c_void_p(d.data_ptr()), 1, C.c_void_p(d.data_ptr()), None))
