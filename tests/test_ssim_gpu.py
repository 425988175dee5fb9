"""xeve_hip_ssim_planes on the GPU (xeve_amd/csrc/ssim.hip): the per-picture, per-plane SSIM sums EQUAL to the numpy restatement (tests/_ssim.py) -- on the encoder's
geometry, at sizes whose last block column / row is partly outside the window, at one block more than the kernel's tile either way, over every content class of the host
program, at picture distances past 2^32 samples -- and every refusal of the contract."""
import ctypes as C

import numpy as np
import pytest

import _ssim as S

# gpu_full (XEVE_GPU_FULL=1): as tests/test_recon_gpu.py, kept out of the default GPU suite and its recorded durations (tests/golden/gpu_suite_durations.json)
pytestmark = [pytest.mark.gpu, pytest.mark.gpu_full]

GUARD = -0x7ABC
TILE = (32, 16)  # ssim.hip's SS_TX x SS_TY: a workgroup's tile in 4x4 blocks (128 x 64 samples, 31 x 15 windows)
# one block wider / taller than the tile in luma (132 / 68 samples), and in chroma (264 / 136 luma samples: several luma tiles each way)
BEYOND_TILE = [(4 * (TILE[0] + 1), 4 * TILE[1]), (4 * TILE[0], 4 * (TILE[1] + 1)), (8 * (TILE[0] + 1), 8 * (TILE[1] + 1))]
SIZES = [(16, 16), (18, 16), (16, 22), (24, 40), (70, 50), (136, 72), (352, 288)] + BEYOND_TILE


@pytest.fixture(scope="module")
def dev():
    import torch

    import xeve_amd

    xeve_amd.init(0)
    return torch.device("cuda:0")


def _ptrs(addresses):
    return (C.c_void_p * 3)(*addresses)


def _call(rec, s_rec, rec_pic, org, s_org, org_pic, w, h, npics, sums):
    """rec / org: three device addresses; s_*, *_pic: (luma, chroma) in samples; sums: a device address -> the return code"""
    import torch

    from xeve_amd import lib

    rc = lib.load().xeve_hip_ssim_planes(_ptrs(rec), s_rec[0], s_rec[1], rec_pic[0], rec_pic[1], _ptrs(org), s_org[0], s_org[1], org_pic[0], org_pic[1], w, h, npics, sums, None)
    torch.cuda.synchronize()
    return rc


class Planes:
    """npics stacked pictures: plane c at `lead` samples into a buffer of its own (luma 16-byte, chroma only 8-byte aligned), rows `stride` apart, pictures
    rows * stride + gap apart; the windows hold `content`, everything between and behind them is random"""

    def __init__(self, rng, dev, w, h, npics, strides, windows, gaps=(40, 20), lead=(8, 4)):
        import torch

        self.strides, self.dist, self.lead = strides, (h * strides[0] + gaps[0], (h // 2) * strides[1] + gaps[1]), lead
        self.host, self.dev = [], []
        for c in range(3):
            pw, ph, s, d, at = (w, h, strides[0], self.dist[0], lead[0]) if c == 0 else (w // 2, h // 2, strides[1], self.dist[1], lead[1])
            a = rng.integers(0, 1024, size=at + npics * d, dtype=np.int16)
            for p in range(npics):
                np.lib.stride_tricks.as_strided(a[at + p * d:], (ph, pw), (2 * s, 2))[:] = windows[p][c]
            self.host.append(a), self.dev.append(torch.from_numpy(a).to(dev))

    def addresses(self):
        return [t.data_ptr() + 2 * self.lead[c > 0] for c, t in enumerate(self.dev)]

    def unchanged(self):
        return all(np.array_equal(t.cpu().numpy(), a) for t, a in zip(self.dev, self.host))


def _pictures(rng, kind, w, h, npics):
    """per picture the three (rec, org) plane pairs of one content class"""
    return [[S.content(rng, kind, pw, ph) for pw, ph in ((w, h), (w // 2, h // 2), (w // 2, h // 2))] for _ in range(npics)]


@pytest.mark.parametrize("w,h", SIZES)
def test_sums_equal_the_restatement(w, h, dev):
    """the encoder's geometry (stores w + 288 / w / 2 + 144 wide, originals w / w / 2 rounded up to 8 / 4), picture distances with a gap, one and three pictures, every
    content class; guard words around `sums` stay as they were and are not added to, the inputs are only read"""
    import torch

    rng = np.random.default_rng(w * 1000 + h)
    wl = (w + 7) & ~7
    for npics in (1, 3):
        for kind in S.CONTENTS:
            pics = _pictures(rng, kind, w, h, npics)
            rec = Planes(rng, dev, w, h, npics, (wl + 288, wl // 2 + 144), [[pl[0] for pl in p] for p in pics])
            org = Planes(rng, dev, w, h, npics, (wl, wl // 2), [[pl[1] for pl in p] for p in pics], gaps=(8, 4))
            want = np.full(2 + npics * 3, GUARD, np.int64)
            for p in range(npics):
                want[1 + 3 * p:4 + 3 * p] = [S.plane_sum(a, b) for a, b in pics[p]]
            sums = torch.full((2 + npics * 3,), GUARD, dtype=torch.int64, device=dev)  # (what stands there before must not be added to)
            assert _call(rec.addresses(), rec.strides, rec.dist, org.addresses(), org.strides, org.dist, w, h, npics, sums.data_ptr() + 8) == 0
            got = sums.cpu().numpy()
            assert np.array_equal(got, want), (npics, kind, got, want)
            if kind in ("identical", "all_max"):
                assert got[1:4].tolist() == [n << 30 for n in (S.windows(w, h), S.windows(w // 2, h // 2), S.windows(w // 2, h // 2))]
            if kind == "checkerboard":
                assert (got[1:-1] < 0).all()
            assert rec.unchanged() and org.unchanged()


def test_the_python_face_takes_the_recon_layout(dev):
    """encode.ssim_planes over pictures as recon() hands them out: in place at a width that is a multiple of 8, through aligned copies at 70x50"""
    import torch

    from xeve_amd import encode

    rng = np.random.default_rng(9)
    for w, h in ((72, 56), (70, 50)):
        pics = _pictures(rng, "noisy", w, h, 3)
        rec, org = (torch.from_numpy(np.stack([np.concatenate([pl[k].reshape(-1) for pl in p]) for p in pics])).to(dev) for k in (0, 1))
        want = [[S.plane_sum(a, b) for a, b in p] for p in pics]
        assert encode.ssim_planes(rec, org, w, h).cpu().tolist() == want
        assert encode.ssim_planes(rec[1], org[1].view(torch.uint8), w, h).cpu().tolist() == want[1]
        assert encode.ssim_windows(w, h) == [S.windows(w, h), S.windows(w // 2, h // 2), S.windows(w // 2, h // 2)]


FAR_DIST = 2 ** 32 + 4096  # samples between the pictures: past what 32 bits hold, and a truncated distance (4096) lands inside picture 0's luma window -- a mismatch, not a fault


def test_picture_distances_past_2_to_the_32(dev):
    """three 64x64 pictures, reconstruction AND original, FAR_DIST samples apart inside one allocation that nothing fills (17 GB, touched at the three windows only),
    distinct data at each: the sums per picture against the restatement"""
    import torch

    w = h = 64
    s_rec, s_org = (w + 288, w // 2 + 144), (w, w // 2)
    at_rec, at_org = (0, 32768, 49152), (65536, 65536 + 8192, 65536 + 12288)  # where the planes of picture 0 start (luma windows 22528 / 4096 samples, chroma 5632 / 1024)
    window = 131072
    free = torch.cuda.mem_get_info()[0]
    need = 2 * (2 * FAR_DIST + window)
    assert free > need + (1 << 30), "the device's free memory does not hold the far allocation (%d of %d bytes)" % (free, need)
    base = torch.empty(2 * FAR_DIST + window, dtype=torch.int16, device=dev)
    try:
        rng = np.random.default_rng(64)
        host = []
        for p in range(3):  # an original of noise and a reconstruction a few steps off it, so that a picture's sums are far from those of a mixed-up pair
            a = rng.integers(0, 1024, size=window, dtype=np.int16)
            for c in range(3):
                pw, ph = (w, h) if c == 0 else (w // 2, h // 2)
                o = np.lib.stride_tricks.as_strided(a[at_org[c]:], (ph, pw), (2 * s_org[c > 0], 2))
                np.lib.stride_tricks.as_strided(a[at_rec[c]:], (ph, pw), (2 * s_rec[c > 0], 2))[:] = np.clip(o + rng.integers(-9, 10, (ph, pw)), 0, 1023)
            host.append(a)
            base[p * FAR_DIST:p * FAR_DIST + window].copy_(torch.from_numpy(a).to(dev))

        def plane(p, at, c, s):
            pw, ph = (w, h) if c == 0 else (w // 2, h // 2)
            return np.lib.stride_tricks.as_strided(host[p][at[c]:], (ph, pw), (2 * s[c > 0], 2)).astype(np.int64)

        sums = torch.zeros(9, dtype=torch.int64, device=dev)
        assert _call([base.data_ptr() + 2 * a for a in at_rec], s_rec, (FAR_DIST, FAR_DIST), [base.data_ptr() + 2 * a for a in at_org], s_org, (FAR_DIST, FAR_DIST), w, h, 3,
                     sums.data_ptr()) == 0
        got = sums.cpu().numpy().reshape(3, 3)
        want = [[S.plane_sum(plane(p, at_rec, c, s_rec), plane(p, at_org, c, s_org)) for c in range(3)] for p in range(3)]
        assert got.tolist() == want and len({tuple(r) for r in want}) == 3
        for p in range(3):  # only read
            assert np.array_equal(base[p * FAR_DIST:p * FAR_DIST + window].cpu().numpy(), host[p]), p
    finally:
        base = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()  # (the encodes behind this file need the memory)


def test_arguments_outside_the_contract_are_refused(dev):
    """odd or undersized w / h, sizes past the largest picture, a stride below the window rounded up, strides and distances that break the rows' alignment, a misaligned
    plane, npics 0 and 65536, a missing plane, host memory for a plane or for the sums: XEVE_HIP_ERR_ARG before any launch"""
    import torch

    from xeve_amd import lib

    t = torch.zeros(8192, dtype=torch.int16, device=dev)
    sums = torch.full((5,), GUARD, dtype=torch.int64, device=dev)
    host = np.zeros(8192, np.int16)
    a = [t.data_ptr()] * 3
    good = dict(rec=a, org=a, w=24, h=16, s=(24, 12), s_org=(24, 12), pic=(0, 0), npics=1, sums=sums.data_ptr() + 8)
    assert _call(good["rec"], good["s"], good["pic"], good["org"], good["s_org"], good["pic"], 24, 16, 1, good["sums"]) == 0  # (the base case itself is accepted)
    sums.fill_(GUARD)
    for kw in (dict(w=17), dict(h=17), dict(w=14), dict(h=14), dict(w=8194), dict(h=4322), dict(s=(16, 12)), dict(s=(24, 8)), dict(s_org=(16, 12)), dict(s_org=(24, 8)),
               dict(w=18, s=(18, 12)), dict(w=18, s=(24, 10)), dict(pic=(4, 0)), dict(pic=(0, 2)), dict(pic=(-8, 0)), dict(rec=[a[0] + 8] + a[1:]), dict(rec=a[:2] + [a[2] + 4]),
               dict(org=[a[0], a[1] + 2, a[2]]), dict(npics=0), dict(npics=65536), dict(rec=[a[0], 0, a[2]]), dict(org=[0] + a[1:]), dict(sums=None), dict(sums=sums.data_ptr() + 4),
               dict(rec=[host.ctypes.data] + a[1:]), dict(org=a[:2] + [host.ctypes.data]), dict(sums=np.zeros(3, np.int64).ctypes.data)):
        k = dict(good, **kw)
        rc = _call(k["rec"], k["s"], k["pic"], k["org"], k["s_org"], k["pic"], k["w"], k["h"], k["npics"], k["sums"])
        assert rc == -2 and "invalid argument" in lib.last_error(), kw
    assert (sums.cpu().numpy() == GUARD).all()
