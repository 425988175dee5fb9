"""xeve_hip_recon_measure on the GPU (xeve_amd/csrc/recon.hip): the packed copy of the stacked pictures' interiors and the per-picture, per-plane sums of squared
differences, both EXACT against numpy -- at the picture sizes where a row is 8, 12, 36, 68 ... samples and only the promised alignment holds (luma 16 bytes, chroma 8),
with sums far past 32 bits, and at picture distances past 2^32 samples."""
import ctypes as C

import numpy as np
import pytest

# gpu_full (XEVE_GPU_FULL=1): the default GPU suite is held to the seconds recorded in tests/golden/gpu_suite_durations.json (tests/test_gpu_suite_budget.py), a file of the
# last full run that this change leaves as it is; measured in a run of their own these tests take 3 s together (profiles/recon_measure.md)
pytestmark = [pytest.mark.gpu, pytest.mark.gpu_full]

SENTINEL = 0x7ABC


@pytest.fixture(scope="module")
def dev():
    import torch

    import xeve_amd

    xeve_amd.init(0)
    return torch.device("cuda:0")


def _ptrs(addresses):
    return (C.c_void_p * 3)(*addresses)


def _call(rec, s_rec, rec_pic, org, s_org, org_pic, w, h, npics, out, out_pic, sse):
    """rec / org: three device addresses (org None: no measurement); s_*, *_pic: (luma, chroma) in samples; out / sse: device addresses or None"""
    import torch

    from xeve_amd import lib

    lib.check(lib.load().xeve_hip_recon_measure(_ptrs(rec), s_rec[0], s_rec[1], rec_pic[0], rec_pic[1], _ptrs(org) if org else None, s_org[0], s_org[1], org_pic[0], org_pic[1],
                                                w, h, npics, out, out_pic, sse, None))
    torch.cuda.synchronize()


class Planes:
    """npics stacked pictures of random 10-bit samples: plane c at `lead[c]` samples into a buffer of its own (luma 16-byte, chroma only 8-byte aligned), rows `stride`
    apart, pictures rows * stride + gap apart; everything between the interiors is random too"""

    def __init__(self, rng, dev, w, h, npics, strides, gaps=(40, 20), lead=(8, 4)):
        import torch

        self.w, self.h, self.npics, self.strides = w, h, npics, strides
        self.dist = (h * strides[0] + gaps[0], (h // 2) * strides[1] + gaps[1])
        self.host, self.dev, self.lead = [], [], lead
        for c in range(3):
            n = lead[c > 0] + npics * self.dist[c > 0]
            a = rng.integers(0, 1024, size=n, dtype=np.int16)
            self.host.append(a), self.dev.append(torch.from_numpy(a).to(dev))

    def addresses(self):
        return [t.data_ptr() + 2 * self.lead[c > 0] for c, t in enumerate(self.dev)]

    def interior(self, pic, c):
        pw, ph, s = (self.w, self.h, self.strides[0]) if c == 0 else (self.w // 2, self.h // 2, self.strides[1])
        at = self.lead[c > 0] + pic * self.dist[c > 0]
        return np.lib.stride_tricks.as_strided(self.host[c][at:], (ph, pw), (2 * s, 2)).astype(np.int64)

    def unchanged(self):
        return all(np.array_equal(t.cpu().numpy(), a) for t, a in zip(self.dev, self.host))


@pytest.mark.parametrize("w,h", [(8, 8), (24, 40), (200, 8), (8, 64), (72, 120), (136, 72), (352, 288)])
def test_copy_and_sums_are_exact_against_numpy(w, h, dev):
    """the encoder's geometry (stores w + 288 / w / 2 + 144 wide, originals w / w / 2), picture distances with a gap, one and three pictures, each of copy only / sums
    only / both; guard words around `out` and `sse` and the gaps between the packed pictures stay as they were, the inputs are only read"""
    import torch

    rng = np.random.default_rng(w * 1000 + h)
    for npics in (1, 3):
        rec, org = Planes(rng, dev, w, h, npics, (w + 288, w // 2 + 144)), Planes(rng, dev, w, h, npics, (w, w // 2), gaps=(8, 4))
        pic, out_pic, guard = w * h * 3 // 2, w * h * 3 // 2 + 8, 8
        want_out = np.full(2 * guard + npics * out_pic, SENTINEL, np.int16)
        want_sse = np.full(2 + npics * 3, -SENTINEL, np.int64)
        for p in range(npics):
            want_out[guard + p * out_pic:guard + p * out_pic + pic] = np.concatenate([rec.interior(p, c).reshape(-1) for c in range(3)]).astype(np.int16)
            for c in range(3):
                want_sse[1 + p * 3 + c] = ((rec.interior(p, c) - org.interior(p, c)) ** 2).sum()
        for copy, measure in ((True, False), (False, True), (True, True)):
            out = torch.full((2 * guard + npics * out_pic,), SENTINEL, dtype=torch.int16, device=dev)
            sse = torch.full((2 + npics * 3,), -SENTINEL, dtype=torch.int64, device=dev)  # (what stands there before must not be added to)
            _call(rec.addresses(), rec.strides, rec.dist, org.addresses() if measure else None, org.strides, org.dist, w, h, npics,
                  out.data_ptr() + 2 * guard if copy else None, out_pic, sse.data_ptr() + 8 if measure else None)
            got_out, got_sse = out.cpu().numpy(), sse.cpu().numpy()
            assert np.array_equal(got_out, want_out if copy else np.full_like(want_out, SENTINEL)), (npics, copy, measure)
            assert np.array_equal(got_sse, want_sse if measure else np.full_like(want_sse, -SENTINEL)), (npics, copy, measure, got_sse, want_sse)
        assert rec.unchanged() and org.unchanged()


@pytest.mark.parametrize("w,h", [(1920, 1080), (8, 4320), (4096, 8)])
def test_sums_past_32_bits_are_exact(w, h, dev):
    """every difference 1023: a luma sum of 1023^2 * w * h (2.17e12 at 1920x1080), a quarter of it per chroma plane -- through many rows of few lanes and few rows of many"""
    import torch

    rec = [torch.full((w * h // (1 if c == 0 else 4),), 1023, dtype=torch.int16, device=dev) for c in range(3)]
    org = [torch.zeros_like(t) for t in rec]
    sse = torch.full((2 * 3,), 5, dtype=torch.int64, device=dev)
    _call([t.data_ptr() for t in rec], (w, w // 2), (0, 0), [t.data_ptr() for t in org], (w, w // 2), (0, 0), w, h, 1, None, 0, sse.data_ptr())
    assert sse.cpu().tolist() == [1023 * 1023 * w * h, 1023 * 1023 * w * h // 4, 1023 * 1023 * w * h // 4, 5, 5, 5]
    again = torch.zeros(3, dtype=torch.int64, device=dev)  # the same bits on every run
    _call([t.data_ptr() for t in rec], (w, w // 2), (0, 0), [t.data_ptr() for t in org], (w, w // 2), (0, 0), w, h, 1, None, 0, again.data_ptr())
    assert again.cpu().tolist() == sse.cpu().tolist()[:3]


FAR_DIST = 2 ** 32 + 4096  # samples between the pictures: past what 32 bits hold, and a truncated distance (4096) lands inside picture 0's luma window -- a mismatch, not a fault


def test_picture_distances_past_2_to_the_32(dev):
    """three 64x64 pictures, reconstruction AND original, FAR_DIST samples apart inside one allocation that nothing fills (17 GB, touched at the three windows only),
    distinct data at each: copy and sums per picture against numpy"""
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
        host = [rng.integers(0, 1024, size=window, dtype=np.int16) for _ in range(3)]
        for p in range(3):
            base[p * FAR_DIST:p * FAR_DIST + window].copy_(torch.from_numpy(host[p]).to(dev))

        def plane(p, at, c, s):
            pw, ph = (w, h) if c == 0 else (w // 2, h // 2)
            return np.lib.stride_tricks.as_strided(host[p][at[c]:], (ph, pw), (2 * s[c > 0], 2)).astype(np.int64)

        pic = w * h * 3 // 2
        out = torch.full((3 * pic,), SENTINEL, dtype=torch.int16, device=dev)
        sse = torch.zeros(9, dtype=torch.int64, device=dev)
        _call([base.data_ptr() + 2 * a for a in at_rec], s_rec, (FAR_DIST, FAR_DIST), [base.data_ptr() + 2 * a for a in at_org], s_org, (FAR_DIST, FAR_DIST), w, h, 3,
              out.data_ptr(), pic, sse.data_ptr())
        got_out, got_sse = out.cpu().numpy().reshape(3, pic), sse.cpu().numpy().reshape(3, 3)
        for p in range(3):
            assert np.array_equal(got_out[p], np.concatenate([plane(p, at_rec, c, s_rec).reshape(-1) for c in range(3)]).astype(np.int16)), p
            assert got_sse[p].tolist() == [int(((plane(p, at_rec, c, s_rec) - plane(p, at_org, c, s_org)) ** 2).sum()) for c in range(3)], p
        for p in range(3):  # only read
            assert np.array_equal(base[p * FAR_DIST:p * FAR_DIST + window].cpu().numpy(), host[p]), p
    finally:
        base = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()  # (the encodes behind this file need the memory)


def test_arguments_outside_the_contract_are_refused(dev):
    """a size that is no multiple of 8, a chroma stride that breaks the 8-byte rows, a misaligned luma pointer, nothing to do: XEVE_HIP_ERR_ARG before any launch"""
    import torch

    from xeve_amd import lib

    t = torch.zeros(4096, dtype=torch.int16, device=dev)
    a, out = [t.data_ptr()] * 3, torch.zeros(4096, dtype=torch.int16, device=dev)
    for kw in (dict(w=12), dict(h=4), dict(s_c=6), dict(rec=[t.data_ptr() + 2] + a[1:]), dict(out=None), dict(npics=0), dict(out_pic=8 * 8 * 3 // 2 - 8)):
        k = dict(dict(w=8, h=8, s_c=4, rec=a, out=out.data_ptr(), npics=1, out_pic=96), **kw)
        rc = lib.load().xeve_hip_recon_measure(_ptrs(k["rec"]), 8, k["s_c"], 0, 0, None, 0, 0, 0, 0, k["w"], k["h"], k["npics"], k["out"], k["out_pic"], None, None)
        assert rc == -2 and "invalid argument" in lib.last_error(), kw
    torch.cuda.synchronize()
    assert not out.any()
