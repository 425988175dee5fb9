"""xeve_hip_frames_load and xeve_hip_recon_crop on the GPU (xeve_amd/csrc/frames.hip): the two ends of a picture whose size is even but no multiple of 8 -- the pushed
frames padded with zeros into the coded planes, the reconstructed pictures' window packed without padding -- both EXACT against numpy, at sizes that cover every even
residue of the width and the height modulo 8, chroma rows of odd length (35 samples at 70 wide: packed rows on 2-byte, for 8-bit input on 1-byte boundaries), a plane one
sample wide, frames and outputs at every alignment the contracts allow, and picture distances that put the last picture past 2^32 bytes from the base."""
import ctypes as C

import numpy as np
import pytest

# gpu_full (XEVE_GPU_FULL=1): as the reconstruction and signature tests (tests/test_recon_gpu.py), kept out of the default GPU suite and its recorded durations
pytestmark = [pytest.mark.gpu, pytest.mark.gpu_full]

SIZES = [(2, 2), (6, 2), (2, 6), (10, 18), (70, 50), (62, 36), (130, 66), (358, 286)]
FILL = -1  # 0xFFFF: what stands in the outputs before the call
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    import torch

    import xeve_amd

    xeve_amd.init(0)
    return torch.device("cuda:0")


def _align8(v):
    return (v + 7) & ~7


def _ptrs(addresses):
    return (C.c_void_p * 3)(*addresses)


def _load(frames, frame_dist, depth, sw, sh, w, h, org, s, pic, npics):
    from xeve_amd import lib

    return lib.load().xeve_hip_frames_load(frames, frame_dist, depth, sw, sh, w, h, _ptrs(org), s[0], s[1], pic[0], pic[1], npics, None)


def _crop(rec, s, pic, cw, ch, npics, out, out_pic):
    from xeve_amd import lib

    return lib.load().xeve_hip_recon_crop(_ptrs(rec), s[0], s[1], pic[0], pic[1], cw, ch, npics, out, out_pic, None)


def _frames(rng, sw, sh, depth, npics, gap):
    """npics frames of sw x sh, `gap` bytes of other data between them: (the bytes, the distance, per picture the three planes as the codec must see them)"""
    n = sw * sh * 3 // 2
    if depth == 8:
        body = rng.integers(0, 256, size=(npics, n), dtype=np.uint8)
        wide = body.astype(np.uint16) << 2
    else:
        wide = (rng.integers(0, 1024, size=(npics, n), dtype=np.uint16) | 3).astype("<u2")  # (the low bits set: nothing may shift or mask them)
        body = wide.view(np.uint8).reshape(npics, -1)
    dist = body.shape[1] + gap
    raw = rng.integers(0, 256, size=npics * dist, dtype=np.uint8)
    for p in range(npics):
        raw[p * dist:p * dist + body.shape[1]] = body[p]
    planes = [[wide[p, :sw * sh].reshape(sh, sw), wide[p, sw * sh:sw * sh * 5 // 4].reshape(sh // 2, sw // 2), wide[p, sw * sh * 5 // 4:].reshape(sh // 2, sw // 2)] for p in range(npics)]
    return raw, dist, planes


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("sw,sh", SIZES)
def test_frames_load_pads_with_zeros_exactly(sw, sh, depth, dev):
    """one and three pictures; the frames start 0 and 2 (8 bit: also 1) bytes into their buffer; the outputs are pre-filled with 0xFFFF, so a padding sample nobody wrote
    shows, and everything outside the w x h windows -- the rows' tails up to the stride, the gaps between the pictures, a guard band behind each plane -- stays as it was"""
    import torch

    w, h = _align8(sw), _align8(sh)
    rng = np.random.default_rng(sw * 1000 + sh + depth)
    s, pic = (w + 8, w // 2 + 4), ((w + 8) * h + 16, (w // 2 + 4) * (h // 2) + 8)
    for npics in (1, 3):
        for lead in ((0, 2) if depth == 10 else (0, 1, 2)):
            raw, dist, planes = _frames(rng, sw, sh, depth, npics, 6)
            d_raw = torch.from_numpy(np.concatenate([np.zeros(lead, np.uint8), raw])).to(dev)
            outs = [torch.full((npics * pic[c > 0] + GUARD,), FILL, dtype=torch.int16, device=dev) for c in range(3)]
            want = [np.full(npics * pic[c > 0] + GUARD, FILL, np.int16).view(np.uint16) for c in range(3)]
            for p in range(npics):
                for c in range(3):
                    pw, ph, st = (w, h, s[0]) if c == 0 else (w // 2, h // 2, s[1])
                    win = np.lib.stride_tricks.as_strided(want[c][p * pic[c > 0]:], (ph, pw), (2 * st, 2))
                    win[:] = 0
                    win[:planes[p][c].shape[0], :planes[p][c].shape[1]] = planes[p][c]
            assert _load(d_raw.data_ptr() + lead, dist, depth, sw, sh, w, h, [t.data_ptr() for t in outs], s, pic, npics) == 0
            torch.cuda.synchronize()
            for c in range(3):
                assert np.array_equal(outs[c].cpu().numpy().view(np.uint16), want[c]), (npics, lead, c)
            assert np.array_equal(d_raw.cpu().numpy()[lead:], raw)


@pytest.mark.parametrize("cw,ch", SIZES)
def test_recon_crop_packs_the_window_exactly(cw, ch, dev):
    """the encoder's stores (W + 288 / W / 2 + 144 wide), one and three pictures, `out` on a 16-byte boundary and 2 bytes behind one, pictures packed back to back and
    out_pic larger than the picture (by an odd number of samples, so that the rows' alignment changes from picture to picture); what lies between and behind the packed
    pictures stays as it was, the stores are only read"""
    import torch

    W, H = _align8(cw), _align8(ch)
    rng = np.random.default_rng(cw * 1000 + ch)
    s = (W + 288, W // 2 + 144)
    pic = (s[0] * H + 40, s[1] * (H // 2) + 20)
    n = cw * ch * 3 // 2
    for npics in (1, 3):
        host = [rng.integers(0, 1024, size=8 + npics * pic[c > 0], dtype=np.int16) for c in range(3)]
        d_rec = [torch.from_numpy(a).to(dev) for a in host]
        lead_rec = (8, 4, 4)
        for lead, extra in ((0, 0), (1, 0), (0, 5), (1, 8)):
            out_pic = n + extra
            out = torch.full((lead + npics * out_pic + GUARD,), FILL, dtype=torch.int16, device=dev)
            want = np.full(lead + npics * out_pic + GUARD, FILL, np.int16)
            for p in range(npics):
                at = lead + p * out_pic
                for c in range(3):
                    pw, ph = (cw, ch) if c == 0 else (cw // 2, ch // 2)
                    win = np.lib.stride_tricks.as_strided(host[c][lead_rec[c] + p * pic[c > 0]:], (ph, pw), (2 * s[c > 0], 2))
                    want[at:at + pw * ph] = win.reshape(-1)
                    at += pw * ph
            assert _crop([t.data_ptr() + 2 * l for t, l in zip(d_rec, lead_rec)], s, pic, cw, ch, npics, out.data_ptr() + 2 * lead, out_pic) == 0
            torch.cuda.synchronize()
            want[:lead] = FILL
            assert np.array_equal(out.cpu().numpy(), want), (npics, lead, extra)
        assert all(np.array_equal(t.cpu().numpy(), a) for t, a in zip(d_rec, host))


def test_arguments_outside_the_contracts_are_refused(dev):
    """XEVE_HIP_ERR_ARG before any launch: odd input sizes, an input larger than the coded picture, coded sizes that are no multiple of 8 or outside 8 .. 8192 x 8 .. 4320,
    a depth of 12, strides that break the aligned rows, misaligned planes, no pictures; for the crop odd or oversized windows, a stride below the window's last chunk, an
    odd output address, pictures that overlap"""
    import torch

    from xeve_amd import lib

    t = torch.zeros(8192, dtype=torch.int16, device=dev)
    src = torch.zeros(8192, dtype=torch.uint8, device=dev)
    a = [t.data_ptr()] * 3
    base = dict(frames=src.data_ptr(), dist=5250, depth=8, sw=70, sh=50, w=72, h=56, org=a, s_l=72, s_c=36, p_l=72 * 56, p_c=36 * 28, npics=1)
    bad = (dict(sw=69), dict(sh=49), dict(sw=0), dict(sw=74), dict(sh=58), dict(w=70), dict(h=50), dict(w=8200, s_l=8200, s_c=4100), dict(h=4328), dict(depth=12), dict(depth=9),
           dict(s_l=70), dict(s_c=34), dict(s_c=38), dict(org=[t.data_ptr() + 2] + a[1:]), dict(org=a[:2] + [t.data_ptr() + 4]), dict(npics=0), dict(npics=65536), dict(frames=None),
           dict(npics=2, dist=5248), dict(npics=2, p_l=72 * 48), dict(depth=10, frames=src.data_ptr() + 1), dict(depth=10, dist=10501, npics=2))
    for kw in bad:
        k = dict(base, **kw)
        rc = _load(k["frames"], k["dist"], k["depth"], k["sw"], k["sh"], k["w"], k["h"], k["org"], (k["s_l"], k["s_c"]), (k["p_l"], k["p_c"]), k["npics"])
        assert rc == -2 and "invalid argument" in lib.last_error(), kw
    out = torch.zeros(8192, dtype=torch.int16, device=dev)
    base = dict(rec=a, s_l=72, s_c=36, p_l=72 * 56, p_c=36 * 28, cw=70, ch=50, npics=1, out=out.data_ptr(), out_pic=5250)
    bad = (dict(cw=69), dict(ch=51), dict(cw=0), dict(ch=0), dict(cw=8194), dict(ch=4322), dict(s_l=64), dict(s_c=32), dict(s_l=76), dict(s_c=38), dict(p_l=72 * 56 + 4),
           dict(p_c=36 * 28 + 2), dict(rec=[t.data_ptr() + 8] + a[1:]), dict(rec=a[:1] + [t.data_ptr() + 4] + a[2:]), dict(out=None), dict(out=out.data_ptr() + 1), dict(npics=0),
           dict(out_pic=5249))
    for kw in bad:
        k = dict(base, **kw)
        rc = _crop(k["rec"], (k["s_l"], k["s_c"]), (k["p_l"], k["p_c"]), k["cw"], k["ch"], k["npics"], k["out"], k["out_pic"])
        assert rc == -2 and "invalid argument" in lib.last_error(), kw
    torch.cuda.synchronize()
    assert not out.any() and not t.any()


FAR_SAMPLES = 2 ** 31 + 4096  # samples between stacked planes: 2^32 + 8192 bytes, so pictures 1 and 2 lie past 2^32 bytes; truncated to 32 bits it lands inside picture 0
FAR_BYTES = 2 ** 32 + 4098  # bytes between the frames (even: 10-bit frames)
WINDOW = 65536


def _far(torch, dev, dtype, n):
    free = torch.cuda.mem_get_info()[0]
    need = n * (2 if dtype == torch.int16 else 1)
    assert free > need + (1 << 30), "the device's free memory does not hold the far allocation (%d of %d bytes)" % (free, need)
    return torch.empty(n, dtype=dtype, device=dev)  # (nothing fills it: touched at the three windows only)


def test_frames_load_with_pictures_past_2_to_the_32_bytes(dev):
    """three 70x50 pictures of 10-bit input whose frames are FAR_BYTES apart and whose planes are FAR_SAMPLES apart, inside allocations that nothing fills: every
    picture's planes against numpy -- a distance cut to 32 bits would read picture 0's frame or write into picture 0's planes"""
    import torch

    sw, sh, w, h = 70, 50, 72, 56
    rng = np.random.default_rng(70)
    _, _, planes = _frames(rng, sw, sh, 10, 3, 0)
    at = (0, 8192, 16384)  # the planes of picture 0 inside the window
    src = org = None
    try:
        src, org = _far(torch, dev, torch.uint8, 2 * FAR_BYTES + WINDOW), _far(torch, dev, torch.int16, 2 * FAR_SAMPLES + WINDOW)
        for p in range(3):
            frame = np.concatenate([pl.reshape(-1) for pl in planes[p]]).astype("<u2").view(np.uint8)
            src[p * FAR_BYTES:p * FAR_BYTES + frame.size].copy_(torch.from_numpy(frame.copy()).to(dev))
            org[p * FAR_SAMPLES:p * FAR_SAMPLES + WINDOW].fill_(FILL)
        assert _load(src.data_ptr(), FAR_BYTES, 10, sw, sh, w, h, [org.data_ptr() + 2 * a for a in at], (w, w // 2), (FAR_SAMPLES, FAR_SAMPLES), 3) == 0
        torch.cuda.synchronize()
        for p in range(3):
            got = org[p * FAR_SAMPLES:p * FAR_SAMPLES + WINDOW].cpu().numpy().view(np.uint16)
            want = np.full(WINDOW, 0xFFFF, np.uint16)
            for c in range(3):
                pw, ph = (w, h) if c == 0 else (w // 2, h // 2)
                win = want[at[c]:at[c] + pw * ph].reshape(ph, pw)
                win[:] = 0
                win[:planes[p][c].shape[0], :planes[p][c].shape[1]] = planes[p][c]
            assert np.array_equal(got, want), p
    finally:
        src = org = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def test_recon_crop_with_pictures_past_2_to_the_32_bytes(dev):
    """three pictures whose stores are FAR_SAMPLES apart and whose packed outputs are FAR_SAMPLES + 1 apart: every picture's window against numpy"""
    import torch

    cw, ch, W = 70, 50, 72
    s = (W + 288, W // 2 + 144)
    at = (0, 32768, 49152)
    rng = np.random.default_rng(71)
    n = cw * ch * 3 // 2
    rec = out = None
    try:
        rec, out = _far(torch, dev, torch.int16, 2 * FAR_SAMPLES + WINDOW), _far(torch, dev, torch.int16, 2 * (FAR_SAMPLES + 1) + WINDOW)
        host = [rng.integers(0, 1024, size=WINDOW, dtype=np.int16) for _ in range(3)]
        for p in range(3):
            rec[p * FAR_SAMPLES:p * FAR_SAMPLES + WINDOW].copy_(torch.from_numpy(host[p]).to(dev))
            out[p * (FAR_SAMPLES + 1):p * (FAR_SAMPLES + 1) + WINDOW].fill_(FILL)
        assert _crop([rec.data_ptr() + 2 * a for a in at], s, (FAR_SAMPLES, FAR_SAMPLES), cw, ch, 3, out.data_ptr(), FAR_SAMPLES + 1) == 0
        torch.cuda.synchronize()
        for p in range(3):
            got = out[p * (FAR_SAMPLES + 1):p * (FAR_SAMPLES + 1) + WINDOW].cpu().numpy()
            want = np.full(WINDOW, FILL, np.int16)
            k = 0
            for c in range(3):
                pw, ph = (cw, ch) if c == 0 else (cw // 2, ch // 2)
                want[k:k + pw * ph] = np.lib.stride_tricks.as_strided(host[p][at[c]:], (ph, pw), (2 * s[c > 0], 2)).reshape(-1)
                k += pw * ph
            assert k == n and np.array_equal(got, want), p
    finally:
        rec = out = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
