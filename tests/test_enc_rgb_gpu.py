"""RGB at the batch encoder's two ends (xeve_hip_enc_push_rgb / _recon_rgb; BatchEncoder.push_rgb, push_video_rgb, recon_rgb, encode_video_rgb): a run fed with RGB
tensors writes the bitstreams of the same run fed with the bytes tests/_color.py converts those tensors to -- at both input depths and with a cropped size --, the
reconstructed pictures come back as the numpy inverse of recon() for every element type, and what is outside the contract is refused with the library's messages."""
import ctypes as C

import numpy as np
import pytest

import _color as K

pytestmark = [pytest.mark.gpu, pytest.mark.gpu_full]

GOPS, FRAMES = 2, 2
COLOUR = dict(matrix="bt709", full_range=False, siting="left")


@pytest.fixture(scope="module")
def dev():
    import torch

    import xeve_amd

    xeve_amd.init(0)
    return torch.device("cuda:0")


def _video(w, h, seed):
    """GOPS * FRAMES pictures of uint8 RGB: a moving gradient under a little noise (content the encoder codes quickly and not trivially)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = np.empty((GOPS * FRAMES, h, w, 3), np.uint8)
    for t in range(GOPS * FRAMES):
        for c in range(3):
            out[t, :, :, c] = np.clip((x * (2 + c) + y * (3 - c) + 17 * t + 40 * c) % 256 + rng.integers(-6, 7, size=(h, w)), 0, 255)
    return out


def _cfg(w, h, depth, **kw):
    from xeve_amd import encode

    return encode.config(w, h, qp=32, keyint=8, bframes=15, closed_gop=True, preset="medium", threads=1, input_depth=depth, **kw)


def _encode_bytes(cfg, video, depth):
    """the run pushed as bytes: (bitstreams, the encoder -- the caller closes it)"""
    from xeve_amd import encode

    enc = encode.BatchEncoder(cfg, GOPS, FRAMES)
    for g in range(GOPS):
        for f in range(FRAMES):
            enc.push(g, f, K.forward_frame(video[g * FRAMES + f], depth=depth, **{"full" if k == "full_range" else k: v for k, v in COLOUR.items()}).tobytes())
    return enc.encode(), enc


@pytest.fixture(scope="module")
def run10(dev):
    """the 64x64 run at input depth 10 with the reconstructed pictures kept, pushed as bytes: shared by the tests below and left unchanged"""
    video = _video(64, 64, 1)
    streams, enc = _encode_bytes(_cfg(64, 64, 10, keep_recon=True), video, 10)
    recon = [[np.frombuffer(enc.recon(g, f), "<u2").copy() for f in range(FRAMES)] for g in range(GOPS)]
    enc.close()
    return video, streams, recon


@pytest.mark.parametrize("depth", (10, 8))
def test_push_rgb_writes_the_bitstreams_of_the_converted_frames(depth, dev, run10):
    """two GOPs of two frames at 64x64, uint8 (H, W, 3) pictures, at both input depths"""
    import torch

    from xeve_amd import encode

    video = run10[0] if depth == 10 else _video(64, 64, 2)
    if depth == 10:
        want = run10[1]
    else:
        want, e = _encode_bytes(_cfg(64, 64, 8), video, 8)
        e.close()
    enc = encode.BatchEncoder(_cfg(64, 64, depth), GOPS, FRAMES)
    t = torch.from_numpy(video).to(dev)
    for g in range(GOPS):
        for f in range(FRAMES):
            enc.push_rgb(g, f, t[g * FRAMES + f], **COLOUR)
    got = enc.encode()
    enc.close()
    assert got == want and all(len(s) > 100 for s in got)


def test_push_rgb_of_a_cropped_size(dev):
    """70x50 with crop=True: the conversion runs at the INPUT size, straight into the frames the padded load reads; pushed GOP by GOP with push_video_rgb from a chw view"""
    import torch

    from xeve_amd import encode

    video = _video(70, 50, 3)
    want, e = _encode_bytes(_cfg(70, 50, 8, crop=True), video, 8)
    e.close()
    enc = encode.BatchEncoder(_cfg(70, 50, 8, crop=True), GOPS, FRAMES)
    t = torch.from_numpy(video).to(dev).permute(0, 3, 1, 2)
    for g in range(GOPS):
        enc.push_video_rgb(g, t[g * FRAMES:(g + 1) * FRAMES], "chw", **COLOUR)
    got = enc.encode()
    enc.close()
    assert got == want


def test_float_tensors_push_what_their_c16_values_say(dev):
    """float32 in [0, 1] (v / 255 is not v * 257 / 65535 in float32 everywhere: the expectation goes through the restatement's c16 of the same floats), one GOP's worth
    compared frame by frame through the leaf the entry point runs, and the run's bitstreams against the bytes"""
    import torch

    from xeve_amd import encode

    video = (_video(64, 64, 4).astype(np.float32) / np.float32(255)).astype(np.float32)
    cfg = _cfg(64, 64, 10)
    a, b = encode.BatchEncoder(cfg, GOPS, FRAMES), encode.BatchEncoder(cfg, GOPS, FRAMES)
    t = torch.from_numpy(video).to(dev)
    for g in range(GOPS):
        for f in range(FRAMES):
            a.push_rgb(g, f, t[g * FRAMES + f], **COLOUR)
            b.push(g, f, K.forward_frame(video[g * FRAMES + f], "bt709", False, "left", 10).tobytes())
    got, want = a.encode(), b.encode()
    a.close(), b.close()
    assert got == want


@pytest.fixture(scope="module")
def kept_run(dev, run10):
    """the same run pushed as RGB with the reconstructed pictures kept: one encoder for the four element types"""
    import torch

    from xeve_amd import encode

    video, streams, _ = run10
    enc = encode.BatchEncoder(_cfg(64, 64, 10, keep_recon=True), GOPS, FRAMES)
    try:
        t = torch.from_numpy(video).to(dev)
        for g in range(GOPS):
            enc.push_video_rgb(g, t[g * FRAMES:(g + 1) * FRAMES], **COLOUR)
        assert enc.encode() == streams
        yield enc
    finally:
        enc.close()


@pytest.mark.parametrize("dtype", K.DTYPES)
def test_recon_rgb_is_the_inverse_of_recon(dtype, dev, run10, kept_run):
    import torch

    recon, enc = run10[2], kept_run
    tdt = {"uint8": torch.uint8, "float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32}[dtype]
    for g in range(GOPS):
        for f in range(FRAMES):
            want = K.inverse_frame(recon[g][f], 64, 64, dtype, "bt709", False, "left")
            got = enc.recon_rgb(g, f, dtype=tdt, **COLOUR)
            assert got.shape == (64, 64, 3) and got.dtype == tdt
            got = got.view(torch.int16).cpu().numpy().view(np.uint16) if dtype == "bfloat16" else got.cpu().numpy()
            assert np.array_equal(got, want), (g, f)


def test_recon_rgb_into_a_view_of_the_callers(dev, run10, kept_run):
    """chw, rows and planes padded, another colour setting: the padding is untouched"""
    import torch

    base = torch.full((3, 70, 80), 9, dtype=torch.uint8, device=dev)
    kept_run.recon_rgb(1, 1, layout="chw", out=base[:, 3:67, 8:72], matrix="bt601", full_range=True, siting="centre")
    want = np.full((3, 70, 80), 9, np.uint8)
    want[:, 3:67, 8:72] = K.inverse_frame(run10[2][1][1], 64, 64, "uint8", "bt601", True, "centre").transpose(2, 0, 1)
    assert np.array_equal(base.cpu().numpy(), want)


def test_encode_video_rgb_joins_the_gops(dev, run10):
    import torch

    from xeve_amd import encode

    video, streams, _ = run10
    assert encode.encode_video_rgb(torch.from_numpy(video).to(dev), _cfg(64, 64, 10), FRAMES, **COLOUR) == b"".join(streams)
    with pytest.raises(ValueError):
        encode.encode_video_rgb(torch.from_numpy(video[:3]).to(dev), _cfg(64, 64, 10), FRAMES, **COLOUR)


def test_what_the_entry_points_refuse(dev, run10):
    """recon_rgb without keep_recon and before a picture has ended, a colour depth that is not the run's input depth, host memory, null arguments, a wrong size"""
    import torch

    from xeve_amd import encode, lib

    video = run10[0]
    t = torch.from_numpy(video).to(dev)
    enc = encode.BatchEncoder(_cfg(64, 64, 10), GOPS, FRAMES)
    try:
        desc = lib.RgbDesc(0, 0, 3, 192, 1, 0)
        for depth in (8, 9):
            assert enc._L.xeve_hip_enc_push_rgb(enc._h, 0, 0, t.data_ptr(), C.byref(desc), C.byref(lib.Color(1, 0, 0, depth))) == -2
            assert "is not the run's input depth (10)" in lib.last_error()
        col = lib.Color(1, 0, 0, 10)
        host = np.zeros(64 * 64 * 3, np.uint8)
        assert enc._L.xeve_hip_enc_push_rgb(enc._h, 0, 0, host.ctypes.data, C.byref(desc), C.byref(col)) == -2 and "not device memory of the encoder's GPU" in lib.last_error()
        assert enc._L.xeve_hip_enc_push_rgb(enc._h, 0, 0, t.data_ptr(), None, C.byref(col)) == -2 and "invalid argument" in lib.last_error()
        assert enc._L.xeve_hip_enc_push_rgb(enc._h, 0, 0, t.data_ptr(), C.byref(desc), None) == -2
        assert enc._L.xeve_hip_enc_push_rgb(enc._h, GOPS, 0, t.data_ptr(), C.byref(desc), C.byref(col)) == -2
        assert enc._L.xeve_hip_enc_push_rgb(enc._h, 0, 0, t.data_ptr(), C.byref(lib.RgbDesc(7, 0, 3, 192, 1, 0)), C.byref(col)) == -2
        with pytest.raises(ValueError):
            enc.push_rgb(0, 0, t[0, :32])
        for g in range(GOPS):
            enc.push_video_rgb(g, t[g * FRAMES:(g + 1) * FRAMES], **COLOUR)
        assert enc.encode() == run10[1]  # (the refused calls pushed nothing and left the run as it was)
        with pytest.raises(lib.XeveHipError, match=r"xeve_hip_enc_recon_rgb: the run was created without reserved\[0\] bit 3"):
            enc.recon_rgb(0, 0)
    finally:
        enc.close()
    enc = encode.BatchEncoder(_cfg(64, 64, 10, keep_recon=True), GOPS, FRAMES)
    try:
        with pytest.raises(lib.XeveHipError, match="no run has begun"):
            enc.recon_rgb(0, 0)
        out = torch.zeros((64, 64, 3), dtype=torch.uint8)
        desc, col = lib.RgbDesc(0, 0, 3, 192, 1, 0), lib.Color(1, 0, 0, 10)
        for g in range(GOPS):
            enc.push_video_rgb(g, t[g * FRAMES:(g + 1) * FRAMES], **COLOUR)
        enc.encode()
        assert enc._L.xeve_hip_enc_recon_rgb(enc._h, 0, 0, out.data_ptr(), C.byref(desc), C.byref(col)) == -2 and "not device memory of the encoder's GPU" in lib.last_error()
        assert enc._L.xeve_hip_enc_recon_rgb(enc._h, 0, FRAMES, t.data_ptr(), C.byref(desc), C.byref(col)) == -2 and "out of range" in lib.last_error()
        assert enc._L.xeve_hip_enc_recon_rgb(enc._h, 0, 0, t.data_ptr(), C.byref(desc), C.byref(lib.Color(1, 0, 0, 8))) == -2 and "invalid argument" in lib.last_error()
        assert enc._L.xeve_hip_enc_recon_rgb(enc._h, 0, 0, t.data_ptr(), None, C.byref(col)) == -2
    finally:
        enc.close()
