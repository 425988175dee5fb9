"""The batch encoder's per-picture SSIM on the GPU (reserved[0] bit 6; xeve_amd/csrc/encode.hip with ssim.hip): for every picture of a two-GOP run the sums
BatchEncoder.ssim() returns EQUAL the numpy restatement (tests/_ssim.py) applied to the frame pushed, widened to 10 bits, and to what recon() hands out -- the shown
window, also at a size coded with padding -- and the figure equals the restatement's own division.  The bit changes no bitstream and no other field of picture(), costs
G * F * 24 bytes of footprint and nothing without it; the refusals are those of picture()."""
import os

import numpy as np
import pytest

import _e2e
import _enc
import _ssim as S

# gpu_full (XEVE_GPU_FULL=1): as the reconstruction tests (tests/test_enc_recon_gpu.py), kept out of the default GPU suite and its recorded durations
pytestmark = [pytest.mark.gpu, pytest.mark.gpu_full]

GOPS, FRAMES = 2, 4
# (w, h, threads, crop, input depth): two row chains per picture (the second writer pass); an even size coded at 72x56 with padding; 16-bit input
CASES = {"aligned_m2": (128, 128, 2, False, 8), "crop_70x50": (70, 50, 1, True, 8), "ten_bit": (128, 128, 2, False, 10)}


@pytest.fixture(scope="module")
def hip():
    import xeve_amd
    from xeve_amd import encode

    xeve_amd.init(0)
    return encode


def _clip(tmp, w, h, depth):
    """per GOP the frames as they are pushed; the smooth drifting texture of tests/_e2e.py, so that the pictures differ and the reconstruction is close to them"""
    p = os.path.join(str(tmp), "clip_%dx%d.yuv" % (w, h))
    _e2e.make_yuv(p, w, h, GOPS * FRAMES, 5001)
    data = open(p, "rb").read()
    if depth == 10:
        data = _enc.widen10(data)
    fb = len(data) // GOPS
    return [data[g * fb:(g + 1) * fb] for g in range(GOPS)]


def _config(hip, name, **kw):
    w, h, threads, crop, depth = CASES[name]
    return hip.config(w, h, qp=30, keyint=8, closed_gop=True, bframes=3, preset="fast", threads=threads, crop=crop, input_depth=depth, **kw)


def _encode(hip, cfg, data):
    enc = hip.BatchEncoder(cfg, GOPS, FRAMES)
    try:
        for g in range(GOPS):
            enc.push_gop(g, data[g])
        return enc, enc.encode()
    except Exception:
        enc.close()
        raise


def _pushed_planes(data, g, f, w, h, depth):
    """frame f of GOP g as the codec sees it: at 10 bits"""
    per = w * h * 3 // 2
    if depth == 10:
        flat = np.frombuffer(data[g], "<u2")[f * per:(f + 1) * per].astype(np.int64)
    else:
        flat = np.frombuffer(data[g], np.uint8)[f * per:(f + 1) * per].astype(np.int64) << 2
    return S.split(flat, w, h)


@pytest.mark.parametrize("name", sorted(CASES))
def test_sums_equal_the_restatement_and_nothing_else_changes(name, hip, tmp_path):
    w, h, _, _, depth = CASES[name]
    data = _clip(tmp_path, w, h, depth)
    plain, plain_streams = _encode(hip, _config(hip, name, measure=True, keep_recon=True), data)
    try:
        rows = [plain.pictures(g) for g in range(GOPS)]
        with pytest.raises(hip._lib.XeveHipError, match="without reserved.*bit 6"):  # a run without the bit refuses
            plain.ssim(0, 0)
    finally:
        plain.close()
    enc, streams = _encode(hip, _config(hip, name, measure=True, keep_recon=True, ssim=True), data)
    try:
        assert streams == plain_streams
        windows = S.windows(w, h), S.windows(w // 2, h // 2), S.windows(w // 2, h // 2)
        seen = set()
        for g in range(GOPS):
            whole = enc.ssim(g)
            for f in range(FRAMES):
                rec = S.split(np.frombuffer(enc.recon(g, f), "<u2").astype(np.int64), w, h)
                want = S.picture_sums(rec, _pushed_planes(data, g, f, w, h, depth))
                got = enc.ssim(g, f)
                print(name, g, f, got["sums"], want, got["ssim"])
                assert got == whole[f]
                assert got["sums"] == want and got["windows"] == list(windows), (g, f)
                assert got["ssim"] == [S.figure(q, n) for q, n in zip(want, windows)], (g, f)
                row = enc.picture(g, f)
                assert row.pop("ssim") == got["ssim"] and row == rows[g][f] and "ssim" not in rows[g][f], (g, f)
                seen.add(tuple(want))
        assert len(seen) == GOPS * FRAMES  # (the pictures differ: a sum read from another picture's place would show)
        with pytest.raises(hip._lib.XeveHipError, match="out of range"):
            enc.ssim(0, FRAMES)
    finally:
        enc.close()


def test_the_bit_alone(hip, tmp_path):
    """bit 6 without bits 2 and 3: ssim() as with them, picture() and recon() refused as ever, the same bitstreams"""
    name = "crop_70x50"
    w, h, _, _, depth = CASES[name]
    data = _clip(tmp_path, w, h, depth)
    both, want_streams = _encode(hip, _config(hip, name, keep_recon=True, ssim=True), data)
    try:
        want = [both.ssim(g) for g in range(GOPS)]
    finally:
        both.close()
    enc, streams = _encode(hip, _config(hip, name, ssim=True), data)
    try:
        assert streams == want_streams and [enc.ssim(g) for g in range(GOPS)] == want
        with pytest.raises(hip._lib.XeveHipError, match="bit 2"):
            enc.picture(0, 0)
        with pytest.raises(hip._lib.XeveHipError, match="bit 3"):
            enc.recon(0, 0)
    finally:
        enc.close()


def test_a_picture_that_has_not_ended_refuses(hip, tmp_path):
    name = "aligned_m2"
    w, h, _, _, depth = CASES[name]
    data = _clip(tmp_path, w, h, depth)
    enc = hip.BatchEncoder(_config(hip, name, ssim=True), GOPS, FRAMES)
    try:
        with pytest.raises(hip._lib.XeveHipError, match="no run has begun"):
            enc.ssim(0, 0)
        for g in range(GOPS):
            enc.push_gop(g, data[g])
        enc.begin()
        total = enc.advance(0)
        with pytest.raises(hip._lib.XeveHipError, match="not ended"):
            enc.ssim(0, 0)
        enc.advance(total // FRAMES)  # the first picture's steps are issued: it ends
        enc.flush()
        first = enc.ssim(0, 0)
        with pytest.raises(hip._lib.XeveHipError, match="not ended"):
            enc.ssim(0)
        while enc.advance(1 << 20):
            pass
        enc.sync()
        assert enc.ssim(0)[0] == first and len(enc.ssim(1)) == FRAMES
    finally:
        enc.close()


def test_the_footprint_grows_by_the_sums_alone(hip):
    """G * F * 24 bytes with the bit -- no device call.  (The footprint counts every buffer in units of 256 bytes, as it always has: the batches below are those whose sums
    fill whole units, and the two-GOP run of this file, 192 bytes, costs one unit.)"""
    for name in sorted(CASES):
        for other in (dict(), dict(measure=True, keep_recon=True), dict(hash=True)):
            for gops, frames in ((8, 4), (32, 8), (64, 16)):
                assert gops * frames * 24 % 256 == 0
                without, with_bit = hip.footprint(_config(hip, name, **other), gops, frames), hip.footprint(_config(hip, name, ssim=True, **other), gops, frames)
                assert with_bit[0] - without[0] == gops * frames * 24 and with_bit[1] == without[1], (name, other, gops, frames)
            assert hip.footprint(_config(hip, name, ssim=True, **other), GOPS, FRAMES)[0] - hip.footprint(_config(hip, name, **other), GOPS, FRAMES)[0] == 256


def test_an_input_below_16_is_refused_at_create(hip):
    for w, h in ((12, 16), (16, 12)):
        cfg = hip.config(w, h, keyint=8, closed_gop=True, crop=True, ssim=True)
        with pytest.raises(hip._lib.XeveHipError, match="bit 6.*16x16"):
            hip.BatchEncoder(cfg, 1, 1)
        hip.BatchEncoder(hip.config(w, h, keyint=8, closed_gop=True, crop=True), 1, 1).close()  # (without the bit the size is what it was: accepted)
    hip.BatchEncoder(hip.config(16, 16, keyint=8, closed_gop=True, ssim=True), 1, 1).close()


def test_encode_file_appends_three_columns(hip, tmp_path):
    """today's rows, byte for byte, with SSIM-Y / U / V behind them"""
    name = "crop_70x50"
    w, h, _, _, depth = CASES[name]
    data = _clip(tmp_path, w, h, depth)
    yuv = os.path.join(str(tmp_path), "clip_%dx%d.yuv" % (w, h))
    cfg = _config(hip, name)
    out = {k: [str(tmp_path / (k + e)) for e in (".evc", ".txt")] for k in ("plain", "ssim")}
    hip.encode_file(yuv, out["plain"][0], cfg, GOPS, FRAMES, stats_path=out["plain"][1])
    hip.encode_file(yuv, out["ssim"][0], cfg, GOPS, FRAMES, stats_path=out["ssim"][1], ssim=True)
    assert open(out["plain"][0], "rb").read() == open(out["ssim"][0], "rb").read()
    plain, more = open(out["plain"][1]).read().splitlines(), open(out["ssim"][1]).read().splitlines()
    assert len(plain) == len(more) == GOPS * FRAMES
    enc, _ = _encode(hip, _config(hip, name, measure=True, ssim=True), data)
    try:
        rows = [p for g in range(GOPS) for p in sorted(enc.pictures(g), key=lambda p: p["coding_pos"])]
    finally:
        enc.close()
    for a, b, p in zip(plain, more, rows):
        assert b == a + "%-10.6f%-10.6f%-10.6f" % tuple(p["ssim"]) and len(b.split()) == len(a.split()) + 3, (a, b)
