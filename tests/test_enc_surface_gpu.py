"""Decoder surfaces at the batch encoder's front end (xeve_hip_enc_push_surface; BatchEncoder.push_surface): a run fed with NV12 / P010 surfaces of ANOTHER size writes,
byte for byte, the bitstreams of the same run fed through push with the bytes tests/_scale.py scales those surfaces to -- at both input depths, from a source twice the
run's size and from one of another aspect, and into a cropped run --, a push of a surface counts as one push and no more, what is outside the contract is refused with the
library's messages, and the configuration's footprint is what it was before the entry point existed."""
import ctypes as C

import numpy as np
import pytest

import _scale as K

pytestmark = [pytest.mark.gpu, pytest.mark.gpu_full]

GOPS, FRAMES = 2, 3
# xeve_hip_enc_footprint of _cfg(...) for GOPS x FRAMES as the parent commit reports it (device bytes, most GOPs of a batch): (w, h, depth, crop) -> value
PARENT_FOOTPRINT = {(64, 64, 8, False): (9810432, 65535), (64, 64, 10, False): (9847296, 65535), (70, 50, 8, True): (6215680, 65535), (70, 50, 10, True): (6247168, 65535)}


@pytest.fixture(scope="module")
def dev():
    import torch

    import xeve_amd

    xeve_amd.init(0)
    return torch.device("cuda:0")


def _cfg(w, h, depth, **kw):
    from xeve_amd import encode

    return encode.config(w, h, qp=32, keyint=8, bframes=1, closed_gop=True, preset="medium", threads=1, input_depth=depth, **kw)


def _video(sw, sh, depth, seed, n=GOPS * FRAMES):
    """n pictures as (y, u, v) planes of samples: a moving gradient under a little noise (content the encoder codes quickly and not trivially)"""
    rng = np.random.default_rng(seed)
    top = (1 << depth) - 1
    out = []
    for t in range(n):
        planes = []
        for c, (h, w) in enumerate(((sh, sw), (sh // 2, sw // 2), (sh // 2, sw // 2))):
            y, x = np.mgrid[0:h, 0:w]
            p = ((x * (2 + c) + y * (3 - c) + 17 * t + 40 * c) % 256 + rng.integers(-6, 7, size=(h, w))) * (top + 1) // 256
            planes.append(np.clip(p, 0, top).astype(np.int64))
        out.append(tuple(planes))
    return out


def _surface_tensors(planes, depth, dev, pad=6):
    """one picture as the decoder hands it over: NV12 (depth 8) or P010 (depth 10: the sample in the top bits), rows `pad` containers further apart than their length"""
    import torch

    y, u, v = planes
    sh, sw = y.shape
    shift, dt = (0, np.uint8) if depth == 8 else (6, np.uint16)
    ty = torch.zeros((sh, sw + pad), dtype=torch.uint8 if depth == 8 else torch.int16, device=dev)
    tuv = torch.zeros((sh // 2, sw // 2 + pad, 2), dtype=ty.dtype, device=dev)
    host = lambda a: torch.from_numpy((a << shift).astype(dt).view(np.uint8 if depth == 8 else np.int16)).to(dev)
    ty[:, :sw] = host(y)
    tuv[:, :sw // 2] = host(np.stack([u, v], axis=2))
    return ty[:, :sw], tuv[:, :sw // 2]


@pytest.mark.parametrize("run", ((64, 64, False), (70, 50, True)), ids=("64x64", "70x50-crop"))
@pytest.mark.parametrize("source", ((128, 128), (96, 80)), ids=("128x128", "96x80"))
@pytest.mark.parametrize("depth", (8, 10), ids=("nv12", "p010"))
def test_push_surface_writes_the_bitstreams_of_the_scaled_frames(depth, source, run, dev):
    """two GOPs of three frames, qp 32, one thread, one B frame, closed GOPs: the surface run against the run pushed with the restatement's bytes"""
    from xeve_amd import encode

    (sw, sh), (w, h, crop) = source, run
    video = _video(sw, sh, depth, sw + h + depth)
    kw = dict(crop=True) if crop else {}
    a, b = encode.BatchEncoder(_cfg(w, h, depth, **kw), GOPS, FRAMES), encode.BatchEncoder(_cfg(w, h, depth, **kw), GOPS, FRAMES)
    try:
        for g in range(GOPS):
            for f in range(FRAMES):
                planes = video[g * FRAMES + f]
                a.push_surface(g, f, *_surface_tensors(planes, depth, dev), msb_aligned=depth > 8)
                b.push(g, f, K.frame(*planes, w, h, "left", depth).tobytes())
        got, want = a.encode(), b.encode()
    finally:
        a.close(), b.close()
    assert got == want and all(len(s) > 100 for s in got) and got[0] != got[1]


def test_the_footprint_is_the_parents(dev):
    """nothing is counted for an entry point that is not called: the numbers are the parent commit's"""
    from xeve_amd import encode

    assert PARENT_FOOTPRINT
    for (w, h, depth, crop), want in PARENT_FOOTPRINT.items():
        assert encode.footprint(_cfg(w, h, depth, **(dict(crop=True) if crop else {})), GOPS, FRAMES) == want, (w, h, depth, crop)


def test_a_surface_counts_as_one_push(dev):
    """begin refuses a second run until EVERY frame has been pushed again, where the picture stores reuse the frames' memory: 1024x576 with 10-bit input and two pictures
    -- a padded store of 3 526 656 bytes fits into the two frames' 3 538 944 (at 64x64 no store fits into the frames, and no run is ever refused for a frame left out, with
    push as little as here).  One surface pushed of two: refused; both: the run begins"""
    from xeve_amd import encode, lib

    w, h, frames = 1024, 576, 2
    video = _video(w // 2, h // 2, 10, 3, frames)
    enc = encode.BatchEncoder(encode.config(w, h, keyint=8, closed_gop=True, preset="medium", threads=8, input_depth=10), 1, frames)
    try:
        tensors = [_surface_tensors(p, 10, dev) for p in video]
        for f in range(frames):
            enc.push_surface(0, f, *tensors[f], msb_aligned=True)
        assert len(enc.encode()[0]) > 1000
        with pytest.raises(lib.XeveHipError, match="consumed its frames"):
            enc.begin()
        enc.push_surface(0, 0, *tensors[0], msb_aligned=True)
        with pytest.raises(lib.XeveHipError, match="consumed its frames"):  # (every frame, not some)
            enc.begin()
        enc.push_surface(0, 1, *tensors[1], msb_aligned=True)
        enc.begin()
    finally:
        enc.close()


def test_what_the_entry_point_refuses(dev):
    """a depth that is not the run's, host memory, null arguments, a gop or frame outside the run, sizes the leaf refuses, and the Python face's own checks; the refused
    calls push nothing and leave the run as it was"""
    import torch

    from xeve_amd import encode, lib

    video = _video(128, 128, 10, 9)
    ref = encode.BatchEncoder(_cfg(64, 64, 10), GOPS, FRAMES)
    enc = encode.BatchEncoder(_cfg(64, 64, 10), GOPS, FRAMES)
    try:
        ty, tuv = _surface_tensors(video[0], 10, dev)

        def desc(depth=10, sb=2, shift=6, y=ty.data_ptr(), uv=tuv.data_ptr(), layout=1):
            s = lib.Surface(layout, sb, depth, shift)
            s.plane[0], s.plane[1] = y, uv
            s.pitch_l, s.pitch_c = ty.stride(0) * 2, tuv.stride(0) * 2
            return s

        push = lambda s, g=0, f=0, sw=128, sh=128, siting=0: enc._L.xeve_hip_enc_push_surface(enc._h, g, f, C.byref(s) if s is not None else None, sw, sh, siting)
        for s in (desc(depth=8, shift=8), desc(depth=8, sb=1, shift=0), desc(depth=9)):
            assert push(s) == -2 and "is not the run's input depth (10)" in lib.last_error()
        host = np.zeros(128 * 140 * 2, np.uint8)
        assert push(desc(y=host.ctypes.data)) == -2 and "plane 0 is not device memory of the encoder's GPU" in lib.last_error()
        assert push(desc(uv=host.ctypes.data)) == -2 and "plane 1 is not device memory of the encoder's GPU" in lib.last_error()
        assert push(desc(uv=None)) == -2 and push(desc(layout=0)) == -2  # (planar: the third plane is missing)
        assert push(None) == -2 and "invalid argument" in lib.last_error()
        assert push(desc(), g=GOPS) == -2 and push(desc(), f=FRAMES) == -2 and push(desc(), g=-1) == -2
        for kw in (dict(sw=127), dict(sh=0), dict(sw=520, sh=8), dict(siting=2), dict(sw=6, sh=6)):
            assert push(desc(), **kw) == -2 and "invalid argument" in lib.last_error(), kw
        assert push(desc(shift=2)) == -2 and push(desc(layout=3)) == -2
        with pytest.raises(ValueError):
            enc.push_surface(0, 0, ty.to(torch.uint8), tuv.to(torch.uint8))  # (bytes into a 10-bit run)
        with pytest.raises(ValueError):
            enc.push_surface(0, 0, ty, tuv, siting="top")
        for e, surf in ((ref, False), (enc, True)):
            for g in range(GOPS):
                for f in range(FRAMES):
                    if surf:
                        e.push_surface(g, f, *_surface_tensors(video[g * FRAMES + f], 10, dev), msb_aligned=True)
                    else:
                        e.push(g, f, K.frame(*video[g * FRAMES + f], 64, 64, "left", 10).tobytes())
        assert enc.encode() == ref.encode()
    finally:
        enc.close(), ref.close()
