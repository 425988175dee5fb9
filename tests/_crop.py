"""Helpers of the cropped-size tests: pictures whose size is even but no multiple of 8.  The reference codes ALIGN8 of both directions, pads the input with zeros on the right
and below (the application zeroes its images once and reads w x h samples into them) and says in the SPS which window to show.  The cases here are the ones
tests/golden/make_crop_golden.py records from the unmodified reference application into tests/golden/crop_v1.json."""
import json
import os

import _e2e
import _enc

GOLDEN_PATH = os.path.join(_enc.ROOT, "tests", "golden", "crop_v1.json")
_RA = ["--closed-gop", "-I", "8", "-b", "7"]
# name -> (w, h, gops, frames per gop, seed, options, threads); all closed GOPs of 8 frames, two GOPs of different content (frames 0 .. 7 and 8 .. 15 of one clip)
CASES = {
    "crop_70x50_ra_medium": (70, 50, 2, 8, 7, ["--preset", "medium", "-q", "27"] + _RA, 1),  # coded 72x56: chroma rows of 35 samples
    "crop_70x50_ra_medium_10bit": (70, 50, 2, 8, 7, ["--preset", "medium", "-q", "27"] + _RA + ["-d", "10"], 1),  # the same clip through _enc.widen10
    "crop_70x50_ra_fast": (70, 50, 2, 8, 7, ["--preset", "fast", "-q", "22"] + _RA, 1),
    "crop_130x66_m2": (130, 66, 2, 8, 7, ["--preset", "medium", "-q", "30"] + _RA, 2),  # coded 136x72: two row chains, the second writer pass
    "crop_62x36_ld": (62, 36, 2, 8, 7, ["--preset", "medium", "-q", "32", "--closed-gop", "-I", "8", "-b", "0"], 1),  # coded 64x40: one CTU wide, low delay
    "crop_202x138_slow_m3": (202, 138, 2, 8, 7, ["--preset", "slow", "-q", "25"] + _RA, 3),  # coded 208x144 (the fused walk only)
    "crop_2x2": (2, 2, 2, 8, 7, ["--preset", "medium", "-q", "32"] + _RA, 1),  # coded 8x8: the smallest input, chroma is one sample
}
HASH_CASE = "crop_70x50_ra_medium"  # also recorded with --hash


def align8(v):
    return (v + 7) & ~7


def golden():
    return json.load(open(GOLDEN_PATH))


def clip(yuv_dir, name):
    """the case's input as the encoders take it (frames of the INPUT size; 16-bit samples where the options say -d 10): (path of the file, one bytes object per GOP)"""
    w, h, gops, frames, seed, cli, _ = CASES[name]
    p = os.path.join(str(yuv_dir), name + ".yuv")
    if not os.path.exists(p):
        _e2e.make_yuv(p, w, h, gops * frames, seed)
        if "-d" in cli:
            assert cli[cli.index("-d") + 1] == "10"
            data = _enc.widen10(open(p, "rb").read())
            open(p, "wb").write(data)
    data = open(p, "rb").read()
    fb = len(data) // gops
    return p, [data[g * fb:(g + 1) * fb] for g in range(gops)]


def pad_frames(data, w, h, sample_bytes=1):
    """planar 4:2:0 frames of w x h -> frames of the coded size, every sample right of column w and below row h zero: what the reference's encoder sees after imgb_read"""
    import numpy as np

    dt = np.uint8 if sample_bytes == 1 else np.dtype("<u2")
    a = np.frombuffer(data, dtype=dt)
    W, H, n = align8(w), align8(h), w * h * 3 // 2
    assert a.size % n == 0
    out = []
    for f in range(a.size // n):
        at = f * n
        for pw, ph, PW, PH in ((w, h, W, H), (w // 2, h // 2, W // 2, H // 2), (w // 2, h // 2, W // 2, H // 2)):
            plane = np.zeros((PH, PW), dtype=dt)
            plane[:ph, :pw] = a[at:at + pw * ph].reshape(ph, pw)
            out.append(plane.tobytes())
            at += pw * ph
    return b"".join(out)


CROP_BIT = 32  # xeve_hip_enc_config.reserved[0] bit 5: w and h may be any even size


def harness_config(name):
    """the case's options as the CPU harness takes them (tests/_enc.py config), w and h the INPUT size, the bit that accepts it set"""
    w, h, _, _, _, cli, threads = CASES[name]
    c = _enc.config(w, h, cli, threads)
    c.reserved[0] |= CROP_BIT
    return c


def product_config(encode, name, **switches):
    """the case's options as xeve_amd.encode.config takes them, w and h the INPUT size"""
    w, h, _, _, _, cli, threads = CASES[name]
    c = _enc.config(w, h, cli, threads)
    return encode.config(w, h, qp=c.qp, keyint=c.keyint, bframes=c.bframes, closed_gop=c.closed_gop, preset=c.preset, threads=c.threads, ref=c.ref, input_depth=c.reserved[1] or 8,
                         crop=True, **switches)
