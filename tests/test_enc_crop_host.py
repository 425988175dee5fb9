"""Even picture sizes that are no multiple of 8, without a device: the frame loop and the high-level syntax (xeve_amd/csrc/enc_plan.h, enc_host.h) on the CPU harness against
tests/golden/crop_v1.json, recorded from the unmodified reference application (tests/golden/make_crop_golden.py); what the product library accepts and refuses; what a
batch of such pictures costs.  The configuration's w, h are the INPUT size; the harness's CPU engine reads coded pictures, so it is handed frames zero-padded to the coded
size -- exactly what the reference's encoder sees after the application's imgb_read."""
import pytest

import _crop
import _enc

GOLDEN = _crop.golden()


@pytest.fixture(scope="module")
def yuv_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("enc_crop_host_yuv")


def _padded(yuv_dir, name):
    w, h, gops, frames, _, cli, threads = _crop.CASES[name]
    _, data = _crop.clip(yuv_dir, name)
    return _crop.harness_config(name), [_crop.pad_frames(d, w, h, 2 if "-d" in cli else 1) for d in data], frames


@pytest.mark.parametrize("name", sorted(_crop.CASES))
def test_cropped_streams_equal_the_reference(name, yuv_dir):
    """both GOPs of every case: the bytes of the reference application's run of that GOP"""
    cfg, gops, frames = _padded(yuv_dir, name)
    want = [(p["bytes"], p["md5"]) for p in GOLDEN[name]["per_gop"]]
    assert len(want) == len(gops) == 2
    got = _enc.encode_cpu(cfg, gops, frames)
    assert [(len(s), _enc.md5(s)) for s in got] == want
    if name == "crop_70x50_ra_medium":
        flushed, after = _enc.encode_cpu_flushed(cfg, gops, frames)
        assert [(len(s), _enc.md5(s)) for s in flushed] == want and after[-1] == want[0][0]


class _Bits:
    def __init__(self, data):
        self.d, self.at = data, 0

    def u(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | ((self.d[self.at >> 3] >> (7 - (self.at & 7))) & 1)
            self.at += 1
        return v

    def ue(self):
        z = 0
        while self.u(1) == 0:
            z += 1
        return (1 << z) - 1 + (self.u(z) if z else 0)


def _sps(payload):
    """(coded width, coded height, cropping flag, [left, right, top, bottom]) of a Baseline SPS (xeve_eco_sps with every tool flag 0)"""
    r = _Bits(payload)
    r.ue(), r.u(8), r.u(8), r.u(32), r.u(32)  # sps id, profile_idc, level_idc, toolset_idc_h / _l
    assert r.ue() == 1  # chroma_format_idc: 4:2:0
    w, h = r.ue(), r.ue()
    assert (r.ue(), r.ue(), r.u(13)) == (2, 2, 0)  # the bit depths minus 8, the thirteen tool flags
    if r.ue() == 0:  # log2_sub_gop_length
        r.ue()  # log2_ref_pic_gap_length
    r.ue()  # max_num_ref_pics
    flag = r.u(1)
    return w, h, flag, [r.ue() for _ in range(4)] if flag else [0, 0, 0, 0]


@pytest.mark.parametrize("name,crop,res", [("crop_70x50_ra_medium", [0, 1, 0, 3], b"69x47"), ("crop_130x66_m2", [0, 3, 0, 3], b"127x63"), ("crop_2x2", [0, 3, 0, 3], b"-1x-1")])
def test_the_sps_carries_the_coded_size_and_the_window(name, crop, res, yuv_dir):
    """the aligned size, picture_cropping_flag and the four offsets (right = (W - w + 1) >> 1, bottom likewise: xeve_enc.c:1578-1582); the option SEI prints the input size
    minus those offsets (xeve_enc.c:2538): 69x47 at 70x50 -- the reference's quirk, reproduced"""
    from xeve_amd import encode

    cfg, gops, frames = _padded(yuv_dir, name)
    w, h = _crop.CASES[name][:2]
    units = encode.split_nal_units(_enc.encode_cpu(cfg, gops[:1], frames)[0])
    sps = [p for nut, _, p in units if nut == 24]
    assert len(sps) == 1 and _sps(sps[0]) == (_crop.align8(w), _crop.align8(h), 1, crop)
    sei = [p for nut, _, p in units if nut == 28]
    assert len(sei) == 1 and b" input-res=" + res + b" " in sei[0]


def test_an_aligned_size_keeps_its_sps(yuv_dir):
    """72x56 pushed as it is: no cropping flag, the input size in the option SEI"""
    import _e2e
    from xeve_amd import encode

    p = str(yuv_dir / "aligned_72x56.yuv")
    _e2e.make_yuv(p, 72, 56, 2, 7)
    cfg = _enc.config(72, 56, ["--preset", "fast", "-I", "0", "-b", "0"], 1)
    units = encode.split_nal_units(_enc.encode_cpu(cfg, [open(p, "rb").read()], 2)[0])
    assert _sps([p for nut, _, p in units if nut == 24][0]) == (72, 56, 0, [0, 0, 0, 0])
    assert b" input-res=72x56 " in [p for nut, _, p in units if nut == 28][0]


@pytest.mark.parametrize("w,h,message", [(71, 50, "width must be even"), (70, 51, "height must be even"), (0, 50, "must be positive"), (70, 0, "must be positive"),
                                         (-2, 50, "must be positive"), (8194, 8, "larger than 8192x4320"), (8, 4322, "larger than 8192x4320")])
def test_sizes_outside_the_set_are_refused_with_their_reason(w, h, message):
    from xeve_amd import encode, lib

    with pytest.raises(lib.XeveHipError, match=message):
        encode.footprint(encode.config(w, h, keyint=8, closed_gop=True, crop=True), 1, 2)


@pytest.mark.parametrize("w,h,threads", [(8190, 4318, 1), (8186, 10, 1), (2, 2, 1), (62, 36, 1), (66, 36, 2)])
def test_even_sizes_up_to_the_largest_coded_picture_are_accepted(w, h, threads):
    from xeve_amd import encode

    assert encode.footprint(encode.config(w, h, keyint=8, closed_gop=True, threads=threads, crop=True), 1, 2)[0] > 0


def test_without_the_bit_only_multiples_of_8_are_accepted():
    """reserved[0] bit 5 (config(crop=True)) is what accepts an even size that is no multiple of 8: without it the size is refused as it always was, with a message that
    names the bit; with it an aligned size is what it is without it -- the same footprint, and (tests/test_enc_crop_gpu.py) the same bytes"""
    from xeve_amd import encode, lib

    for w, h in ((70, 50), (130, 64), (128, 60), (2, 2)):
        with pytest.raises(lib.XeveHipError, match="multiple of 8.*bit 5"):
            encode.footprint(encode.config(w, h, keyint=8, closed_gop=True), 1, 2)
        assert encode.footprint(encode.config(w, h, keyint=8, closed_gop=True, crop=True), 1, 2)[0] > 0
    assert encode.config(72, 56, crop=True).reserved[0] & _crop.CROP_BIT and not encode.config(72, 56).reserved[0] & _crop.CROP_BIT
    assert encode.footprint(encode.config(72, 56, keyint=8, closed_gop=True, crop=True), 3, 8) == encode.footprint(encode.config(72, 56, keyint=8, closed_gop=True), 3, 8)


def test_row_chains_are_refused_by_the_coded_width():
    """62x36 is coded 64 wide: one CTU column, where the reference's row threads race"""
    from xeve_amd import encode, lib

    with pytest.raises(lib.XeveHipError, match="one CTU wide"):
        encode.footprint(encode.config(62, 36, keyint=8, closed_gop=True, threads=2, crop=True), 1, 2)


def test_an_aligned_size_costs_what_it_did():
    """120x72, 3 GOPs x 4 frames with measure and keep_recon: the bytes xeve_hip_enc_footprint reported before even sizes were accepted (tests/test_enc_crop_gpu.py
    encodes the same case on the device)"""
    from xeve_amd import encode

    w, h, gops, frames, _, cli, threads = _enc.PICTURE_SIZE_CASES["size_120x72_noise_3gops"]
    c = _enc.config(w, h, cli, threads)
    cfg = encode.config(w, h, qp=c.qp, keyint=c.keyint, bframes=c.bframes, closed_gop=c.closed_gop, preset=c.preset, threads=c.threads, ref=c.ref, measure=True, keep_recon=True)
    assert encode.footprint(cfg, gops, frames) == (16043776, 65535)


def _round256(n):
    return (n + 255) & ~255


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("gops,frames", [(1, 8), (5, 8), (3, 4)])
def test_the_footprint_counts_frames_and_kept_pictures_at_the_input_size(gops, frames, depth):
    """70x50 against 72x56: the same coded picture, so every buffer but the frames' (and, with keep_recon, the kept pictures') has the same size -- the library sums its
    buffers rounded up to 256 bytes each"""
    from xeve_amd import encode

    sb = 2 if depth > 8 else 1
    kw = dict(qp=27, keyint=8, bframes=7, closed_gop=True, input_depth=depth)
    for keep in (False, True):
        small, most_small = encode.footprint(encode.config(70, 50, keep_recon=keep, crop=True, **kw), gops, frames)
        large, most_large = encode.footprint(encode.config(72, 56, keep_recon=keep, **kw), gops, frames)
        assert most_small == most_large
        want = _round256(gops * frames * 72 * 56 * 3 // 2 * sb) - _round256(gops * frames * 70 * 50 * 3 // 2 * sb)
        if keep:
            want += _round256(gops * frames * 72 * 56 * 3) - _round256(gops * frames * 70 * 50 * 3)
        assert large - small == want and want > 0, (keep, large, small, want)
