"""The batch encoder on the GPU at even picture sizes that are no multiple of 8 (xeve_amd/csrc/encode.hip with frames.hip: the pushed frames padded on the device, the
reconstructed pictures cropped again) against tests/golden/crop_v1.json, recorded from the unmodified reference application (tests/golden/make_crop_golden.py): the
bitstreams, the application's table rows -- whose PSNRs run over the CODED planes, zero padding included --, the cropped -r files, and with --hash the signature units,
whose digests are over the coded planes and therefore NOT the md5 of the -r planes.  Nothing of the reference tree is read here."""
import pytest

import _crop
import _enc

# gpu_full (XEVE_GPU_FULL=1): as the reconstruction and signature tests (tests/test_enc_recon_gpu.py), kept out of the default GPU suite and its recorded durations
pytestmark = [pytest.mark.gpu, pytest.mark.gpu_full]

GOLDEN = _crop.golden()
HALF_ULP = 0.5e-4  # of the application's four printed decimals
COMPOSED, FUSED, BY_WIDTH = 0, 1, -1
FUSED_ONLY = ("crop_202x138_slow_m3",)  # preset slow lives on the fused walk


@pytest.fixture(scope="module")
def hip():
    import xeve_amd
    from xeve_amd import encode

    xeve_amd.init(0)
    return encode


@pytest.fixture(scope="module")
def yuv_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("enc_crop_gpu_yuv")


def _run(hip, yuv_dir, name, walk=BY_WIDTH, on_device=False, **switches):
    """both GOPs of a case in one batch -> (the encoder, still open, and its bitstreams)"""
    w, h, gops, frames = _crop.CASES[name][:4]
    cfg = _crop.product_config(hip, name, **switches)
    _, data = _crop.clip(yuv_dir, name)
    with hip.walk_select(FUSED if name in FUSED_ONLY else walk):
        enc = hip.BatchEncoder(cfg, gops, frames)
        try:
            assert enc.frame_bytes * frames == len(data[0])  # frames of the INPUT size
            if on_device:
                import torch

                for g in range(gops):
                    src = torch.frombuffer(bytearray(data[g]), dtype=torch.uint8).cuda()
                    for f in range(frames):
                        enc.push(g, f, src[f * enc.frame_bytes:(f + 1) * enc.frame_bytes])  # (frames of 5250 bytes back to back: most start on 2-byte boundaries only)
            else:
                for g in range(gops):
                    enc.push_gop(g, data[g])
            return enc, enc.encode()
        except Exception:
            enc.close()
            raise


def _same_rows(enc, name):
    g_case = GOLDEN[name]
    for g in range(g_case["gops"]):
        pics = enc.pictures(g)
        assert [p["frame"] for p in pics] == list(range(g_case["frames"]))
        for k, want in enumerate(g_case["pictures"][g]):  # (the golden lists them as the application prints them: in coding order)
            frame, poc, typ, tid, qp, bits = want["row"][:6]
            got, where = pics[frame], (name, g, k)
            assert (got["frame"], got["poc"], got["type"], got["tid"], got["qp"], got["coding_pos"], got["idr"]) == (frame, poc, typ, tid, qp, k, k == 0), where
            assert got["bytes"] * 8 == bits, where
            for c in range(3):
                assert abs(got["psnr"][c] - want["row"][6 + c]) <= HALF_ULP + 1e-9, (where, c, got["psnr"], want["row"])


def _same_recon(enc, name):
    w, h, _, frames = _crop.CASES[name][:4]
    for g, want in enumerate(GOLDEN[name]["recon"]["per_gop"]):
        r = enc.recon(g)
        assert len(r) == frames * w * h * 3 == want["bytes"] and _enc.md5(r) == want["md5"], (name, g)


def _same_streams(streams, want, where):
    assert [(len(s), _enc.md5(s)) for s in streams] == [(p["bytes"], p["md5"]) for p in want], where


@pytest.mark.parametrize("name", sorted(_crop.CASES))
def test_streams_rows_and_recon_equal_the_reference(name, hip, yuv_dir):
    """every case on the library's choice of walk, both GOPs in one batch, both switches on"""
    enc, streams = _run(hip, yuv_dir, name, measure=True, keep_recon=True)
    try:
        _same_streams(streams, GOLDEN[name]["per_gop"], name)
        _same_rows(enc, name)
        _same_recon(enc, name)
    finally:
        enc.close()


@pytest.mark.parametrize("walk", [COMPOSED, FUSED], ids=["composed", "fused"])
def test_both_walks_pinned(walk, hip, yuv_dir):
    name = "crop_70x50_ra_medium"
    enc, streams = _run(hip, yuv_dir, name, walk=walk, measure=True, keep_recon=True)
    try:
        _same_streams(streams, GOLDEN[name]["per_gop"], (name, walk))
        _same_rows(enc, name)
        _same_recon(enc, name)
    finally:
        enc.close()


def test_each_switch_alone_and_none(hip, yuv_dir):
    """keep_recon without measure (the crop kernel alone), measure without keep_recon (the sums over the coded planes alone), neither: the same bytes every time"""
    name = "crop_70x50_ra_medium"
    for switches in (dict(keep_recon=True), dict(measure=True), dict()):
        enc, streams = _run(hip, yuv_dir, name, **switches)
        try:
            _same_streams(streams, GOLDEN[name]["per_gop"], switches)
            if "keep_recon" in switches:
                _same_recon(enc, name)
            if "measure" in switches:
                _same_rows(enc, name)
        finally:
            enc.close()


def test_hash_signs_the_coded_planes(hip, yuv_dir):
    """--hash: the stream with the signature units is the reference's, signatures() are the digests in it -- over the 72x56 coded planes, so none of them is the md5 of
    the cropped plane recon() hands out; the table and the -r file stay what they are without the switch"""
    import hashlib

    name = _crop.HASH_CASE
    w, h, gops, frames = _crop.CASES[name][:4]
    want = GOLDEN[name]["hash"]
    enc, streams = _run(hip, yuv_dir, name, hash=True, measure=True, keep_recon=True)
    try:
        _same_streams(streams, want["per_gop"], name)
        _same_rows(enc, name)
        _same_recon(enc, name)
        for g in range(gops):
            sig, rec = enc.signatures(g), enc.recon(g)
            for p in want["pictures"][g]:
                assert [d.hex() for d in sig[p["frame"]]] == p["md5"], (g, p["frame"])
            assert [(tid, [d.hex() for d in ds]) for tid, ds in hip.read_signatures(streams[g])] == [(p["tid"], p["md5"]) for p in want["pictures"][g]]
            assert hashlib.md5(rec[:w * h * 2]).digest() != sig[0][0]  # (the digest covers the padding columns and rows as well)
    finally:
        enc.close()


def test_10_bit_input(hip, yuv_dir):
    name = "crop_70x50_ra_medium_10bit"
    enc, streams = _run(hip, yuv_dir, name, measure=True, keep_recon=True)
    try:
        assert enc.frame_bytes == 70 * 50 * 3
        _same_streams(streams, GOLDEN[name]["per_gop"], name)
        _same_rows(enc, name)
        _same_recon(enc, name)
    finally:
        enc.close()


def test_frames_pushed_from_device_memory(hip, yuv_dir):
    import torch

    name = "crop_70x50_ra_medium"
    w, h, gops, frames = _crop.CASES[name][:4]
    enc, streams = _run(hip, yuv_dir, name, on_device=True, keep_recon=True)
    try:
        _same_streams(streams, GOLDEN[name]["per_gop"], name)
        _same_recon(enc, name)
        whole = enc.recon(1)
        t = enc.recon_into(1, frames - 1, torch.empty(w * h * 3, dtype=torch.uint8, device="cuda:0"))  # the cropped picture, device to device
        assert t.cpu().numpy().tobytes() == whole[(frames - 1) * w * h * 3:] == enc.recon(1, frames - 1)
    finally:
        enc.close()


def test_encode_file_writes_the_cropped_recon_file_and_the_table(hip, yuv_dir, tmp_path):
    """the whole clip through encode_file: the bitstream and the -r file of the reference's whole-sequence run, one table row per picture in the application's columns"""
    name = "crop_70x50_ra_medium"
    w, h, gops, frames = _crop.CASES[name][:4]
    yuv, _ = _crop.clip(yuv_dir, name)
    cfg, g_case = _crop.product_config(hip, name), GOLDEN[name]
    evc, rec, stats = (str(tmp_path / n) for n in ("out.evc", "rec.yuv", "stats.txt"))
    hip.encode_file(yuv, evc, cfg, gops, frames, recon_path=rec, stats_path=stats)
    b, r = open(evc, "rb").read(), open(rec, "rb").read()
    assert (len(b), _enc.md5(b)) == (g_case["whole"]["bytes"], g_case["whole"]["md5"])
    assert len(r) == gops * frames * w * h * 3 and (len(r), _enc.md5(r)) == (g_case["recon"]["whole"]["bytes"], g_case["recon"]["whole"]["md5"])
    lines = open(stats).read().splitlines()
    want = [p for g in range(gops) for p in g_case["pictures"][g]]
    assert len(lines) == len(want) == gops * frames
    for line, p in zip(lines, want):
        frame, poc, typ, tid, qp, bits, py, pu, pv = p["row"]
        got = line.split()
        assert got[:4] == [str(poc), str(tid), "(%s)" % typ, str(qp)] and got[7] == str(bits) and len(got) == 8, (line, p)
        for text, printed in zip(got[4:7], (py, pu, pv)):
            assert len(text.split(".")[1]) == 4 and abs(float(text) - printed) <= 1e-4 + 1e-9, (line, p)  # (both are roundings of values half a unit apart at the most)


# xeve_hip_enc_footprint of tests/_enc.py PICTURE_SIZE_CASES "size_120x72_noise_3gops" (3 GOPs x 4 frames, measure and keep_recon on) as the library reported it before
# even sizes were accepted: the aligned path allocates what it did
ALIGNED_GUARD = ("size_120x72_noise_3gops", 16043776)


@pytest.mark.parametrize("crop", [False, True], ids=["plain", "crop_bit"])
def test_an_aligned_size_stays_on_its_path(crop, hip, yuv_dir):
    """120x72 is a multiple of 8 both ways: the same footprint as before, the bitstreams of tests/golden/enc_v1.json, the -r files of recon_v1.json -- without the bit that
    accepts any even size and with it (nothing is padded or cropped: the SPS has no window)"""
    import json
    import os

    import _e2e

    name, footprint = ALIGNED_GUARD
    w, h, gops, frames, seed, cli, threads = _enc.PICTURE_SIZE_CASES[name]
    c = _enc.config(w, h, cli, threads)
    cfg = hip.config(w, h, qp=c.qp, keyint=c.keyint, bframes=c.bframes, closed_gop=c.closed_gop, preset=c.preset, threads=c.threads, ref=c.ref, measure=True, keep_recon=True,
                     crop=crop)
    assert hip.footprint(cfg, gops, frames)[0] == footprint
    p = os.path.join(str(yuv_dir), name + ".yuv")
    _e2e.make_yuv(p, w, h, gops * frames, seed)
    data = open(p, "rb").read()
    fb = len(data) // gops
    enc = hip.BatchEncoder(cfg, gops, frames)
    try:
        for g in range(gops):
            enc.push_gop(g, data[g * fb:(g + 1) * fb])
        _same_streams(enc.encode(), _enc.golden()["batches"][name]["per_gop"], name)
        rec = json.load(open(os.path.join(_enc.ROOT, "tests", "golden", "recon_v1.json")))[name]
        for g in range(gops):
            r = enc.recon(g)
            assert (len(r), _enc.md5(r)) == (rec["per_gop"][g]["bytes"], rec["per_gop"][g]["md5"]), g
    finally:
        enc.close()


def test_without_the_bit_the_size_is_refused(hip):
    """70x50 without config(crop=True): refused at create, with the message that names the bit"""
    import xeve_amd

    with pytest.raises(xeve_amd.XeveHipError, match="multiple of 8.*bit 5"):
        hip.BatchEncoder(hip.config(70, 50, keyint=8, closed_gop=True), 1, 1)
