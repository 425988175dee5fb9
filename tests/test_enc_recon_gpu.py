"""The batch encoder's per-picture report and reconstructed pictures on the GPU (xeve_hip_enc_picture_info / xeve_hip_enc_recon; xeve_amd/encode.py pictures / recon /
recon_into / encode_file): against tests/golden/recon_v1.json, recorded from the unmodified reference application's -r files and -v 3 table
(tests/golden/make_recon_golden.py).  The library's default walk only; nothing of the reference tree is read here."""
import json
import os

import pytest

import _e2e
import _enc

# gpu_full (XEVE_GPU_FULL=1): the default GPU suite is held to the seconds recorded in tests/golden/gpu_suite_durations.json (tests/test_gpu_suite_budget.py), a file of the
# last full run that this change leaves as it is; measured in a run of their own these tests take 7 s together (profiles/recon_measure.md)
pytestmark = [pytest.mark.gpu, pytest.mark.gpu_full]

GOLDEN = json.load(open(os.path.join(_enc.ROOT, "tests", "golden", "recon_v1.json")))
TABLES = dict(list(_enc.BATCH_CASES.items()) + list(_enc.PICTURE_SIZE_CASES.items()) + list(_enc.DEPTH10_CASES.items()))
HALF_ULP = 0.5e-4  # of the application's four printed decimals


@pytest.fixture(scope="module")
def hip():
    import xeve_amd
    from xeve_amd import encode

    xeve_amd.init(0)
    return encode


@pytest.fixture(scope="module")
def yuv_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("enc_recon_gpu_yuv")


def _case(encode, yuv_dir, name, **switches):
    """(configuration, one bytes object per GOP, frames per GOP, the path of the input file)"""
    w, h, gops, frames, seed, cli, threads = TABLES[name]
    p = os.path.join(yuv_dir, name + ".yuv")
    if not os.path.exists(p):
        _e2e.make_yuv(p, w, h, gops * frames, seed)
        if "-d" in cli:
            data = _enc.widen10(open(p, "rb").read())
            open(p, "wb").write(data)
    data = open(p, "rb").read()
    c = _enc.config(w, h, cli, threads)
    cfg = encode.config(w, h, qp=c.qp, keyint=c.keyint, bframes=c.bframes, closed_gop=c.closed_gop, preset=c.preset, threads=c.threads, ref=c.ref, input_depth=c.reserved[1] or 8,
                        **switches)
    fb = len(data) // gops
    return cfg, [data[g * fb:(g + 1) * fb] for g in range(gops)], frames, p


def _encoder(encode, cfg, gops_data, frames):
    enc = encode.BatchEncoder(cfg, len(gops_data), frames)
    for g, d in enumerate(gops_data):
        enc.push_gop(g, d)
    return enc


def _same_picture(got, want, where):
    """got: a dict of BatchEncoder.pictures; want: {"row": [frame, poc, type, tid, qp, bits, psnr_y, psnr_u, psnr_v], "sse": [3]} of the golden"""
    frame, poc, typ, tid, qp, bits = want["row"][:6]
    assert (got["frame"], got["poc"], got["type"], got["tid"], got["qp"]) == (frame, poc, typ, tid, qp), where
    assert got["sse"] == want["sse"], where
    assert got["bytes"] * 8 == bits, where
    for c in range(3):
        assert abs(got["psnr"][c] - want["row"][6 + c]) <= HALF_ULP + 1e-9, (where, c, got["psnr"], want["row"])


def _check_run(enc, name, streams):
    g_enc, g_rec = _enc.golden()["batches"][name], GOLDEN[name]
    assert [(len(s), _enc.md5(s)) for s in streams] == [(p["bytes"], p["md5"]) for p in g_enc["per_gop"]], "the switches must not change a byte"
    for g in range(g_rec["gops"]):
        r = enc.recon(g)
        assert (len(r), _enc.md5(r)) == (g_rec["per_gop"][g]["bytes"], g_rec["per_gop"][g]["md5"]), (name, g)
        pics = enc.pictures(g)
        assert [p["frame"] for p in pics] == list(range(g_rec["frames"]))
        for k, want in enumerate(g_rec["pictures"][g]):  # (the golden lists them as the application prints them: in coding order)
            _same_picture(pics[want["row"][0]], want, (name, g, k))
            assert pics[want["row"][0]]["coding_pos"] == k and pics[want["row"][0]]["idr"] == (k == 0)


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_recon_and_picture_table_equal_the_reference(name, hip, yuv_dir):
    """both switches on: the bitstreams are what they are without them; every GOP's reconstruction is the reference's -r file, every picture's row its table's, the SSE
    the integer the recorder computed from the reference's files; recon_into hands out the same bytes device to device"""
    import torch

    cfg, data, frames, _ = _case(hip, yuv_dir, name, measure=True, keep_recon=True)
    enc = _encoder(hip, cfg, data, frames)
    try:
        _check_run(enc, name, enc.encode())
        w, h = cfg.w, cfg.h
        for g in range(len(data)):
            whole = enc.recon(g)
            for f, dtype, n in ((0, torch.uint8, w * h * 3), (frames - 1, torch.int16, w * h * 3 // 2)):
                t = enc.recon_into(g, f, torch.zeros(n, dtype=dtype, device="cuda:0"))
                assert t.cpu().numpy().tobytes() == whole[f * w * h * 3:(f + 1) * w * h * 3] == enc.recon(g, f), (name, g, f)
    finally:
        enc.close()


def test_each_switch_alone(hip, yuv_dir):
    """measure without keep_recon: the table is served, recon() is refused; keep_recon without measure: the pictures are served, there are no sums and the table is refused"""
    import ctypes as C

    from xeve_amd.lib import XeveHipError, check

    name = "size_24x40_moving"
    g_enc, g_rec = _enc.golden()["batches"][name], GOLDEN[name]
    for switches in (dict(measure=True), dict(keep_recon=True)):
        cfg, data, frames, _ = _case(hip, yuv_dir, name, **switches)
        enc = _encoder(hip, cfg, data, frames)
        try:
            streams = enc.encode()
            assert [(len(s), _enc.md5(s)) for s in streams] == [(p["bytes"], p["md5"]) for p in g_enc["per_gop"]]
            if "measure" in switches:
                pics = enc.pictures(0)
                for k, want in enumerate(g_rec["pictures"][0]):
                    _same_picture(pics[want["row"][0]], want, (switches, k))
                with pytest.raises(XeveHipError, match="bit 3"):
                    enc.recon(0)
                with pytest.raises(XeveHipError, match="bit 3"):
                    enc.recon(0, 1)
            else:
                assert _enc.md5(enc.recon(0)) == g_rec["per_gop"][0]["md5"]
                host = C.create_string_buffer(cfg.w * cfg.h * 3)  # host memory announced as device memory: refused, not copied into
                with pytest.raises(XeveHipError, match="not device memory"):
                    check(enc._L.xeve_hip_enc_recon(enc._h, 0, 0, host, 1))
                assert host.raw == bytes(cfg.w * cfg.h * 3)
                with pytest.raises(XeveHipError, match="bit 2"):
                    enc.pictures(0)
        finally:
            enc.close()


def test_part_way_only_ended_pictures_are_served(hip, yuv_dir):
    """three pictures' steps, then flush(): those three (in CODING order) are served and equal the golden, every other frame is refused -- never a stale or unfinished
    picture; the run then goes on to its end and everything equals the golden"""
    from xeve_amd.lib import XeveHipError

    name = "gops_128x64_noise"
    cfg, data, frames, _ = _case(hip, yuv_dir, name, measure=True, keep_recon=True)
    g_rec = GOLDEN[name]
    enc = _encoder(hip, cfg, data, frames)
    try:
        enc.begin()
        total = enc.advance(0)
        assert total % frames == 0
        for g in range(len(data)):  # nothing has ended yet
            with pytest.raises(XeveHipError, match="not ended"):
                enc.picture(g, 0)
            with pytest.raises(XeveHipError, match="not ended"):
                enc.recon(g, 0)
        assert enc.advance(3 * (total // frames)) == total - 3 * (total // frames)
        enc.flush()
        early = {}
        for g in range(len(data)):
            ended = [want["row"][0] for want in g_rec["pictures"][g][:3]]
            for k, want in enumerate(g_rec["pictures"][g][:3]):
                _same_picture(enc.picture(g, want["row"][0]), want, (g, k))
                early[g, want["row"][0]] = enc.recon(g, want["row"][0])
            for f in set(range(frames)) - set(ended):
                with pytest.raises(XeveHipError, match="not ended"):
                    enc.picture(g, f)
                with pytest.raises(XeveHipError, match="not ended"):
                    enc.recon(g, f)
            with pytest.raises(XeveHipError, match="not ended"):
                enc.recon(g)
            with pytest.raises(XeveHipError, match="out of range"):
                enc.picture(g, frames)
        with pytest.raises(XeveHipError, match="out of range"):
            enc.recon(len(data), 0)
        while enc.advance(1 << 20):
            pass
        enc.sync()
        _check_run(enc, name, enc.bitstreams())
        n = cfg.w * cfg.h * 3
        for (g, f), r in early.items():
            assert r == enc.recon(g)[f * n:(f + 1) * n], (g, f)
    finally:
        enc.close()


def test_a_second_run_of_the_same_object(hip, yuv_dir):
    """begin() again after pushing again: nothing of the first run is served before its pictures end again, and the sums are the same -- set, not added to"""
    from xeve_amd.lib import XeveHipError

    name = "size_8x8_noise"
    cfg, data, frames, _ = _case(hip, yuv_dir, name, measure=True, keep_recon=True)
    enc = _encoder(hip, cfg, data, frames)
    try:
        _check_run(enc, name, enc.encode())
        first = enc.pictures(0)
        enc.push_gop(0, data[0])
        enc.begin()
        with pytest.raises(XeveHipError, match="not ended"):
            enc.picture(0, 0)
        with pytest.raises(XeveHipError, match="not ended"):
            enc.recon(0, 0)
        while enc.advance(1 << 20):
            pass
        enc.sync()
        _check_run(enc, name, enc.bitstreams())
        assert enc.pictures(0) == first
    finally:
        enc.close()


def test_encode_file_writes_the_recon_file_and_the_table(hip, yuv_dir, tmp_path):
    """three GOPs of 120x72: recon_path is the reference's -r file of the WHOLE-sequence run, stats_path one row per picture in the application's columns, GOP after GOP
    in coding order; the bitstream is the whole-sequence run's"""
    name = "size_120x72_noise_3gops"
    cfg, data, frames, yuv = _case(hip, yuv_dir, name)
    g_enc, g_rec = _enc.golden()["batches"][name], GOLDEN[name]
    evc, rec, stats = (str(tmp_path / n) for n in ("out.evc", "rec.yuv", "stats.txt"))
    hip.encode_file(yuv, evc, cfg, len(data), frames, recon_path=rec, stats_path=stats)
    assert _enc.md5(open(evc, "rb").read()) == g_enc["whole"]["md5"]
    r = open(rec, "rb").read()
    assert (len(r), _enc.md5(r)) == (g_rec["whole"]["bytes"], g_rec["whole"]["md5"])
    lines = open(stats).read().splitlines()
    want = [p for g in range(g_rec["gops"]) for p in g_rec["pictures"][g]]
    assert len(lines) == len(want) == g_rec["gops"] * frames
    for line, p in zip(lines, want):
        frame, poc, typ, tid, qp, bits, py, pu, pv = p["row"]
        got = line.split()
        assert got[:4] == [str(poc), str(tid), "(%s)" % typ, str(qp)] and got[7] == str(bits) and len(got) == 8, (line, p)
        for text, printed in zip(got[4:7], (py, pu, pv)):
            assert len(text.split(".")[1]) == 4 and abs(float(text) - printed) <= 1e-4 + 1e-9, (line, p)  # (both are roundings of values half a unit apart at the most)
    assert cfg.reserved[0] & 12 == 0  # the caller's configuration is left as it was
