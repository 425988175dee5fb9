"""The batch encoder's --hash on the GPU (reserved[0] bit 4: a picture-signature SEI with the MD5 of each decoded plane behind every picture, hashed on the device;
xeve_amd/encode.py config(hash=True) / signatures / read_signatures / encode_file): against tests/golden/hash_v1.json, recorded from the unmodified reference
application run with --hash (tests/golden/make_hash_golden.py).  The library's default walk only; nothing of the reference tree is read here."""
import hashlib
import json
import os

import pytest

import _e2e
import _enc

# gpu_full (XEVE_GPU_FULL=1): the default GPU suite is held to the seconds recorded in tests/golden/gpu_suite_durations.json, a file this change leaves as it is
pytestmark = [pytest.mark.gpu, pytest.mark.gpu_full]

GOLDEN = json.load(open(os.path.join(_enc.ROOT, "tests", "golden", "hash_v1.json")))
RECON_GOLDEN = json.load(open(os.path.join(_enc.ROOT, "tests", "golden", "recon_v1.json")))
TABLES = dict(list(_enc.BATCH_CASES.items()) + list(_enc.PICTURE_SIZE_CASES.items()) + list(_enc.DEPTH10_CASES.items()))


@pytest.fixture(scope="module")
def hip():
    import xeve_amd
    from xeve_amd import encode

    xeve_amd.init(0)
    return encode


@pytest.fixture(scope="module")
def yuv_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("enc_hash_gpu_yuv")


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


def _want(p):
    return [bytes.fromhex(x) for x in p["md5"]]


def _check_run(encode, enc, name, streams):
    """every GOP's stream is the reference's --hash stream; signatures() and the stream's own signature units are the golden's, in coding order"""
    case = GOLDEN[name]
    assert [(len(s), _enc.md5(s)) for s in streams] == [(p["bytes"], p["md5"]) for p in case["per_gop"]], name
    for g in range(case["gops"]):
        by_frame = enc.signatures(g)
        assert len(by_frame) == case["frames"]
        assert [by_frame[p["frame"]] for p in case["pictures"][g]] == [_want(p) for p in case["pictures"][g]], (name, g)
        assert encode.read_signatures(streams[g]) == [(p["tid"], _want(p)) for p in case["pictures"][g]], (name, g)
        for p in case["pictures"][g]:
            assert enc.signatures(g, p["frame"]) == _want(p)
    if "whole" in case:
        joined = b"".join(streams)
        assert (len(joined), _enc.md5(joined)) == (case["whole"]["bytes"], case["whole"]["md5"]), name


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_the_hash_stream_and_the_signatures_equal_the_reference(name, hip, yuv_dir):
    cfg, data, frames, _ = _case(hip, yuv_dir, name, hash=True)
    enc = _encoder(hip, cfg, data, frames)
    try:
        _check_run(hip, enc, name, enc.encode())
    finally:
        enc.close()


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_with_the_table_and_the_kept_pictures(name, hip, yuv_dir):
    """measure and keep_recon added: the table's bytes stay the application's Bits / 8 (the signature unit is not counted), and hashlib.md5 of the planes of recon()
    is what signatures() returns and the stream carries"""
    cfg, data, frames, _ = _case(hip, yuv_dir, name, hash=True, measure=True, keep_recon=True)
    enc = _encoder(hip, cfg, data, frames)
    try:
        _check_run(hip, enc, name, enc.encode())
        w, h = cfg.w, cfg.h
        n = w * h * 2
        for g in range(len(data)):
            pics = enc.pictures(g)
            for want in RECON_GOLDEN[name]["pictures"][g]:
                assert pics[want["row"][0]]["bytes"] * 8 == want["row"][5], (name, g, want)
            for f in range(frames):
                r = enc.recon(g, f)
                planes = [r[:n], r[n:n + n // 4], r[n + n // 4:]]
                assert [hashlib.md5(p).digest() for p in planes] == enc.signatures(g, f), (name, g, f)
                assert pics[f]["md5"] == [d.hex() for d in enc.signatures(g, f)]
    finally:
        enc.close()


def test_with_the_switch_off_nothing_changes(hip, yuv_dir):
    from xeve_amd.lib import XeveHipError

    for name in ("size_8x8_noise", "gops_128x128_moving_m2"):
        cfg, data, frames, _ = _case(hip, yuv_dir, name, measure=True)
        enc = _encoder(hip, cfg, data, frames)
        try:
            streams = enc.encode()
            assert [(len(s), _enc.md5(s)) for s in streams] == [(p["bytes"], p["md5"]) for p in _enc.golden()["batches"][name]["per_gop"]]
            assert hip.read_signatures(streams[0]) == []
            assert "md5" not in enc.pictures(0)[0]
            with pytest.raises(XeveHipError, match="bit 4"):
                enc.signatures(0)
            with pytest.raises(XeveHipError, match="bit 4"):
                enc.signatures(0, 0)
        finally:
            enc.close()


def test_part_way_only_ended_pictures_are_served(hip, yuv_dir):
    """three pictures' steps, then flush(): those three (in CODING order) are served and equal the golden, every other frame is refused; the run then goes on to its
    end and everything equals the golden"""
    from xeve_amd.lib import XeveHipError

    name = "gops_128x64_noise"
    cfg, data, frames, _ = _case(hip, yuv_dir, name, hash=True)
    case = GOLDEN[name]
    enc = _encoder(hip, cfg, data, frames)
    try:
        enc.begin()
        total = enc.advance(0)
        assert total % frames == 0
        for g in range(len(data)):
            with pytest.raises(XeveHipError, match="not ended"):
                enc.signatures(g, 0)
        assert enc.advance(3 * (total // frames)) == total - 3 * (total // frames)
        enc.flush()
        for g in range(len(data)):
            first = case["pictures"][g][:3]
            for p in first:
                assert enc.signatures(g, p["frame"]) == _want(p), (g, p["frame"])
            assert hip.read_signatures(enc.bitstream(g)) == [(p["tid"], _want(p)) for p in first]
            for f in set(range(frames)) - {p["frame"] for p in first}:
                with pytest.raises(XeveHipError, match="not ended"):
                    enc.signatures(g, f)
            with pytest.raises(XeveHipError, match="not ended"):
                enc.signatures(g)
            with pytest.raises(XeveHipError, match="out of range"):
                enc.signatures(g, frames)
        with pytest.raises(XeveHipError, match="out of range"):
            enc.signatures(len(data), 0)
        while enc.advance(1 << 20):
            pass
        enc.sync()
        _check_run(hip, enc, name, enc.bitstreams())
    finally:
        enc.close()


def test_a_second_run_of_the_same_object(hip, yuv_dir):
    """begin() again after pushing again: nothing of the first run is served before its pictures end again, and the digests come out the same"""
    from xeve_amd.lib import XeveHipError

    name = "size_8x8_noise"
    cfg, data, frames, _ = _case(hip, yuv_dir, name, hash=True)
    enc = _encoder(hip, cfg, data, frames)
    try:
        _check_run(hip, enc, name, enc.encode())
        first = enc.signatures(0)
        enc.push_gop(0, data[0])
        enc.begin()
        with pytest.raises(XeveHipError, match="not ended"):
            enc.signatures(0, 0)
        while enc.advance(1 << 20):
            pass
        enc.sync()
        _check_run(hip, enc, name, enc.bitstreams())
        assert enc.signatures(0) == first
    finally:
        enc.close()


def test_encode_file_with_hash(hip, yuv_dir, tmp_path):
    """three GOPs of 120x72 through encode_file(hash=True): the whole-sequence run's --hash stream; the table written beside it is the one without --hash"""
    name = "size_120x72_noise_3gops"
    cfg, data, frames, yuv = _case(hip, yuv_dir, name)
    case, g_rec = GOLDEN[name], RECON_GOLDEN[name]
    evc, stats = str(tmp_path / "out.evc"), str(tmp_path / "stats.txt")
    streams = hip.encode_file(yuv, evc, cfg, len(data), frames, stats_path=stats, hash=True)
    out = open(evc, "rb").read()
    assert (len(out), _enc.md5(out)) == (case["whole"]["bytes"], case["whole"]["md5"]) and b"".join(streams) == out
    assert hip.read_signatures(out) == [(p["tid"], _want(p)) for g in range(case["gops"]) for p in case["pictures"][g]]
    want = [p for g in range(g_rec["gops"]) for p in g_rec["pictures"][g]]
    lines = open(stats).read().splitlines()
    assert [int(line.split()[7]) for line in lines] == [p["row"][5] for p in want]
    assert cfg.reserved[0] & 28 == 0  # the caller's configuration is left as it was
