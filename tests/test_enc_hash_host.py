"""CPU suite: the host side of the batch encoder's --hash (reserved[0] bit 4; xeve_hip_md5_planes / xeve_hip_enc_signature / xeve_hip_signature_sei;
xeve_amd/encode.py signatures / signature_sei / split_nal_units / read_signatures): exported symbols, the switch's bit and what it adds to the footprint, the
picture-signature SEI unit against every unit the unmodified reference application wrote (tests/golden/hash_v1.json, made by tests/golden/make_hash_golden.py), the
bitstream helpers on the committed 8x8 stream, the refusal before xeve_hip_init() and by a frame loop whose engine has no digests.  No GPU."""
import ctypes as C
import hashlib
import json
import os

import pytest

import _enc

GOLDEN = json.load(open(os.path.join(_enc.ROOT, "tests", "golden", "hash_v1.json")))
RECON_GOLDEN = json.load(open(os.path.join(_enc.ROOT, "tests", "golden", "recon_v1.json")))
NEW_SYMBOLS = ("xeve_hip_md5_planes", "xeve_hip_enc_signature", "xeve_hip_signature_sei")


def test_the_new_entry_points_are_exported_and_bound():
    from xeve_amd import lib

    L = lib.load()
    for name in NEW_SYMBOLS:
        assert C.c_void_p.in_dll(L, name) is not None and name in lib.FUNCTIONS, name
    src = open(os.path.join(_enc.ROOT, "include", "xeve_hip.h")).read()
    for name in NEW_SYMBOLS + ("xeve_hip_md5_job", "XEVE_HIP_SIGNATURE_SEI_BYTES 56"):
        assert name in src, name
    assert C.sizeof(lib.Md5Job) == 24 and (lib.Md5Job.offset.offset, lib.Md5Job.stride.offset, lib.Md5Job.w.offset, lib.Md5Job.h.offset) == (0, 8, 12, 16)
    assert lib.SIGNATURE_SEI_BYTES == 56


def test_the_bit_is_the_documented_one():
    from xeve_amd import encode

    base = encode.config(128, 64).reserved[0]
    assert encode.config(128, 64, hash=False).reserved[0] == base
    assert encode.config(128, 64, hash=True).reserved[0] == base | 16
    assert encode.config(128, 64, hash=True, measure=True, keep_recon=True, always_second_pass=True, sei_info=False, level_idc=51).reserved[0] == 1 | 2 | 4 | 8 | 16 | (51 << 8)


def _round256(n):
    return (n + 255) & ~255


@pytest.mark.parametrize("w,h,G,F,threads", [(8, 8, 1, 1, 1), (128, 64, 3, 8, 1), (120, 72, 2, 4, 1), (352, 288, 5, 8, 2), (1920, 1080, 4, 8, 8), (3840, 2160, 2, 8, 8)])
def test_the_switch_costs_exactly_the_digest_buffer(w, h, G, F, threads):
    from xeve_amd import encode

    kw = dict(keyint=8, closed_gop=True, preset="medium", threads=threads)
    plain, most = encode.footprint(encode.config(w, h, **kw), G, F)
    hashed, most_hashed = encode.footprint(encode.config(w, h, hash=True, **kw), G, F)
    assert hashed - plain == _round256(G * F * 48)
    assert most_hashed == most
    every, _ = encode.footprint(encode.config(w, h, hash=True, measure=True, keep_recon=True, **kw), G, F)
    assert every - plain == _round256(G * F * 48) + _round256(G * F * w * h * 3) + _round256(G * F * 24)


def _every_unit():
    for name, case in sorted(GOLDEN.items()):
        for g, pics in enumerate(case["pictures"]):
            for k, p in enumerate(pics):
                yield (name, g, k), p


def test_the_signature_unit_is_the_references_for_every_recorded_picture():
    """xeve_hip_signature_sei from a picture's temporal id and digests = the 56 bytes the reference application wrote behind that picture"""
    from xeve_amd import encode, lib

    n = 0
    for where, p in _every_unit():
        unit = encode.signature_sei(p["tid"], [bytes.fromhex(x) for x in p["md5"]])
        assert unit.hex() == p["unit"] and len(unit) == 56 == lib.SIGNATURE_SEI_BYTES, where
        n += 1
    assert n == sum(c["gops"] * c["frames"] for c in GOLDEN.values()) and n > 70
    assert {p["tid"] for _, p in _every_unit()} >= {0, 1, 2}  # more than one temporal id is pinned
    L = lib.load()
    out, d = (C.c_uint8 * 64)(), bytes(48)
    assert L.xeve_hip_signature_sei(0, d, out, 55) == -2 and "invalid argument" in lib.last_error()  # too small a buffer
    assert L.xeve_hip_signature_sei(8, d, out, 64) == -2 and L.xeve_hip_signature_sei(-1, d, out, 64) == -2
    assert L.xeve_hip_signature_sei(0, None, out, 64) == -2 and L.xeve_hip_signature_sei(0, d, None, 64) == -2
    assert bytes(out) == bytes(64)
    assert L.xeve_hip_signature_sei(7, d, out, 64) == 56 and bytes(out[:8]) == bytes([0, 0, 0, 0x34, 0x3B, 0xC0, 0x10, 0x10]) and bytes(out[56:]) == bytes(8)


def test_read_signatures_and_split_nal_units_on_the_committed_stream():
    from xeve_amd import encode

    case = GOLDEN["size_8x8_noise"]
    stream = bytes.fromhex(case["stream"])
    assert (len(stream), hashlib.md5(stream).hexdigest()) == (case["per_gop"][0]["bytes"], case["per_gop"][0]["md5"])
    units = encode.split_nal_units(stream)
    assert sum(6 + len(p) for _, _, p in units) == len(stream)  # consumed exactly
    assert [nut for nut, _, _ in units] == [24, 25, 28, 1, 28] + [0, 28] * 3  # SPS PPS option-SEI IDR signature, then slice + signature per picture
    assert b" hash=1 " in units[2][2] and b" hash=0 " not in units[2][2]
    got = encode.read_signatures(stream)
    assert got == [(p["tid"], [bytes.fromhex(x) for x in p["md5"]]) for p in case["pictures"][0]]
    # without the signature units and with hash=0 the stream is the plain run's (tests/golden/enc_v1.json)
    plain = b"".join((len(p) + 2).to_bytes(4, "big") + (((nut + 1) << 9) | (tid << 6)).to_bytes(2, "big") + p for nut, tid, p in units if not (nut == 28 and p[:2] == b"\x10\x10"))
    plain = plain.replace(b" hash=1 ", b" hash=0 ")
    want = _enc.golden()["batches"]["size_8x8_noise"]["per_gop"][0]
    assert (len(plain), hashlib.md5(plain).hexdigest()) == (want["bytes"], want["md5"])
    assert encode.read_signatures(plain) == []
    for cut in (stream[:-1], stream[:3], stream + b"\0", stream + bytes([0, 0, 0, 1, 0])):
        with pytest.raises(ValueError):
            encode.split_nal_units(cut)
    assert encode.split_nal_units(b"") == []


def test_uninitialised_use_fails_loudly():
    """before xeve_hip_init() the two device entry points refuse as the existing ones do (XEVE_HIP_ERR_UNINIT; XEVE_HIP_ERR_ARG for their NULL arguments where an earlier
    test of the same process has initialised the library); xeve_hip_signature_sei is host only and works either way"""
    from xeve_amd import lib

    L = lib.load()
    initialised = L.xeve_hip_avg(None, None, None, 0, None) != -3
    out = (C.c_uint8 * 48)()
    for call in (lambda: L.xeve_hip_md5_planes(None, None, 1, None, None), lambda: L.xeve_hip_enc_signature(None, 0, 0, out)):
        rc = call()
        assert rc == (-2 if initialised else -3) and ("invalid argument" if initialised else "xeve_hip_init") in lib.last_error()
    unit = (C.c_uint8 * 56)()
    assert L.xeve_hip_signature_sei(0, bytes(48), unit, 56) == 56


def test_the_golden_is_consistent_with_the_other_goldens():
    enc = _enc.golden()["batches"]
    assert sorted(GOLDEN) == sorted(RECON_GOLDEN) and len(GOLDEN) == 9
    for name, case in GOLDEN.items():
        assert (case["w"], case["h"], case["gops"], case["frames"]) == tuple(enc[name][k] for k in ("w", "h", "gops", "frames"))
        assert len(case["per_gop"]) == len(case["pictures"]) == case["gops"]
        for g, pics in enumerate(case["pictures"]):
            assert len(pics) == case["frames"]  # one signature unit per picture
            assert case["per_gop"][g]["bytes"] == enc[name]["per_gop"][g]["bytes"] + 56 * case["frames"]
            rows = RECON_GOLDEN[name]["pictures"][g]
            assert [(p["frame"], p["tid"]) for p in pics] == [(r["row"][0], r["row"][3]) for r in rows]  # the same pictures in the same (coding) order
            assert sorted(p["frame"] for p in pics) == list(range(case["frames"]))
            for p in pics:
                assert len(p["unit"]) == 112 and all(len(x) == 32 for x in p["md5"]) and p["unit"][16:] == "".join(p["md5"])
        assert ("whole" in case) == (case["gops"] > 1)
        if case["gops"] > 1:
            assert case["whole"]["bytes"] == sum(p["bytes"] for p in case["per_gop"])
    assert "stream" in GOLDEN["size_8x8_noise"] and len(GOLDEN["size_8x8_noise"]["stream"]) < 4096


def test_a_frame_loop_whose_engine_has_no_digests_refuses_hash():
    """the CPU harness instantiates the product's frame loop with an engine that hashes nothing: begin() refuses bit 4 with a message instead of writing a stream
    without signatures; without the bit the same call codes"""
    import _e2e

    w, h, gops, frames, seed, cli, threads = _enc.PICTURE_SIZE_CASES["size_8x8_noise"]
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "in.yuv")
        _e2e.make_yuv(p, w, h, gops * frames, seed)
        data = open(p, "rb").read()
    cfg = _enc.config(w, h, cli, threads)
    want = _enc.golden()["batches"]["size_8x8_noise"]["per_gop"][0]
    assert [_enc.md5(s) for s in _enc.encode_cpu(cfg, [data], frames)] == [want["md5"]]
    cfg.reserved[0] |= 16
    with pytest.raises(RuntimeError, match="--hash needs an engine"):
        _enc.encode_cpu(cfg, [data], frames)
