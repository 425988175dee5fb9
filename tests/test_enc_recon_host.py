"""CPU suite: the host side of the batch encoder's per-picture report and reconstructed pictures (xeve_hip_enc_picture_info / xeve_hip_enc_recon /
xeve_hip_recon_measure; xeve_amd/encode.py pictures / recon): exported symbols, the record's layout, what the two switches (reserved[0] bits 2 and 3) add to the
footprint, the PSNR formula against the reference application's printed table (tests/golden/recon_v1.json), and the refusal before xeve_hip_init().  No GPU."""
import ctypes as C
import json
import math
import os

import pytest

import _enc

RECON_GOLDEN = json.load(open(os.path.join(_enc.ROOT, "tests", "golden", "recon_v1.json")))
NEW_SYMBOLS = ("xeve_hip_recon_measure", "xeve_hip_enc_picture_info", "xeve_hip_enc_recon")


def test_the_new_entry_points_are_exported_and_bound():
    from xeve_amd import lib

    L = lib.load()
    for name in NEW_SYMBOLS:
        assert C.c_void_p.in_dll(L, name) is not None and name in lib.FUNCTIONS, name
    src = open(os.path.join(_enc.ROOT, "include", "xeve_hip.h")).read()
    for name in NEW_SYMBOLS + ("xeve_hip_enc_picture",):
        assert name in src, name


def test_the_picture_record_has_the_headers_layout():
    """xeve_hip_enc_picture as include/xeve_hip.h declares it: eight 32-bit fields, then bytes, sse[3], psnr[3] -- 32 + 8 + 24 + 24 = 88 bytes, no padding (encode.hip
    holds the same numbers in a static_assert)"""
    from xeve_amd import lib

    P = lib.EncPicture
    assert C.sizeof(P) == 88
    assert [getattr(P, n).offset for n in "frame poc slice_type tid qp idr coding_pos reserved".split()] == list(range(0, 32, 4))
    assert (P.bytes.offset, P.sse.offset, P.psnr.offset) == (32, 40, 64)
    assert (P.bytes.size, P.sse.size, P.psnr.size) == (8, 24, 24)


def _round256(n):  # the footprint counts every buffer at the allocator's granularity, as it does for the buffers it already has
    return (n + 255) & ~255


@pytest.mark.parametrize("w,h,G,F,threads", [(8, 8, 1, 1, 1), (128, 64, 3, 8, 1), (120, 72, 2, 4, 1), (352, 288, 5, 8, 2), (1920, 1080, 4, 8, 8), (3840, 2160, 2, 8, 8)])
def test_the_switches_cost_exactly_their_buffers(w, h, G, F, threads):
    from xeve_amd import encode

    kw = dict(keyint=8, closed_gop=True, preset="medium", threads=threads)
    plain, most = encode.footprint(encode.config(w, h, **kw), G, F)
    explicit_off, _ = encode.footprint(encode.config(w, h, measure=False, keep_recon=False, **kw), G, F)
    assert encode.config(w, h, **kw).reserved[0] == encode.config(w, h, measure=False, keep_recon=False, **kw).reserved[0] and explicit_off == plain
    kept, most_kept = encode.footprint(encode.config(w, h, keep_recon=True, **kw), G, F)
    measured, most_measured = encode.footprint(encode.config(w, h, measure=True, **kw), G, F)
    both, _ = encode.footprint(encode.config(w, h, measure=True, keep_recon=True, **kw), G, F)
    assert kept - plain == _round256(G * F * w * h * 3)
    assert measured - plain == _round256(G * F * 24)
    assert both - plain == _round256(G * F * w * h * 3) + _round256(G * F * 24)
    assert most_kept == most_measured == most  # (the batch's addressing limits do not move; what fits the free memory is plan_batches' arithmetic on the footprint)


def test_the_bits_are_the_documented_ones():
    from xeve_amd import encode

    base = encode.config(128, 64).reserved[0]
    assert encode.config(128, 64, measure=True).reserved[0] == base | 4
    assert encode.config(128, 64, keep_recon=True).reserved[0] == base | 8
    assert encode.config(128, 64, measure=True, keep_recon=True, always_second_pass=True, sei_info=False, level_idc=51).reserved[0] == 1 | 2 | 4 | 8 | (51 << 8)


def test_plan_batches_sees_the_larger_footprint():
    """3840x2160, 8-frame GOPs: the kept pictures are 199 MB per GOP, and a round of batches holds fewer GOPs in the same memory"""
    from xeve_amd import encode

    kw = dict(keyint=8, closed_gop=True, preset="medium", threads=8)
    one, _ = encode.footprint(encode.config(3840, 2160, keep_recon=True, **kw), 1, 8)
    two, _ = encode.footprint(encode.config(3840, 2160, keep_recon=True, **kw), 2, 8)
    one0, _ = encode.footprint(encode.config(3840, 2160, **kw), 1, 8)
    two0, _ = encode.footprint(encode.config(3840, 2160, **kw), 2, 8)
    assert (two - one) - (two0 - one0) == 8 * 3840 * 2160 * 3 == 199065600
    free = 64 << 30
    held = lambda cfg: sum(n for _, n in encode.plan_batches(cfg, 10000, 8, free)[0])
    assert held(encode.config(3840, 2160, keep_recon=True, **kw)) < held(encode.config(3840, 2160, **kw))


def test_the_psnr_helper_reproduces_the_applications_table():
    from xeve_amd import encode

    n = 0
    for name, case in RECON_GOLDEN.items():
        samples = (case["w"] * case["h"], case["w"] * case["h"] // 4, case["w"] * case["h"] // 4)
        for gop in case["pictures"]:
            for pic in gop:
                for c in range(3):
                    assert abs(encode.psnr(pic["sse"][c], samples[c]) - pic["row"][6 + c]) <= 0.5e-4 + 1e-9, (name, pic)
                    n += 1
    assert n == 3 * sum(case["gops"] * case["frames"] for case in RECON_GOLDEN.values()) and n > 200
    assert encode.psnr(0, 64) == 100.0
    assert abs(encode.psnr(64 * 16, 64) - 20 * math.log10(255)) < 1e-9  # an error of one 8-bit step (four at 10 bits) everywhere


def test_the_stats_line_is_the_applications_row():
    from xeve_amd import encode

    line = encode.stats_line({"poc": 8, "tid": 0, "type": "B", "qp": 37, "psnr": [29.12346, 38.5, 100.0], "bytes": 123})
    assert line.split() == ["8", "0", "(B)", "37", "29.1235", "38.5000", "100.0000", "984"]


def test_the_golden_holds_what_the_gpu_tests_compare_against():
    enc = _enc.golden()["batches"]
    assert len(RECON_GOLDEN) == 9
    for name, case in RECON_GOLDEN.items():
        assert (case["w"], case["h"], case["gops"], case["frames"]) == tuple(enc[name][k] for k in ("w", "h", "gops", "frames"))
        assert len(case["per_gop"]) == len(case["pictures"]) == case["gops"]
        for g, pics in enumerate(case["pictures"]):
            assert case["per_gop"][g]["bytes"] == case["frames"] * case["w"] * case["h"] * 3
            assert sorted(p["row"][0] for p in pics) == list(range(case["frames"]))
            assert sum(p["row"][5] for p in pics) == 8 * enc[name]["per_gop"][g]["bytes"]  # the application's Bits column sums to the bitstream
        assert ("whole" in case) == (case["gops"] > 1)


def test_uninitialised_use_fails_loudly():
    """before xeve_hip_init() the new entry points refuse as the existing ones do (XEVE_HIP_ERR_UNINIT); where an earlier test of the same process has initialised the
    library, the NULL arguments are refused instead (XEVE_HIP_ERR_ARG) -- a message either way, never a crash"""
    from xeve_amd import lib

    L = lib.load()
    initialised = L.xeve_hip_avg(None, None, None, 0, None) != -3
    pic = lib.EncPicture()
    calls = (lambda: L.xeve_hip_recon_measure(None, 0, 0, 0, 0, None, 0, 0, 0, 0, 8, 8, 1, None, 0, None, None), lambda: L.xeve_hip_enc_picture_info(None, 0, 0, C.byref(pic)),
             lambda: L.xeve_hip_enc_recon(None, 0, 0, None, 0))
    for call in calls:
        rc = call()
        assert rc == (-2 if initialised else -3) and ("invalid argument" if initialised else "xeve_hip_init") in lib.last_error()
