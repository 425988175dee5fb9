"""Batches of the closed-GOP encoder: what a batch costs (xeve_hip_enc_footprint -- host arithmetic, no device), how a job larger than a batch is cut
(xeve_amd/encode.py plan_batches), and -- on the GPU -- that GOPs coded in several batches side by side, in several rounds, are the reference's bitstreams."""
import pytest

import _enc
from xeve_amd import encode


def _cfg(w, h, threads=8):
    return encode.config(w, h, qp=32, keyint=8, bframes=15, closed_gop=True, preset="medium", threads=threads)


def test_a_batch_ends_where_its_halved_offsets_into_the_stacked_originals_reach_32_bits():
    """the library's own job records count PAIRS of samples (xh_common.h XH_OFF2_HALF): 2^33 samples of stacked originals per batch -- 896 pictures of 3840x2160, more
    than a GPU's HBM holds of 8-frame GOPs, so a GPU's job is ONE batch"""
    c = _cfg(3840, 2160)
    assert encode.footprint(c, 1, 2)[1] == 896  # (2496 rows x 3840 samples per stacked picture)
    assert encode.footprint(_cfg(1920, 1080), 1, 2)[1] == (2 ** 33 - 1) // (1408 * 1920)
    encode.footprint(c, 896, 2)
    with pytest.raises(Exception):
        encode.footprint(c, 897, 2)


@pytest.mark.parametrize("threads", [1, 8])
def test_the_largest_accepted_picture_has_a_footprint_and_its_batch_the_three_limits(threads):
    """8192x4320, the upper end of what Param::finish takes: the call succeeds, and max_gops is the smallest of the three limits xeve_hip_enc_footprint names -- GOPs x row
    chains a grid dimension (65535), a stacked picture's rows in 1/16 sample units in 31 bits, the stacked originals below 2^33 samples -- derived here from the sizes:
    a stacked picture is 4320 + 2 * 144 rows rounded up to 64 = 4608"""
    vh = (4320 + 2 * 144 + 63) // 64 * 64
    assert vh == 4608
    limits = (65535 // threads, (2 ** 31 - 1) // (vh * 32), (2 ** 33 - 1) // (vh * 8192))
    assert limits == ((65535, 14563, 227) if threads == 1 else (8191, 14563, 227))
    need, most = encode.footprint(_cfg(8192, 4320, threads), 1, 2)
    assert most == min(limits) == 227 and need > 2 * 8192 * 4320 * 3  # (more than the two pictures' 16-bit samples)
    encode.footprint(_cfg(8192, 4320, threads), 227, 2)
    with pytest.raises(Exception):
        encode.footprint(_cfg(8192, 4320, threads), 228, 2)


def test_the_footprint_is_linear_in_the_gops_and_grows_with_the_frames():
    c = _cfg(3840, 2160)
    b = [encode.footprint(c, n, 2)[0] for n in (1, 2, 3, 896)]
    assert abs((b[1] - b[0]) - (b[2] - b[1])) <= 65536  # (the composed walk's workspace is some forty arrays, each rounded up to 256 bytes)
    per_gop = b[1] - b[0]
    assert 200e6 < per_gop < 300e6  # two picture stores, original, input, maps, both CTU stores in the writer's form, the walk's state of 8 chains
    # (the walk's workspace is the composed walk's at every width since round 6 -- walk.hip; rounds 4-5: the fused kernel's up to 1024 chains)
    assert abs(b[3] - 896 * per_gop) < 0.01 * b[3]
    w = [encode.footprint(c, n, 2)[0] for n in (200, 300, 400)]
    assert abs((w[1] - w[0]) - (w[2] - w[1])) <= 65536 and abs((w[1] - w[0]) / 100 - per_gop) < 0.01 * per_gop
    assert encode.footprint(c, 16, 8)[0] > encode.footprint(c, 16, 2)[0]  # more frames to hold, more picture stores alive
    assert encode.footprint(_cfg(3840, 2160, threads=1), 16, 2)[0] < encode.footprint(c, 16, 2)[0]  # one chain: no second pass, no CTU stores


def test_a_job_is_cut_into_rounds_of_batches_that_fit():
    c = _cfg(3840, 2160)
    per_gop = encode.footprint(c, 2, 2)[0] - encode.footprint(c, 1, 2)[0]
    free = 286 * 10 ** 9
    rounds = encode.plan_batches(c, 3000, 2, free)
    flat = [b for r in rounds for b in r]
    assert [f for f, _ in flat] == [sum(n for _, n in flat[:i]) for i in range(len(flat))] and sum(n for _, n in flat) == 3000  # every GOP once, in order
    for r in rounds:
        assert len(r) <= 3 and all(1 <= n <= 896 for _, n in r)
        assert sum(n for _, n in r) * per_gop <= free - (8 << 30)
    assert rounds[0][0][1] == 896  # a round is filled as far as the limit and the memory go
    assert encode.plan_batches(c, 5, 2, free) == [[(0, 5)]]
    assert encode.plan_batches(c, 10, 2, free, max_batches=2, batch_gops=4) == [[(0, 4), (4, 4)], [(8, 2)]]
    with pytest.raises(Exception):
        encode.plan_batches(c, 5, 2, 1 << 20)


def test_the_slice_buffer_is_sized_by_the_runs_lowest_slice_qp():
    """tests/golden/slice_bytes_v1.json and slice_bytes_binary_v1.json (make_slice_bytes_golden.py): what the unmodified reference spends on a picture of i.i.d. uniform
    noise and of i.i.d. BINARY noise (every sample 0 or 255 -- the densest content found, 1.25 .. 2.2 times the bytes of uniform noise) at every -q, 128x64 all-intra; the
    binary table also holds the I and the inter picture of a low-delay run per -q, each under the slice QP the application reports.  A picture's slice buffer holds
    1.25 x the larger rate at 128x64 and at 3840x2160 -- the margin covers the rate's dependence on the picture size and on the picture type -- and stays
    w * h * 3 / 2 + 4096 wherever that already does (-q 32, the benchmark's, among them: its footprint must not move)"""
    import json
    import os

    t, tb = (json.load(open(os.path.join(_enc.ROOT, "tests", "golden", n))) for n in ("slice_bytes_v1.json", "slice_bytes_binary_v1.json"))
    rate = [0.0] * 52  # the most bytes per sample of any recorded picture of slice QP q
    for tab in (t, tb):
        assert [r["q"] for r in tab["per_q"]] == list(range(52)) and tab["samples_per_picture"] == 128 * 64 * 3 // 2
        for r in tab["per_q"]:
            assert r["bytes_per_sample"] == max(r["slice_bytes"]) / tab["samples_per_picture"]
            rate[r["q"]] = max(rate[r["q"]], r["bytes_per_sample"])
    for r in tb["per_q"]:
        assert r["bytes_per_sample"] > 1.25 * t["per_q"][r["q"]]["bytes_per_sample"]  # (binary noise IS the denser one, at every QP)
        assert len(r["low_delay_slice_bytes"]) == len(r["low_delay_slice_qp"]) == 2 and r["low_delay_slice_qp"][0] == max(0, r["q"] - 1) < r["low_delay_slice_qp"][1]
        for n, q in zip(r["low_delay_slice_bytes"], r["low_delay_slice_qp"]):
            rate[q] = max(rate[q], n / tb["samples_per_picture"])
    kept = {}
    for w, h in ((128, 64), (3840, 2160)):
        samples, before = w * h * 3 // 2, w * h * 3 // 2 + 4096
        for q in range(52):
            need = 1.25 * rate[q] * samples
            cap = encode.slice_capacity(encode.config(w, h, qp=q, keyint=1, bframes=0, preset="fast"), 2)  # (all-intra: every slice QP is -q)
            assert cap >= need, (w, h, q, cap, need)
            assert q == 0 or cap <= encode.slice_capacity(encode.config(w, h, qp=q - 1, keyint=1, bframes=0, preset="fast"), 2)  # monotone
            if before >= need:
                assert cap == before, (w, h, q, cap, before)
                kept.setdefault((w, h), []).append(q)
    assert 32 in kept[(128, 64)] and 32 in kept[(3840, 2160)] and min(kept[(3840, 2160)]) > 0  # (and the low end is NOT kept: the rule is needed)
    assert kept[(128, 64)] == list(range(24, 52)) and kept[(3840, 2160)] == list(range(28, 52))  # (what DESIGN.md section 2 and enc_plan.h say about the floor)
    # the benchmark's configuration (bench.py: -q 32, closed GOPs of 8 frames, 8 row chains) keeps its footprint to the byte.  The four figures are what
    # encode.footprint(c, 1, 8)[0] and encode.footprint(c, 2, 8)[0] returned from a build of the commit before the binary table (uniform-noise k[] alone), read off there
    for (w, h), one, two in (((3840, 2160), 390476544, 780881920), ((1920, 1080), 134949120, 269827072)):
        c = encode.config(w, h, qp=32, keyint=8, bframes=15, closed_gop=True, preset="medium", threads=8)
        assert encode.slice_capacity(c, 8) == w * h * 3 // 2 + 4096
        assert (encode.footprint(c, 1, 8)[0], encode.footprint(c, 2, 8)[0]) == (one, two)
    # the lowest slice QP of the run counts, not -q: the low-delay hierarchy codes its I picture at -q - 1, the 16-picture random-access one at -q - 3 -- where a run has one
    q0 = encode.slice_capacity(encode.config(128, 64, qp=0, keyint=1, bframes=0, preset="fast"), 2)
    assert encode.slice_capacity(encode.config(128, 64, qp=1, keyint=0, bframes=0, preset="fast"), 3) == q0 > 10.1 * 1.25 * 128 * 64 * 3 // 2
    q12 = encode.slice_capacity(encode.config(128, 64, qp=12, keyint=1, bframes=0, preset="fast"), 2)
    assert encode.slice_capacity(encode.config(128, 64, qp=15, keyint=0, bframes=15, preset="medium"), 17) == q12
    # and the footprint carries it: per GOP, the slice buffer's growth and nothing else
    a, b = (encode.config(3840, 2160, qp=q, keyint=8, bframes=15, closed_gop=True, preset="medium", threads=8) for q in (32, 10))
    grow = encode.slice_capacity(b, 8) - encode.slice_capacity(a, 8)
    assert grow > 0 and encode.footprint(b, 256, 8)[0] - encode.footprint(a, 256, 8)[0] == 256 * grow  # (256 GOPs: both buffers end on the allocator's 256-byte grain)


@pytest.mark.gpu
def test_gops_coded_in_batches_side_by_side_and_in_rounds_are_the_references(tmp_path):
    import _e2e
    import xeve_amd

    xeve_amd.init(0)
    w, h, gops, frames, seed, cli, threads = _enc.BATCH_CASES["gops_128x64_noise"]
    gold = _enc.golden()["batches"]["gops_128x64_noise"]["per_gop"]
    p = str(tmp_path / "in.yuv")
    _e2e.make_yuv(p, w, h, gops * frames, seed)
    data, fb = open(p, "rb").read(), w * h * 3 // 2 * frames
    c0 = _enc.config(w, h, cli, threads)
    cfg = encode.config(w, h, qp=c0.qp, keyint=c0.keyint, bframes=c0.bframes, closed_gop=c0.closed_gop, preset=c0.preset, threads=c0.threads, ref=c0.ref)
    N = 10  # GOP i = the case's GOP i % 3
    fed = []

    def feed(enc, first, n):
        fed.append((first, n))
        for g in range(n):
            enc.push_gop(g, data[((first + g) % gops) * fb:((first + g) % gops + 1) * fb])

    # four GOPs per batch, two batches at a time: a round of 4 + 4, then one of 2
    out = encode.encode_gops(cfg, N, frames, feed, max_batches=2, batch_gops=4)
    assert fed == [(0, 4), (4, 4), (8, 2)]
    assert [(len(o), _enc.md5(o)) for o in out] == [(gold[i % gops]["bytes"], gold[i % gops]["md5"]) for i in range(N)]


def _stack_boundaries(w, h, gops):
    """GOP indices at which the stacks of a one-chain batch cross 2^31 and 2^32 samples: the stacked originals (vh rows of w samples per GOP) and the padded picture
    stores (vh rows of w + 2 * 144 samples per GOP)"""
    vh = (h + 2 * 144 + 63) & ~63
    out = []
    for what, per_gop in (("originals", vh * w), ("picture stores", vh * (w + 2 * 144))):
        for e in (31, 32):
            if (2 ** e) // per_gop < gops:
                out.append(("2^%d samples of stacked %s" % (e, what), (2 ** e) // per_gop))
    return vh, out


# (measured on one MI355X: 7.6 s and 98.1 GB of device memory for the 11 264 GOPs; 4.7 s and 49.1 GB for 5 632, which cross 2^31 only -- the whole case is in the default suite)
@pytest.mark.gpu
def test_a_batch_whose_stack_crosses_2e31_and_2e32_samples_is_the_references(tmp_path):
    """one batch of 1024x64 closed GOPs of two frames on one row chain, GOP i = clip i % 5 (tests/_enc.py WIDE_STACK_CASES): every bitstream is the reference application's
    for its clip -- also those whose pictures lie beyond 2^31 and 2^32 samples of the stack, where the 32-bit job records and every offset a kernel forms are at their
    limits.  The walk is the library's own choice at this width."""
    import _e2e
    import xeve_amd

    xeve_amd.init(0)
    gops = _enc.WIDE_STACK_GOPS
    (name, (w, h, clips, frames, seed, cli, threads)), = _enc.WIDE_STACK_CASES.items()
    gold = _enc.golden()["batches"][name]["per_gop"]
    vh, bounds = _stack_boundaries(w, h, gops)
    assert vh == 384 and [g for _, g in bounds] == [5461, 10922, 4262, 8525]
    assert all((2 ** e) % (vh * w * 5 * k) for e in (31, 32) for k in (1, 2)) and gops % 5  # (no multiple of five GOPs ends on a boundary: the wrap-around target of GOP i is another clip)
    p = str(tmp_path / "in.yuv")
    _e2e.make_yuv(p, w, h, clips * frames, seed)
    data, fb = open(p, "rb").read(), w * h * 3 // 2 * frames
    c0 = _enc.config(w, h, cli, threads)
    cfg = encode.config(w, h, qp=c0.qp, keyint=c0.keyint, bframes=c0.bframes, closed_gop=c0.closed_gop, preset=c0.preset, threads=c0.threads, ref=c0.ref)
    need, most = encode.footprint(cfg, gops, frames)
    assert most == (2 ** 33 - 1) // (vh * w) == 21845 and gops <= most
    print("wide stack: %d GOPs, footprint %.1f GB" % (gops, need / 1e9))
    enc = encode.BatchEncoder(cfg, gops, frames)
    try:
        for g in range(gops):
            enc.push_gop(g, data[(g % clips) * fb:(g % clips + 1) * fb])
        out = enc.encode()
    finally:
        enc.close()
    want = [(gold[i]["bytes"], gold[i]["md5"]) for i in range(clips)]
    memo = {}  # (five streams, thousands of copies of each: hash a byte string once)
    bad = [g for g in range(gops) if memo.setdefault(out[g], (len(out[g]), _enc.md5(out[g]))) != want[g % clips]]
    if bad:
        near = lambda g: min(bounds, key=lambda b: abs(b[1] - g))
        pytest.fail("%d of %d GOPs differ from the reference; the first is GOP %d (nearest boundary: %s, in GOP %d), the last is GOP %d (nearest boundary: %s, in GOP %d); all boundaries: %s"
                    % (len(bad), gops, bad[0], *near(bad[0]), bad[-1], *near(bad[-1]), bounds))
