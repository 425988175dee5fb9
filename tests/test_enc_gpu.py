"""The closed-GOP batch encoder on the GPU (xeve_hip_enc_*, xeve_amd/encode.py): every GOP's bitstream must be byte-identical to the reference application's run
over that GOP's frames.  Goldens: tests/golden/enc_v1.json (make_enc_golden.py) and e2e_v1.json (make_e2e_golden.py), recorded from the unmodified reference; no oracle
in between, and nothing of /root/reference is read here."""
import json
import os

import pytest

import _e2e
import _enc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import xeve_amd
    from xeve_amd import encode

    xeve_amd.init(0)
    return encode


@pytest.fixture(scope="module")
def yuv_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("enc_gpu_yuv")


def _frames(yuv_dir, name, w, h, n, seed):
    p = os.path.join(yuv_dir, name + ".yuv")
    if not os.path.exists(p):
        _e2e.make_yuv(p, w, h, n, seed)
    return open(p, "rb").read()


def _cfg(encode, w, h, cli, threads=1, **kw):
    c = _enc.config(w, h, cli, threads)
    return encode.config(w, h, qp=c.qp, keyint=c.keyint, bframes=c.bframes, closed_gop=c.closed_gop, preset=c.preset, threads=c.threads, ref=c.ref, **kw)


def _run(encode, cfg, gops_data, frames):
    enc = encode.BatchEncoder(cfg, len(gops_data), frames)
    for g, d in enumerate(gops_data):
        enc.push_gop(g, d)
    out = enc.encode()
    st = enc.stats()
    enc.close()
    return out, st


E2E = json.load(open(os.path.join(_enc.ROOT, "tests", "golden", "e2e_v1.json")))
SINGLE = ["tiny_ldb_fast", "tiny_ra_medium", "tiny_closed_gop", "tiny_ldb_fast_2threads", "moving_ra_medium", "moving_ldb_ref3", "moving_ra_b3_medium", "jumpy_ldb_fast",
          "noise_allintra_medium", "moving_cif_ra_medium"]


@pytest.mark.parametrize("name", SINGLE)
def test_single_runs_on_the_gpu_reproduce_the_reference_bitstreams(name, hip, yuv_dir):
    """one encoder run per clip (a batch of one): all-intra, low-delay B incl. several reference pictures, random access with 1 and 3 B pictures, closed GOP, two row
    chains (second writer pass), CIF with partial CTUs"""
    w, h, n, seed, cli = _e2e.CASES[name]
    out, _ = _run(hip, _cfg(hip, w, h, cli), [_frames(yuv_dir, name, w, h, n, seed)], n)
    assert (len(out[0]), _enc.md5(out[0])) == (E2E[name]["bytes"], E2E[name]["md5"])


@pytest.mark.parametrize("name", sorted(_enc.BATCH_CASES))
def test_batches_of_closed_gops_on_the_gpu(name, hip, yuv_dir):
    """G closed GOPs in lockstep -- I, P-like and B pictures of different GOPs decided by the same launches (the stacked-picture form of the inter analysis) -- with
    1 .. 8 row chains per picture: every GOP = the reference application's run over its frames (4 GOPs x 8 frames at 352x288 among them)"""
    w, h, gops, frames, seed, cli, threads = _enc.BATCH_CASES[name]
    g = _enc.golden()["batches"][name]
    data, fb = _frames(yuv_dir, name, w, h, gops * frames, seed), w * h * 3 // 2 * frames
    outs, st = _run(hip, _cfg(hip, w, h, cli, threads), [data[i * fb:(i + 1) * fb] for i in range(gops)], frames)
    print(name, st)
    assert [(len(o), _enc.md5(o)) for o in outs] == [(p["bytes"], p["md5"]) for p in g["per_gop"]]


@pytest.mark.parametrize("name", sorted(_enc.DEPTH10_CASES))
def test_ten_bit_input_on_the_gpu(name, hip, yuv_dir):
    """the application's -d 10 (16-bit little-endian samples, twice the bytes per frame): every GOP = the reference's run over it"""
    w, h, gops, frames, seed, cli, threads = _enc.DEPTH10_CASES[name]
    g = _enc.golden()["batches"][name]
    data, fb = _enc.widen10(_frames(yuv_dir, name, w, h, gops * frames, seed)), w * h * 3 * frames
    outs, _ = _run(hip, _cfg(hip, w, h, cli, threads, input_depth=10), [data[i * fb:(i + 1) * fb] for i in range(gops)], frames)
    assert [(len(o), _enc.md5(o)) for o in outs] == [(p["bytes"], p["md5"]) for p in g["per_gop"]]


@pytest.mark.parametrize("name", sorted(_enc.HEADER_OPTION_CASES))
def test_header_only_options_on_the_gpu(name, hip, yuv_dir):
    """--info 0 and --level-idc through the library's configuration record (reserved[0] bit 1 and bits 8-15)"""
    w, h, gops, frames, seed, cli, threads = _enc.HEADER_OPTION_CASES[name]
    g = _enc.golden()["batches"][name]
    c = _enc.config(w, h, cli, threads)
    data, fb = _frames(yuv_dir, name, w, h, gops * frames, seed), w * h * 3 // 2 * frames
    cfg = hip.config(w, h, qp=c.qp, keyint=c.keyint, bframes=c.bframes, closed_gop=c.closed_gop, preset=c.preset, threads=c.threads, ref=c.ref,
                     sei_info=not (c.reserved[0] & 2), level_idc=((c.reserved[0] >> 8) & 0xFF) or 40)
    assert cfg.reserved[0] == c.reserved[0]
    outs, _ = _run(hip, cfg, [data[i * fb:(i + 1) * fb] for i in range(gops)], frames)
    assert [(len(o), _enc.md5(o)) for o in outs] == [(p["bytes"], p["md5"]) for p in g["per_gop"]]


@pytest.mark.parametrize("walk", [0, 1], ids=["composed", "fused"])
@pytest.mark.parametrize("name", sorted(_enc.HOST_PINNED_CASES))
def test_p_slices_and_chroma_qp_offsets_on_the_gpu(name, walk, hip, yuv_dir):
    """--inter-slice-type 1 (P pictures: low delay with one and three reference pictures, the hierarchical closed GOP) and --qp-cb-offset / --qp-cr-offset (chroma QPs,
    lambdas and distortion weights of their own; the offsets in the slice header): options the reference APPLICATION cannot parse, so the goldens come from the reference
    LIBRARY with the parameters set on the way into xeve_create (oracle/ref_param_pin.c).  Both walks."""
    w, h, gops, frames, seed, cli, threads = _enc.HOST_PINNED_CASES[name]
    g = _enc.golden()["batches"][name]
    c = _enc.config(w, h, cli, threads)
    data, fb = _frames(yuv_dir, name, w, h, gops * frames, seed), w * h * 3 // 2 * frames
    cfg = hip.config(w, h, qp=c.qp, keyint=c.keyint, bframes=c.bframes, closed_gop=c.closed_gop, preset=c.preset, threads=c.threads, ref=c.ref,
                     inter_slice_type=c.inter_slice_type, qp_cb_offset=c.reserved[2], qp_cr_offset=c.reserved[3])
    assert cfg.inter_slice_type or cfg.reserved[2] or cfg.reserved[3]
    with hip.walk_select(walk):
        outs, _ = _run(hip, cfg, [data[i * fb:(i + 1) * fb] for i in range(gops)], frames)
    assert [(len(o), _enc.md5(o)) for o in outs] == [(p["bytes"], p["md5"]) for p in g["per_gop"]]


WALK_NAME = {-1: "by_width", 0: "composed", 1: "fused"}  # xeve_hip_walk_select


def _qp_range_params():
    """fast and medium presets on the composed walk AND the fused kernel, slow and placebo on the fused kernel (the only walk that codes them)"""
    out = []
    for n in sorted(_enc.QP_RANGE_CASES):
        fused_only = _enc.QP_RANGE_CASES[n][5][1] in ("slow", "placebo")
        out += [pytest.param(n, w, id="%s-%s" % (n, WALK_NAME[w])) for w in ((1,) if fused_only else (0, 1))]
    return out


@pytest.mark.parametrize("name,walk", _qp_range_params())
def test_the_ends_of_the_qp_range_on_the_gpu(name, walk, hip, yuv_dir):
    """-q 0 .. 2 and 47 .. 51 through the device path -- the walk's quantiser and bit counts at levels in the thousands, the writers with unary level strings thousands of
    bins long, slice buffers several times the raw picture (sized by the run's lowest slice QP), the QP-1 clamp of a slice of QP 0, the hierarchy's offsets clipped at 51,
    the chroma tables at both ends, 10-bit input, flat 0 / flat 255 frames: every GOP = the unmodified reference's bytes (tests/golden/enc_v1.json), no harness between"""
    w, h, gops, frames, seed, cli, threads = _enc.QP_RANGE_CASES[name]
    g = _enc.golden()["batches"][name]
    c = _enc.config(w, h, cli, threads)
    cfg = hip.config(w, h, qp=c.qp, keyint=c.keyint, bframes=c.bframes, closed_gop=c.closed_gop, preset=c.preset, threads=c.threads, ref=c.ref, inter_slice_type=c.inter_slice_type,
                     qp_cb_offset=c.reserved[2], qp_cr_offset=c.reserved[3], input_depth=c.reserved[1] or 8)
    with hip.walk_select(walk):
        outs, _ = _run(hip, cfg, _enc.qp_range_input(yuv_dir, name), frames)
    assert [(len(o), _enc.md5(o)) for o in outs] == [(p["bytes"], p["md5"]) for p in g["per_gop"]]


def _saturated_params():
    """as _qp_range_params; the cases outside _enc.SATURATED_GPU_DEFAULT carry gpu_full"""
    out = []
    for n in sorted(_enc.SATURATED_CASES):
        fused_only = _enc.SATURATED_CASES[n][5][1] in ("slow", "placebo")
        for w in ((1,) if fused_only else (0, 1)):
            full = n not in _enc.SATURATED_GPU_DEFAULT or (n, w) == ("sat_noise_q0_ldb", 1)  # (4.7 s: the first case to leave the default suite for its 900 s)
            out.append(pytest.param(n, w, id="%s-%s" % (n, WALK_NAME[w]), marks=(pytest.mark.gpu_full,) if full else ()))
    return out


def _saturated_run(hip, cases, name, walk, yuv_dir):
    w, h, gops, frames, seed, cli, threads = cases[name]
    c = _enc.config(w, h, cli, threads)
    cfg = hip.config(w, h, qp=c.qp, keyint=c.keyint, bframes=c.bframes, closed_gop=c.closed_gop, preset=c.preset, threads=c.threads, ref=c.ref, input_depth=c.reserved[1] or 8)
    with hip.walk_select(walk):
        outs, st = _run(hip, cfg, _enc.qp_range_input(yuv_dir, name, cases), frames)
    return outs, st


@pytest.mark.parametrize("name,walk", _saturated_params())
def test_saturated_content_on_the_gpu(name, walk, hip, yuv_dir):
    """pictures whose every sample is 0 or 255 (tests/_e2e.py: binary noise, drifting 32x32 cells, the flipping one-sample checkerboard, the scene cut) at QPs down to 0
    through the device path: full-scale flat residuals on 32- and 64-point blocks where the reference's (s16) levels wrap, the matrix-core transforms at full scale, the
    walk's quantiser / RDOQ and its packed run / level entries, unary level strings tens of thousands of bins long, the reconstruction's clip under ringing, slice data
    1.25 .. 2.2 times that of uniform noise (enc_plan.h slice_capacity): every GOP = the unmodified reference's bytes (tests/golden/enc_v1.json), no harness between"""
    outs, _ = _saturated_run(hip, _enc.SATURATED_CASES, name, walk, yuv_dir)
    assert [(len(o), _enc.md5(o)) for o in outs] == [(p["bytes"], p["md5"]) for p in _enc.golden()["batches"][name]["per_gop"]]


SIZE_FUSED = ("size_8x8_noise", "size_24x40_moving", "size_104x112_noise", "size_176x144_noise_m2")  # the fused walk's device build at four of the shapes its host side is held at


def _picture_size_params():
    """fast and medium presets: every shape on the composed walk (no host twin), four on the fused kernel; slow and placebo on the fused kernel (the only walk that codes them)"""
    out = []
    for n in _enc.PICTURE_SIZE_CASES:
        fused_only = _enc.PICTURE_SIZE_CASES[n][5][1] in ("slow", "placebo")
        out += [pytest.param(n, w, id="%s-%s" % (n, WALK_NAME[w])) for w in ((1,) if fused_only else (0, 1) if n in SIZE_FUSED else (0,))]
    return out


@pytest.mark.parametrize("name,walk", _picture_size_params())
def test_picture_sizes_modulo_the_ctu_on_the_gpu(name, walk, hip, yuv_dir):
    """pictures smaller than one CTU in one or both directions (8x8, one CU row of one and of four CTUs, one CU column) and partial last CTU columns and rows of every
    remainder 8 .. 56 through the device path -- frame loading and padding deeper than the picture, the walks' tile loops and neighbour windows, search windows clipped to a
    picture smaller than the range and than the block, the loop filter, the writers with one CTU column or row: every GOP = the unmodified reference's bytes
    (tests/golden/enc_v1.json), no harness between"""
    w, h, gops, frames, seed, cli, threads = _enc.PICTURE_SIZE_CASES[name]
    g = _enc.golden()["batches"][name]
    data, fb = _frames(yuv_dir, name, w, h, gops * frames, seed), w * h * 3 // 2 * frames
    with hip.walk_select(walk):
        outs, _ = _run(hip, _cfg(hip, w, h, cli, threads), [data[i * fb:(i + 1) * fb] for i in range(gops)], frames)
    assert [(len(o), _enc.md5(o)) for o in outs] == [(p["bytes"], p["md5"]) for p in g["per_gop"]]


def _largest_size_params():
    """both walks (slow and placebo: the fused kernel, the only walk that codes them), all gpu_full: the default suite has no room for a 128-step strip
    (tests/test_gpu_suite_budget.py); it keeps the leaf tests of the zone (tests/test_hip_me.py, tests/test_hip_inter.py)"""
    out = []
    for n in _enc.LARGEST_SIZE_CASES:
        fused_only = _enc.LARGEST_SIZE_CASES[n][5][1] in ("slow", "placebo")
        for w in ((1,) if fused_only else (0, 1)):
            out.append(pytest.param(n, w, id="%s-%s" % (n, WALK_NAME[w]), marks=(pytest.mark.gpu_full,)))
    return out


@pytest.mark.parametrize("name,walk", _largest_size_params())
def test_the_widest_and_tallest_accepted_pictures_on_the_gpu(name, walk, hip, yuv_dir):
    """strips of the largest accepted pictures (tests/_enc.py LARGEST_SIZE_CASES) through the device path: 8192 samples wide, where predictors and start vectors that point
    right wrap in the last CTU column as the reference's s16 frame coordinates do and the searches run at the picture's left end (tests/test_enc_host.py counts on the CPU
    that these clips get there; the 8128-wide control cannot), and 4320 rows high on one and on eight row chains: every GOP = the unmodified reference's bytes
    (tests/golden/enc_v1.json), no harness between"""
    w, h, gops, frames, seed, cli, threads = _enc.LARGEST_SIZE_CASES[name]
    g = _enc.golden()["batches"][name]
    with hip.walk_select(walk):
        outs, _ = _run(hip, _cfg(hip, w, h, cli, threads), [_frames(yuv_dir, name, w, h, gops * frames, seed)], frames)
    assert [(len(o), _enc.md5(o)) for o in outs] == [(p["bytes"], p["md5"]) for p in g["per_gop"]]


@pytest.mark.parametrize("name", sorted(_e2e.SLOW_CASES))
def test_preset_slow_single_runs_on_the_gpu(name, hip, yuv_dir):
    """--preset slow on the device (the fused walk: walk_dbk.h estimates the loop filter's share of every candidate's distortion -- rdo_dbk_switch = 1 --, the search
    runs its quarter-pel stage, ME range 128): low delay, hierarchical B pictures, closed GOPs with partial CTUs, all-intra, two row chains = the reference's bitstreams"""
    w, h, n, seed, cli = _e2e.SLOW_CASES[name]
    threads = int(cli[cli.index("-m") + 1]) if "-m" in cli else 1
    cli = [a for i, a in enumerate(cli) if a != "-m" and (i == 0 or cli[i - 1] != "-m")]
    out, _ = _run(hip, _cfg(hip, w, h, cli, threads), [_frames(yuv_dir, name, w, h, n, seed)], n)
    assert (len(out[0]), _enc.md5(out[0])) == (E2E[name]["bytes"], E2E[name]["md5"])


@pytest.mark.parametrize("team", [0, 3], ids=["one_chain_per_team", "three_chains_per_team"])
@pytest.mark.parametrize("name", sorted(_enc.SLOW_BATCH_CASES))
def test_preset_slow_batches_on_the_gpu(name, team, hip, yuv_dir):
    """... closed GOPs in lockstep with 3 / 8 row chains, teams of one and of three chains"""
    w, h, gops, frames, seed, cli, threads = _enc.SLOW_BATCH_CASES[name]
    g = _enc.golden()["batches"][name]
    data, fb = _frames(yuv_dir, name, w, h, gops * frames, seed), w * h * 3 // 2 * frames
    with hip.walk_select(-1, team):
        outs, _ = _run(hip, _cfg(hip, w, h, cli, threads), [data[i * fb:(i + 1) * fb] for i in range(gops)], frames)
    assert [(len(o), _enc.md5(o)) for o in outs] == [(p["bytes"], p["md5"]) for p in g["per_gop"]]


@pytest.mark.parametrize("name", sorted(n for n in _e2e.PLACEBO_CASES if n != "placebo_one_ctu_ldb"))  # (that one is the CPU race detector's clip)
def test_preset_placebo_single_runs_on_the_gpu(name, hip, yuv_dir):
    """--preset placebo on the device (the fused walk): inter CUs of 4x4 beside the intra analysis of every 4x4 node, 64x64 intra CUs in I slices, two reference pictures
    per list, the raster search, ME range 384, eight sub-pel positions per stage, four merge candidates, rdo_dbk_switch = the reference application's bitstreams"""
    w, h, n, seed, cli = _e2e.PLACEBO_CASES[name]
    threads = int(cli[cli.index("-m") + 1]) if "-m" in cli else 1
    cli = [a for i, a in enumerate(cli) if a != "-m" and (i == 0 or cli[i - 1] != "-m")]
    out, _ = _run(hip, _cfg(hip, w, h, cli, threads), [_frames(yuv_dir, name, w, h, n, seed)], n)
    assert (len(out[0]), _enc.md5(out[0])) == (E2E[name]["bytes"], E2E[name]["md5"])


@pytest.mark.parametrize("team", [0, 3], ids=["one_chain_per_team", "three_chains_per_team"])
@pytest.mark.parametrize("name", sorted(_enc.PLACEBO_BATCH_CASES))
def test_preset_placebo_batches_on_the_gpu(name, team, hip, yuv_dir):
    w, h, gops, frames, seed, cli, threads = _enc.PLACEBO_BATCH_CASES[name]
    g = _enc.golden()["batches"][name]
    data, fb = _frames(yuv_dir, name, w, h, gops * frames, seed), w * h * 3 // 2 * frames
    with hip.walk_select(-1, team):
        outs, _ = _run(hip, _cfg(hip, w, h, cli, threads), [data[i * fb:(i + 1) * fb] for i in range(gops)], frames)
    assert [(len(o), _enc.md5(o)) for o in outs] == [(p["bytes"], p["md5"]) for p in g["per_gop"]]


def test_a_run_consumes_its_frames_and_says_so(hip):
    """round 6: the picture stores of later pictures live in the memory of frames already coded (encode.hip dims(): a store over the frames' buffer as soon as it ends inside the
    frames coded so far).  1280x720 with 10-bit input (a frame is 2.8 MB, a padded store 4.8 MB): the second store of a two-picture GOP lies over both frames.  A second run
    of the same object without new frames is refused; with the frames pushed again it writes the same bytes.  (That the bytes are the reference's with stores placed so is what
    the cases at 1920x1080 and 3840x2160 hold: their goldens.)"""
    import xeve_amd

    w, h, frames = 1280, 720, 2
    cfg = hip.config(w, h, keyint=8, closed_gop=True, preset="medium", threads=8, input_depth=10)
    import numpy as np

    cfg8 = hip.config(w, h, keyint=8, closed_gop=True, preset="medium", threads=8)
    # (with 8-bit input a store is 3.5 frames and both stores are memory of their own: the 10-bit batch, whose frames are twice the size, is the SMALLER one)
    assert hip.footprint(cfg, 1, frames)[0] < hip.footprint(cfg8, 1, frames)[0], "the second store is not over the frames"
    clip = np.random.default_rng(9).integers(0, 1024, size=2 * frames * w * h * 3 // 2, dtype=np.uint16).tobytes()
    fb = w * h * 3 * frames  # bytes of a GOP: two bytes per sample
    enc = hip.BatchEncoder(cfg, 2, frames)
    for g in range(2):
        enc.push_gop(g, clip[g * fb:(g + 1) * fb])
    first = enc.encode()
    with pytest.raises(xeve_amd.XeveHipError, match="consumed its frames"):
        enc.encode()
    enc.push_gop(0, clip[:fb])
    with pytest.raises(xeve_amd.XeveHipError, match="consumed its frames"):  # (every frame, not some)
        enc.encode()
    enc.push_gop(0, clip[:fb]), enc.push_gop(1, clip[fb:])
    again = enc.encode()
    enc.close()
    assert again == first and len(first[0]) > 1000 and first[0] != first[1]


def test_preset_slow_is_refused_where_the_fused_walk_is_switched_off(hip):
    import xeve_amd

    with hip.walk_select(0):
        enc = hip.BatchEncoder(hip.config(128, 64, keyint=4, bframes=3, closed_gop=True, preset="slow"), 1, 2)
        for f in range(2):
            enc.push(0, f, bytes(128 * 64 * 3 // 2))
        with pytest.raises(xeve_amd.XeveHipError, match="fused walk"):
            enc.encode()
        enc.close()
        enc = hip.BatchEncoder(hip.config(128, 64, bframes=0, preset="placebo"), 1, 2)  # (its I picture is the composed walk's to code; the 4x4 inter CUs of the next are not)
        for f in range(2):
            enc.push(0, f, bytes(128 * 64 * 3 // 2))
        with pytest.raises(xeve_amd.XeveHipError, match="fused walk"):
            enc.encode()
        enc.close()
    with pytest.raises(xeve_amd.XeveHipError, match="chroma qp offsets"):
        hip.BatchEncoder(hip.config(128, 64, preset="slow", qp_cb_offset=1), 1, 1)


def test_one_chain_through_the_second_writer_pass_on_the_gpu(hip, yuv_dir):
    w, h, n, seed, cli = _e2e.CASES["tiny_closed_gop"]
    f = _frames(yuv_dir, "tiny_closed_gop", w, h, n, seed)
    out, _ = _run(hip, _cfg(hip, w, h, cli, always_second_pass=True), [f], n)
    assert _enc.md5(out[0]) == E2E["tiny_closed_gop"]["md5"]


def test_a_batch_is_the_same_as_its_gops_coded_alone(hip, yuv_dir):
    """the lockstep axis must not leak between GOPs: GOP 1 of a batch of three = the same GOP as a batch of one"""
    w, h, gops, frames, seed, cli, threads = _enc.BATCH_CASES["gops_128x64_noise"]
    data, fb = _frames(yuv_dir, "gops_128x64_noise", w, h, gops * frames, seed), w * h * 3 // 2 * frames
    alone, _ = _run(hip, _cfg(hip, w, h, cli, threads), [data[fb:2 * fb]], frames)
    assert _enc.md5(alone[0]) == _enc.golden()["batches"]["gops_128x64_noise"]["per_gop"][1]["md5"]


@pytest.mark.parametrize("shape", ["first_pass", "second_pass", "second_pass_two_chains"])
def test_a_picture_that_outgrows_its_slice_buffer_ends_the_run_with_an_error(shape, hip, yuv_dir, monkeypatch):
    """the engine's handling of an overflow (the writers' own bounds checks: tests/test_eco_lane.py, tests/test_hip_tree.py).  Binary noise at -q 12 with the writer kernels
    and the fetch TOLD a buffer of half the slice data of the golden's largest picture (XEVE_HIP_ENC_SLICE_TOLD, read at create; the allocation stays slice_capacity(),
    so a defective bounds check shows here as a failed assertion, not as a fault): the run ends with the error and no GOP has a byte of bitstream -- on one chain (the
    first-pass writer appends the slice data), through the second writer pass at 128x64 (one CTU row: one chain), and with two row chains at 128x128.  A fresh encoder of
    the same process is untouched.  The slice data is the slice NAL unit WITHOUT the cabac_zero_words the host appends: 12 279 of the I picture's 38 555 bytes here, so
    half of the NAL unit's size would still hold every picture."""
    import xeve_amd

    name = "sat_noise_q12_m2" if shape == "second_pass_two_chains" else "sat_noise_q12_closed"
    sizes = _enc.golden()["batches"][name]["per_gop"][0]["slice_data_bytes"]
    told = max(sizes) // 2
    w, h, gops, frames, seed, cli, threads = _enc.SATURATED_CASES[name]
    cfg = _cfg(hip, w, h, cli, threads, always_second_pass=shape == "second_pass")
    assert len(sizes) == frames and 0 < told < min(sizes) and max(sizes) < hip.slice_capacity(cfg, frames)  # (every picture outgrows it; none outgrows the allocation)
    monkeypatch.setenv("XEVE_HIP_ENC_SLICE_TOLD", str(hip.slice_capacity(cfg, frames) + 1))
    with pytest.raises(xeve_amd.XeveHipError, match="XEVE_HIP_ENC_SLICE_TOLD"):  # (above the allocation: refused)
        hip.BatchEncoder(cfg, 2, frames)
    monkeypatch.setenv("XEVE_HIP_ENC_SLICE_TOLD", str(told))
    data = _enc.qp_range_input(yuv_dir, name, _enc.SATURATED_CASES)[0]
    enc = hip.BatchEncoder(cfg, 2, frames)
    try:
        for g in range(2):
            enc.push_gop(g, data)
        with pytest.raises(xeve_amd.XeveHipError, match="outgrew"):
            enc.encode()
        assert enc.bitstream_sizes() == [0, 0]
    finally:
        enc.close()
    monkeypatch.delenv("XEVE_HIP_ENC_SLICE_TOLD")
    w, h, gops, frames, seed, cli, threads = _enc.BATCH_CASES["gops_128x64_noise"]
    gold = _enc.golden()["batches"]["gops_128x64_noise"]["per_gop"]
    data, fb = _frames(yuv_dir, "gops_128x64_noise", w, h, gops * frames, seed), w * h * 3 // 2 * frames
    outs, _ = _run(hip, _cfg(hip, w, h, cli, threads), [data[i * fb:(i + 1) * fb] for i in range(gops)], frames)
    assert [(len(o), _enc.md5(o)) for o in outs] == [(p["bytes"], p["md5"]) for p in gold]


def test_a_wide_batch_fed_from_device_memory_keeps_every_gop_exact(hip, yuv_dir):
    """288 GOPs in lockstep (96 copies of the three GOPs of the noise case), the frames pushed as device tensors that torch is still producing on its own stream when
    push is called: GOP i of the batch = the reference's bytes of GOP i % 3, at both ends of the batch and everywhere between"""
    import torch

    w, h, gops, frames, seed, cli, threads = _enc.BATCH_CASES["gops_128x64_noise"]
    gold = _enc.golden()["batches"]["gops_128x64_noise"]["per_gop"]
    data, fb = _frames(yuv_dir, "gops_128x64_noise", w, h, gops * frames, seed), w * h * 3 // 2 * frames
    src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    G = 96 * gops
    enc = hip.BatchEncoder(_cfg(hip, w, h, cli, threads), G, frames)
    for g in range(G):
        d = (src[(g % gops) * fb:(g % gops + 1) * fb].to(torch.int32) + 0).to(torch.uint8)  # (a fresh tensor from kernels queued on torch's stream)
        enc.push_gop(g, d)
    outs = enc.encode()
    enc.close()
    bad = [g for g in range(G) if (len(outs[g]), _enc.md5(outs[g])) != (gold[g % gops]["bytes"], gold[g % gops]["md5"])]
    assert not bad, bad[:10]


@pytest.mark.parametrize("side", [1, 0, 2], ids=["side_stream", "one_stream", "stream_per_level"])
def test_every_gop_of_a_wide_batch_of_one_clip_comes_out_equal(side, hip):
    """668 GOPs x 8 row chains of ONE noise clip (512x512: 64 CTUs, IDR + one B picture, 44 lockstep steps = 235 000 chain-steps) on the composed walk: whatever goes wrong in
    one chain of one step -- a race between the waves of a block, between the two streams -- shows as a second bitstream.  (Round 6: a barrier dropped from the tree
    operations made ~12 of 658 GOPs differ per 3840x2160 run, one chain-step in 250 000; every other test of the suite passed, the bench's seeded-GOP check caught it.)"""
    import torch

    w, h, G, F = 512, 512, 668, 2
    fb = w * h * 3 // 2
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4242)
    clip = torch.randint(0, 256, (fb * F,), dtype=torch.uint8, device="cuda", generator=gen)
    with hip.walk_select(0, 0, side):
        enc = hip.BatchEncoder(hip.config(w, h, qp=32, keyint=8, bframes=15, closed_gop=True, preset="medium", threads=8), G, F)
        for g in range(G):
            enc.push_gop(g, clip)
        outs = enc.encode()
        enc.close()
    first = _enc.md5(outs[0])
    bad = [g for g in range(G) if _enc.md5(outs[g]) != first]
    assert not bad and len(outs[0]) > 100000, (len(bad), bad[:10])


@pytest.mark.gpu_last
@pytest.mark.gpu_full
@pytest.mark.parametrize("name", sorted(_enc.PRESET_REAL_CASES))
def test_presets_slow_and_placebo_at_1920x1080_on_the_gpu(name, hip, yuv_dir):
    """--preset slow (noise) and --preset placebo (drifting texture) at 1920x1080 with 8 row chains: 510 CTUs per picture through the fused walk's loop-filter estimate, its
    quarter-pel and raster searches and its 4x4 inter CUs = the reference application's bitstreams.  XEVE_GPU_FULL=1 (profiles/r05i_*.log): a repeat at a larger size"""
    w, h, gops, frames, seed, cli, threads = _enc.PRESET_REAL_CASES[name]
    g = _enc.golden()["batches"][name]
    data, fb = _frames(yuv_dir, name, w, h, gops * frames, seed), w * h * 3 // 2 * frames
    outs, st = _run(hip, _cfg(hip, w, h, cli, threads), [data[i * fb:(i + 1) * fb] for i in range(gops)], frames)
    print(name, st)
    assert [(len(o), _enc.md5(o)) for o in outs] == [(p["bytes"], p["md5"]) for p in g["per_gop"]]


@pytest.mark.gpu_last
@pytest.mark.gpu_full
@pytest.mark.parametrize("name", sorted(_enc.SATURATED_REAL_CASES))
def test_saturated_content_at_1920x1080_on_the_gpu(name, hip, yuv_dir):
    """binary noise at -q 24 (0.94 bytes per sample: above what the slice buffers held before they were sized for it) and the 32x32 cells at -q 1 (the wrap zone of the
    64- and 32-point blocks), two low-delay pictures at 1920x1080 with 8 row chains, on the library's own choice of walk = the reference application's bitstreams"""
    outs, st = _saturated_run(hip, _enc.SATURATED_REAL_CASES, name, -1, yuv_dir)
    print(name, st)
    assert [(len(o), _enc.md5(o)) for o in outs] == [(p["bytes"], p["md5"]) for p in _enc.golden()["batches"][name]["per_gop"]]


# BASELINE's configs at their real picture sizes (gpu_last: after every other GPU test).  The default suite has to fit the driver's 1200 s on one MI355X (tests/conftest.py),
# so it runs the forms that add something -- config 3 over a whole 16-picture sub-GOP on the library's own choice of walk, config 2 on the COMPOSED walk (the bench's path
# at width), the whole 8-frame 1080p GOP and (round 6) the whole 8-frame 3840x2160 GOP of config 4 on the composed walk -- and leaves the forms those contain (9 frames of
# config 3, 2 frames / IDR + two B pictures of config 4) and the repeats (17 frames of config 2, the moving 1080p GOPs, the 4K GOP on the fused kernel) to XEVE_GPU_FULL=1.
REAL_DEFAULT = {"cfg3_1080p_ra_medium_17f_m8": -1, "cfg2_720p_ldb_fast_8f_m8": 0}  # name -> walk (xeve_hip_walk_select)
REAL_FULL = {"cfg2_720p_ldb_fast_17f_m8": -1, "cfg2_720p_ldb_fast_64f_m8": 0, "gops_1080p_moving_m8": 0, "cfg3_1080p_ra_medium_9f_m8": 0, "cfg4_2160p_closedgop_medium_2f_m8": -1}
assert set(REAL_DEFAULT) | set(REAL_FULL) == set(_enc.BATCH_CASES_REAL)


@pytest.mark.gpu_last
@pytest.mark.parametrize("name,walk", [pytest.param(n, w, id="%s-%s" % (n, WALK_NAME[w])) for n, w in sorted(REAL_DEFAULT.items())] +
                         [pytest.param(n, w, id="%s-%s" % (n, WALK_NAME[w]), marks=pytest.mark.gpu_full) for n, w in sorted(REAL_FULL.items())])
def test_batches_at_real_picture_sizes_on_the_gpu(name, walk, hip, yuv_dir):
    """BASELINE's configs 2 and 3 as runs of 8 / 17 frames at 1280x720 / 1920x1080 (8 row chains per picture, the second writer pass over 510
    CTUs per picture, four B layers with reference distances 16 / 8 / 4 / 2 / 1) = the reference application's bitstreams"""
    w, h, gops, frames, seed, cli, threads = _enc.BATCH_CASES_REAL[name]
    g = _enc.golden()["batches"][name]
    data, fb = _frames(yuv_dir, name, w, h, gops * frames, seed), w * h * 3 // 2 * frames
    with hip.walk_select(walk):
        outs, st = _run(hip, _cfg(hip, w, h, cli, threads), [data[i * fb:(i + 1) * fb] for i in range(gops)], frames)
    print(name, WALK_NAME[walk], st)
    assert [(len(o), _enc.md5(o)) for o in outs] == [(p["bytes"], p["md5"]) for p in g["per_gop"]]


FULL_GOPS = json.load(open(os.path.join(_enc.ROOT, "tests", "golden", "cfg4_8f_v1.json")))  # make_cfg4_8f_golden.py: the unmodified reference on the bench's own clips
C3, C4 = "cfg3_1080p_closedgop_medium_8f_m8", "cfg4_2160p_closedgop_medium_8f_m8"
assert {C3, C4} <= set(FULL_GOPS), sorted(FULL_GOPS)  # (the file also holds the clips at presets slow and placebo: bench.py --preset)


@pytest.mark.gpu_last
@pytest.mark.parametrize("name,walk,pictures", [
    # (round 6, VERDICT r05 next 4: the WHOLE 3840x2160 GOP, 8 of 8 pictures, in the default suite -- the composed walk with its side stream takes a lockstep step of
    # 16 chains in ~60 ms, 2416 steps in ~150 s; rounds 4-5 ran IDR + two B pictures here and left the whole GOP to XEVE_GPU_FULL and to bench.py --pictures 0)
    pytest.param(C4, 0, 8, id="2160p-composed-whole_gop"),
    # (the whole 1920x1080 GOP: 46-58 s; the default suite keeps 1920x1080 as config 3's 17-frame run and as test_e2e_real_sizes.py, and the whole GOP at 3840x2160)
    pytest.param(C3, 0, 8, id="1080p-composed-whole_gop", marks=pytest.mark.gpu_full),
    pytest.param(C4, 0, 3, id="2160p-composed-idr_and_two_b", marks=pytest.mark.gpu_full),
    # (the fused kernel at 1920x1080 is the 17-frame run of config 3 above: 1768 steps of four B layers; the same kernel over this GOP: 78 s more for the default suite)
    pytest.param(C3, 1, 8, id="1080p-fused-whole_gop", marks=pytest.mark.gpu_full), pytest.param(C4, 1, 3, id="2160p-fused-idr_and_two_b", marks=pytest.mark.gpu_full), pytest.param(C4, 1, 8, id="2160p-fused-whole_gop", marks=pytest.mark.gpu_full)])
def test_full_eight_frame_closed_gops_at_the_baseline_sizes(name, walk, pictures, hip):
    """BASELINE config 4 (3840x2160) and 1920x1080 as FULL `-I 8` closed GOPs (1 IDR + 7 hierarchical B pictures, -m 8) -- the clip
    bench.py seeds its batches with -- on the composed walk (what the bench runs at width) AND the fused kernel.  GOP 1 of the batch is the same clip with its frames in
    reverse order (another GOP beside it in lockstep); GOP 0 must be the reference's file byte for byte: after `pictures` pictures (xeve_hip_enc_flush) the golden's prefix
    after the same picture, and with the whole GOP run, the file.  3840x2160 in the default suite = the IDR picture and two B pictures (POC 4 from the IDR picture alone,
    POC 2 from two different reference pictures) is the gpu_full form; the default suite runs the whole 4K GOP, 8 of 8 pictures (round 6)"""
    import numpy as np

    from bench import check_prefix, reference_noise

    r = FULL_GOPS[name]
    w, h, frames = r["w"], r["h"], r["frames"]
    fb = w * h * 3 // 2
    clip = reference_noise(fb * frames, r["seed"])
    back = np.ascontiguousarray(clip.reshape(frames, fb)[::-1]).reshape(-1)
    with hip.walk_select(walk):
        enc = hip.BatchEncoder(hip.config(w, h, qp=32, keyint=8, bframes=15, closed_gop=True, preset="medium", threads=8), 2, frames)
        for g, d in enumerate((clip.tobytes(), back.tobytes())):
            enc.push_gop(g, d)
        enc.begin()
        per_picture = enc.advance(0) // frames
        left = enc.advance(pictures * per_picture)
        enc.sync()
        enc.flush()
        outs, st = enc.bitstreams(), enc.stats()
        enc.close()
    print(name, WALK_NAME[walk], pictures, st)
    assert check_prefix(outs[0], r) == pictures
    assert outs[1] != outs[0] and len(outs[1]) > len(outs[0]) // 2
    if pictures == frames:
        assert left == 0 and (len(outs[0]), _enc.md5(outs[0])) == (r["bytes"], r["md5"])


def test_configurations_outside_the_supported_set_are_refused_by_the_library(hip):
    """the refusals of tests/_enc.py CONFIG_ACCEPTANCE through xeve_hip_enc_create (the same table is held on the CPU through xeve_hip_enc_footprint, tests/test_enc_host.py)"""
    import xeve_amd

    refused = [dict(kw) for kw, ok in _enc.CONFIG_ACCEPTANCE if not ok]
    assert len(refused) >= 10
    for kw in refused:
        kw.setdefault("keyint", 8), kw.setdefault("closed_gop", True)
        c = hip.config(kw.pop("w"), kw.pop("h"), **kw)
        with pytest.raises(xeve_amd.XeveHipError):
            hip.BatchEncoder(c, 1, 1)
