"""GPU suite: xeve_hip_me_ipel_diamond_jobs (one complete me_ipel_diamond per wave) against the reference goldens and
against the oracle on batches of seeded jobs; the same for the sub-pel pattern and the whole pinter_me_epzs.  Beside noise and texture: content where candidates tie
and search windows clip (_me_cases: flat, periodic, outward, static) -- the first candidate in evaluation order must win among equal costs, which the lane-parallel
search gets from a wave minimum, a ballot and the first set bit, and from `<` across the passes of a candidate list longer than a wave."""
import ctypes as C

import numpy as np
import pytest

from _me_cases import PAD, make_planes, run_oracle
from _me_golden import golden_cases

pytestmark = pytest.mark.gpu


_planes_on_device = []  # [(numpy plane, tensor)]: the last few planes sent, so that the rows of a fixture that share a plane pair do not send it once per launch


def plane_on_device(a, dev):
    import torch

    for k, t in _planes_on_device:
        if k is a:
            return t
    _planes_on_device.append((a, torch.from_numpy(a).to(dev)))
    del _planes_on_device[:-4]
    return _planes_on_device[-1][1]


def gpu_run(cases, bit_depth=10):
    """all cases share planes, block size and every launch-level parameter"""
    import torch

    import xeve_amd
    from xeve_amd import device as D
    from xeve_amd import lib

    xeve_amd.init(0)
    dev = torch.device("cuda:0")
    c0 = cases[0]
    S = c0["S"]
    jobs = np.zeros(len(cases), dtype=lib.ME_JOB_DTYPE)
    bi_buf = np.zeros((len(cases), S * S), np.int16)
    for i, c in enumerate(cases):
        jobs[i] = (c["x"], c["y"], i * S * S, c["range"], c["gmvp"], c["mvi"], c["beststep_in"])
        bi_buf[i] = c["org_bi"]
    P = lib.MeParams(c0["lambda_mv"], 1, c0["mot_other"], c0["bi"], c0["faststep"], c0["msr"], c0["sr"], (C.c_int32 * 2)(*c0["min_clip"]),
                     (C.c_int32 * 2)(*c0["max_clip"]), 0)
    org, ref = plane_on_device(c0["org"], dev), plane_on_device(c0["ref"], dev)
    o0 = PAD * c0["s"] + PAD
    return D.me_ipel_diamond_jobs(org, o0, c0["s"], torch.from_numpy(bi_buf).to(dev), ref, o0, c0["s"], jobs, S.bit_length() - 1, bit_depth, P)


def test_me_matches_reference_goldens():
    n = 0
    for c, (cost, mvx, mvy, beststep) in golden_cases():
        res = gpu_run([c])[0]
        assert (int(res["cost"]), int(res["mv"][0]), int(res["mv"][1]), int(res["beststep"])) == (cost, mvx, mvy, beststep), (n, c["S"], c["bi"])
        n += 1
    assert n == 96


@pytest.mark.parametrize("S", [8, 16, 32, 64])
@pytest.mark.parametrize("bi", [0, 1, 2])
@pytest.mark.parametrize("textured", [False, True])
def test_me_batches_vs_oracle(S, bi, textured):
    from _me_cases import BATCH_STEPS, batch_launches

    steps = set()
    for cases in batch_launches(S, bi, textured):
        got = gpu_run(cases)
        for i, c in enumerate(cases):
            e = run_oracle(c)
            g = got[i]
            assert (int(g["cost"]), int(g["mv"][0]), int(g["mv"][1]), int(g["beststep"]), int(g["best_mv_bits"])) == \
                   (e.cost, e.mv[0], e.mv[1], e.beststep, e.best_mv_bits), (S, bi, textured, i)
            steps.add(e.beststep)
    # the searches end in the dense round and at several ring sizes: as many distinct values as the oracle gives on the CPU (tests/test_me_degenerate.py)
    assert len(steps) >= BATCH_STEPS[(S, bi, textured)] and (bi == 1 or len(steps) >= 3), sorted(steps)


def gpu_run_spel(cases, bit_depth=10):
    import torch

    import xeve_amd
    from xeve_amd import device as D
    from xeve_amd import lib

    xeve_amd.init(0)
    dev = torch.device("cuda:0")
    c0 = cases[0]
    S = c0["S"]
    jobs = np.zeros(len(cases), dtype=lib.SPEL_JOB_DTYPE)
    bi_buf = np.zeros((len(cases), S * S), np.int16)
    for i, c in enumerate(cases):
        jobs[i] = (c["x"], c["y"], i * S * S, c["gmvp"], c["mvi"])
        bi_buf[i] = c["org_bi"]
    P = lib.SpelParams(c0["lambda_mv"], 1, c0["mot_other"], c0["bi"], c0["hpel_cnt"], c0["qpel_cnt"])
    org, ref = plane_on_device(c0["org"], dev), plane_on_device(c0["ref"], dev)
    o0 = PAD * c0["s"] + PAD
    return D.me_spel_pattern_jobs(org, o0, c0["s"], torch.from_numpy(bi_buf).to(dev), ref, o0, c0["s"], jobs, S.bit_length() - 1, bit_depth, P)


def test_spel_matches_reference_goldens():
    from _me_golden import golden_spel_cases

    n = 0
    for c, (cost, mvx, mvy) in golden_spel_cases():
        res = gpu_run_spel([c])[0]
        assert (int(res["cost"]), int(res["mv"][0]), int(res["mv"][1])) == (cost, mvx, mvy), (n, c["S"], c["bi"])
        n += 1
    assert n == 64


@pytest.mark.parametrize("S", [8, 16, 32, 64])
@pytest.mark.parametrize("bi", [0, 1])
def test_spel_batches_vs_oracle(S, bi):
    from _me_cases import make_spel_job, run_oracle_spel

    r = np.random.default_rng(1100 + S + bi)
    pl = make_planes(r, True)
    base = make_spel_job(r, pl, S, bi)
    cases = []
    for _ in range(120):
        c = make_spel_job(r, pl, S, bi)
        for k in ("lambda_mv", "mot_other", "hpel_cnt", "qpel_cnt"):
            c[k] = base[k]
        cases.append(c)
    got = gpu_run_spel(cases)
    for i, c in enumerate(cases):
        e = run_oracle_spel(c)
        g = got[i]
        assert (int(g["cost"]), int(g["mv"][0]), int(g["mv"][1]), int(g["best_mv_bits"])) == (e.cost, e.mv[0], e.mv[1], e.best_mv_bits), (S, bi, i)


@pytest.mark.parametrize("S", [8, 16, 32, 64])
@pytest.mark.parametrize("bi", [0, 1])
def test_epzs_search_vs_oracle(S, bi):
    """xeve_amd.me.epzs_search_device = xeve_hip_me_epzs_jobs: pinter_me_epzs per block (diamond, refinement loop, sub-pel) on the GPU, vs the oracle"""
    import torch

    import xeve_amd
    from _me_cases import make_epzs_job, run_oracle_epzs
    from xeve_amd import me

    xeve_amd.init(0)
    dev = torch.device("cuda:0")
    r = np.random.default_rng(1200 + S + bi)
    pl = make_planes(r, True)
    base = make_epzs_job(r, pl, S, bi)
    cases = []
    for _ in range(100):
        c = make_epzs_job(r, pl, S, bi)
        for k in ("lambda_mv", "mot_other", "msr", "sr", "hpel_cnt", "qpel_cnt"):
            c[k] = base[k]
        cases.append(c)
    org, ref = torch.from_numpy(pl["org"]).to(dev), torch.from_numpy(pl["ref"]).to(dev)
    o0 = PAD * pl["s"] + PAD
    org_bi = torch.from_numpy(np.stack([c["org_bi"] for c in cases])).to(dev)
    args = (org, o0, pl["s"], ref, o0, pl["s"], [c["x"] for c in cases], [c["y"] for c in cases], [c["mvp"] for c in cases],
            S.bit_length() - 1, 10, base["lambda_mv"], 1, base["msr"], base["sr"], base["min_clip"], base["max_clip"], base["hpel_cnt"], base["qpel_cnt"])
    kw = dict(bi=bi, org_bi=org_bi, mv_start=[c["mv0"] for c in cases], extra_bits=base["mot_other"])
    exp = [run_oracle_epzs(c) for c in cases]
    cost, mv = me.epzs_search_device(*args, **kw)
    for i in range(len(cases)):
        assert (int(cost[i]), int(mv[i, 0]), int(mv[i, 1])) == exp[i], (S, bi, i)
    # the side effect on pi->mot_bits[lidx] (the next bi-directional search reads it): oracle -1 = untouched = 0 here
    cost, mv, mot = me.epzs_search_device(*args, with_mot_bits=True, **kw)
    for i, c in enumerate(cases):
        e = run_oracle_epzs(c, with_mot=True)
        assert int(mot[i]) == (e[3] if e[3] > 0 else 0), (S, bi, i)


@pytest.mark.parametrize("S", [8, 16, 32, 64])
def test_hip_epzs_raster_search_and_integer_refinement_vs_oracle(S):
    """the branches of pinter_me_epzs outside presets fast / medium: me_raster (me_complexity > 1) after a first search that ended far from its start,
    with refi 0 / 1, and me_ipel_refinement instead of the sub-pel pattern (me_level = ME_LEV_IPEL), uni- and bi-directional"""
    import torch

    import xeve_amd
    from _me_cases import make_epzs_job, run_oracle_epzs
    from xeve_amd import me

    xeve_amd.init(0)
    dev = torch.device("cuda:0")
    r = np.random.default_rng(3100 + S)
    pl = make_planes(r, True)
    org, ref = torch.from_numpy(pl["org"]).to(dev), torch.from_numpy(pl["ref"]).to(dev)
    o0 = PAD * pl["s"] + PAD
    rastered = 0
    for (bi, raster, refi, ipel) in [(0, 1, 0, 0), (0, 1, 1, 0), (0, 1, 1, 1), (0, 0, 0, 1), (1, 1, 0, 1), (1, 0, 0, 0)]:
        base = make_epzs_job(r, pl, S, bi)
        if ipel:
            base["hpel_cnt"], base["qpel_cnt"] = 0, 0
        cases = []
        for _ in range(60):
            c = make_epzs_job(r, pl, S, bi)
            for k in ("lambda_mv", "mot_other", "msr", "sr", "hpel_cnt", "qpel_cnt"):
                c[k] = base[k]
            c["mvp"] = (int(r.integers(-160, 161)), int(r.integers(-160, 161)))
            c["raster"], c["refi"] = raster, refi
            cases.append(c)
        org_bi = torch.from_numpy(np.stack([c["org_bi"] for c in cases])).to(dev)
        cost, mv, mot = me.epzs_search_device(org, o0, pl["s"], ref, o0, pl["s"], [c["x"] for c in cases], [c["y"] for c in cases], [c["mvp"] for c in cases],
                                              S.bit_length() - 1, 10, base["lambda_mv"], 1, base["msr"], base["sr"], base["min_clip"], base["max_clip"], base["hpel_cnt"],
                                              base["qpel_cnt"], bi=bi, org_bi=org_bi, mv_start=[c["mv0"] for c in cases], extra_bits=base["mot_other"], with_mot_bits=True,
                                              raster=bool(raster), refi=refi)
        for i, c in enumerate(cases):
            e = run_oracle_epzs(c, with_mot=True)
            assert (int(cost[i]), int(mv[i, 0]), int(mv[i, 1]), int(mot[i])) == (e[0], e[1], e[2], e[3] if e[3] > 0 else 0), (S, bi, raster, refi, ipel, i, c["mvp"])
            if raster and bi == 0:
                rastered += run_oracle_epzs(dict(c, raster=0), with_mot=True) != e
    assert rastered > 0


# ---- where candidates tie and search windows clip ------------------------------------------------------------------------------------------------------------------
def gpu_run_epzs(cases, bit_depth=10):
    """xeve_hip_me_epzs_jobs for cases that share planes, block size, bi and every launch-level parameter (raster, refi and the sub-pel counts among them) -> cost, mv, mot_bits"""
    import torch

    import xeve_amd
    from xeve_amd import me

    xeve_amd.init(0)
    dev = torch.device("cuda:0")
    c0 = cases[0]
    org, ref = plane_on_device(c0["org"], dev), plane_on_device(c0["ref"], dev)
    o0 = PAD * c0["s"] + PAD
    org_bi = torch.from_numpy(np.stack([c["org_bi"] for c in cases])).to(dev)
    return me.epzs_search_device(org, o0, c0["s"], ref, o0, c0["s"], [c["x"] for c in cases], [c["y"] for c in cases], [c["mvp"] for c in cases], c0["S"].bit_length() - 1,
                                 bit_depth, c0["lambda_mv"], 1, c0["msr"], c0["sr"], c0["min_clip"], c0["max_clip"], c0["hpel_cnt"], c0["qpel_cnt"], bi=c0["bi"], org_bi=org_bi,
                                 mv_start=[c["mv0"] for c in cases], extra_bits=c0["mot_other"], with_mot_bits=True, raster=bool(c0["raster"]), refi=c0["refi"])


def test_me_degenerate_matches_reference_goldens():
    """every row of tests/golden/me_degenerate_v1.npz -- the reference's own results on flat, periodic, outward and static content, bit depth 8 / 10 / 12 -- through the three
    entry points: the diamond, the 8 + 8 point sub-pel pattern, pinter_me_epzs plain, with the raster search (refi 0 / 1) and with the integer refinement"""
    from _me_cases import EPZS_VARIANTS, GOLDEN_SETS, epzs_variant_of, spel_case_of
    from _me_golden import golden_degenerate_cases

    n = 0
    for key, bd, c, dia, sp, ep in golden_degenerate_cases():
        g = gpu_run([c], bd)[0]
        assert (int(g["cost"]), int(g["mv"][0]), int(g["mv"][1]), int(g["beststep"])) == dia, (key, n, c["S"], c["bi"])
        g = gpu_run_spel([spel_case_of(c)], bd)[0]
        assert (int(g["cost"]), int(g["mv"][0]), int(g["mv"][1])) == sp, (key, n, "spel", c["S"], c["bi"])
        for v, e in zip(EPZS_VARIANTS, ep):
            cost, mv, mot = gpu_run_epzs([epzs_variant_of(c, v)], bd)
            assert (int(cost[0]), int(mv[0, 0]), int(mv[0, 1]), int(mot[0])) == (e[0], e[1], e[2], e[3] if e[3] > 0 else 0), (key, n, "epzs", v, c["S"], c["bi"])
        n += 1
    assert n == 24 * len(GOLDEN_SETS)


def _diamond_launch_vs_oracle(family, S, bi, bd=10):
    from _me_cases import assert_family_condition, degenerate_launch

    assert_family_condition(family, S, bi, bd)  # on the CPU, before anything goes to the GPU
    _, cases, exp = degenerate_launch(family, S, bi, bd)
    got = gpu_run(cases, bd)
    for i, (g, e) in enumerate(zip(got, exp)):
        assert (int(g["cost"]), int(g["mv"][0]), int(g["mv"][1]), int(g["beststep"]), int(g["best_mv_bits"])) == (e.cost, e.mv[0], e.mv[1], e.beststep, e.best_mv_bits), \
               (family, S, bi, bd, i, cases[i]["x"], cases[i]["y"], cases[i]["gmvp"], cases[i]["range"])


TIE_LAUNCHES = [(f, S, bi) for f in ("flat", "periodic4", "periodic8", "periodic16", "periodic32", "outward") for S in (8, 16, 32, 64) for bi in (0, 1, 2)
                if bi != 1 or f in ("flat", "periodic4", "outward")]  # (bi == 1 has no rings: its 121-candidate round is the two-pass path)


@pytest.mark.parametrize("family,S,bi", TIE_LAUNCHES, ids=["%s-%d-%d" % t for t in TIE_LAUNCHES])
def test_me_ties_and_clipped_windows_vs_oracle(family, S, bi):
    """100 jobs per launch: flat and periodic4 tie inside the dense round, periodic8 / 16 / 32 in the ring of radius 4 / 8 / 16 (two exact matches at equal vector bits, the
    earlier one wins), outward has its centre on a clip limit and a cut dense grid.  The oracle is pinned to the reference on this content by tests/test_me_oracle_vs_ref.py."""
    _diamond_launch_vs_oracle(family, S, bi)


@pytest.mark.parametrize("family", ["periodic8", "outward"])
@pytest.mark.parametrize("bd", [8, 12])
def test_me_ties_and_clipped_windows_at_bit_depth_8_and_12(family, bd):
    """the SAD is shifted by bit_depth - 8: at 12 bits four low bits are gone and ordinary content ties; S 8 and 64, bi 0 and 2"""
    for S in (8, 64):
        for bi in (0, 2):
            _diamond_launch_vs_oracle(family, S, bi, bd)


SUB_FAMILIES = [("flat", "flat"), ("periodic4", "flat"), ("periodic8", "flat"), ("periodic16", "flat"), ("periodic32", "flat"), ("outward", "flat"), ("static", "flat"),
                ("static", "periodic")]
N_SUB = 40


@pytest.mark.parametrize("family,kind", SUB_FAMILIES, ids=[f if f != "static" else f + "_" + k for f, k in SUB_FAMILIES])
def test_spel_ties_vs_oracle(family, kind):
    """all 8 half-pel and 8 quarter-pel points around an integer-pel predictor equal to the centre: (-2, 0) and (2, 0) cost the same bits, and so do the four quarter-pel
    axis points -- on flat and flat static content they tie outright, and every job must end on (-2, 0), the first of them"""
    from _me_cases import degenerate_launch, run_oracle_spel, spel_case_of

    for S in (8, 16, 32, 64):
        for bi in (0, 1):
            cases = [spel_case_of(c) for c in degenerate_launch(family, S, bi, 10, kind)[1][:N_SUB]]
            exp = [run_oracle_spel(c) for c in cases]
            if family in ("flat", "static") and kind == "flat":  # every SAD is the same: (-2, 0), the first of the four cheapest half-pel points, and no quarter-pel point is cheaper
                assert all((e.mv[0] - c["mvi"][0], e.mv[1] - c["mvi"][1]) == (-2, 0) for c, e in zip(cases, exp))
            got = gpu_run_spel(cases)
            for i, (g, e) in enumerate(zip(got, exp)):
                assert (int(g["cost"]), int(g["mv"][0]), int(g["mv"][1]), int(g["best_mv_bits"])) == (e.cost, e.mv[0], e.mv[1], e.best_mv_bits), (family, kind, S, bi, i)


@pytest.mark.parametrize("family,kind", SUB_FAMILIES, ids=[f if f != "static" else f + "_" + k for f, k in SUB_FAMILIES])
def test_epzs_ties_and_clipped_windows_vs_oracle(family, kind):
    """the whole pinter_me_epzs through epzs_search_device on the same content: the first search, the raster search (the periodic16 / 32 launches reach it: their first search
    ends at step 8 / 16, and from S = 32 on its grid sees one SAD at every point, 81 points for refi 0), the refinement loop (on static and periodic content it re-centres on
    a zero-SAD plateau), the sub-pel pattern or the integer refinement; cost, vector and mot_bits"""
    from _me_cases import EPZS_VARIANTS, degenerate_launch, epzs_variant_of, run_oracle_epzs

    for S in (8, 16, 32, 64):
        for bi, v in [(0, EPZS_VARIANTS[0]), (0, EPZS_VARIANTS[1]), (0, EPZS_VARIANTS[4]), (1, EPZS_VARIANTS[0]), (1, EPZS_VARIANTS[3])]:
            cases = [epzs_variant_of(c, v) for c in degenerate_launch(family, S, bi, 10, kind)[1][:N_SUB]]
            cost, mv, mot = gpu_run_epzs(cases)
            for i, c in enumerate(cases):
                e = run_oracle_epzs(c, with_mot=True)
                assert (int(cost[i]), int(mv[i, 0]), int(mv[i, 1]), int(mot[i])) == (e[0], e[1], e[2], e[3] if e[3] > 0 else 0), (family, kind, S, bi, v, i, c["mvp"])


# ---- the last CTU column of an 8192-wide picture: quarter-pel frame coordinates beyond an s16 -------------------------------------------------------------------------
@pytest.mark.parametrize("S", [64, 32, 16, 8])
def test_me_right_edge_matches_reference_goldens_and_oracle(S):
    """_me_cases' right-edge family at x = 8192 - S: predictors and start vectors whose frame coordinate wraps as the reference's s16 gmvp / mvi do (three jobs of five
    per launch; each differs from its twin without a wrap -- both asserted on the CPU first, from the reference's recorded results), for bi 0 / 1 / 2 and the ranges of
    the four presets.  xeve_hip_me_ipel_diamond_jobs takes the wrapped values as its caller hands them down; xeve_hip_me_spel_pattern_jobs wraps cx and mv_x itself (around
    the true motion, and around the vector the diamond brought back from the picture's left end, which wraps back); xeve_hip_me_epzs_jobs makes gmvp and mvi from the raw
    mvp -- its own casts -- and runs the raster search and the integer refinement behind a wrapped first search.  Against tests/golden/me_right_edge_v1.npz and, for
    best_mv_bits, the oracle."""
    from _me_cases import assert_right_edge_conditions, right_edge_epzs_case, right_edge_spel_case, run_oracle_spel
    from _me_golden import golden_right_edge_cases

    launches = {}
    for L, t, c, g in golden_right_edge_cases():
        if L[0] == S:
            launches.setdefault(L, []).append((c, g))
    assert len(launches) == 12
    assert assert_right_edge_conditions([(L, c, g["dia"], g["twin_dia"], g["epzs"], g["twin_epzs"]) for L, rows in launches.items() for c, g in rows]) == 36
    for L, rows in launches.items():
        cases = [c for c, _ in rows]
        got = gpu_run(cases)
        for i, (c, g) in enumerate(rows):
            e, r = run_oracle(c), got[i]
            assert (int(r["cost"]), int(r["mv"][0]), int(r["mv"][1]), int(r["beststep"])) == g["dia"] and int(r["best_mv_bits"]) == e.best_mv_bits, (L, i, "diamond")
        for key, scs in (("spel", [right_edge_spel_case(c) for c in cases]), ("spel_at_dia", [right_edge_spel_case(c, g["dia"][1:3]) for c, g in rows])):
            got = gpu_run_spel(scs)
            for i, (c, g) in enumerate(rows):
                e, r = run_oracle_spel(scs[i]), got[i]
                assert (int(r["cost"]), int(r["mv"][0]), int(r["mv"][1])) == g[key] and int(r["best_mv_bits"]) == e.best_mv_bits, (L, i, key)
        for key, ipel in (("epzs", False), ("epzs_ipel", True)):
            cost, mv, mot = gpu_run_epzs([right_edge_epzs_case(c, ipel=ipel) for c in cases])
            for i, (c, g) in enumerate(rows):
                e = g[key]
                assert (int(cost[i]), int(mv[i, 0]), int(mv[i, 1]), int(mot[i])) == (e[0], e[1], e[2], e[3] if e[3] > 0 else 0), (L, i, key, c["mvp"])
