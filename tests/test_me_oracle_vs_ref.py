"""Pins the oracle's integer-pel diamond search (xo_me_ipel_diamond, xo_mv_bits) against the REAL static functions of
the reference (src_base/xeve_pinter.c:74-120, 363-551), reached through oracle/ref_me_driver.c, which compiles the
reference's xeve_pinter.c in place."""
import ctypes as C

import numpy as np
import pytest

from _libs import oracle_me, ptr, ref_me
from ctypes import c_int, c_void_p
from _me_cases import PAD, REFI_BITS_2_0, make_case, run_oracle

pytestmark = pytest.mark.skipif(ref_me() is None, reason="oracle/_ref/libref_me.so not built (needs /root/reference)")


def test_mv_bits_table_closed_form():
    O, R = oracle_me(), ref_me()
    assert R.refdrv_refi_bits(2, 0) == REFI_BITS_2_0
    for mvd in list(range(-2100, 2101)) + [-5000, 5000, -32768, 32767, 4095, 4096, -4096, 8191, 8192, 16383, 16384]:
        assert O.xo_mv_bits(mvd, 0) + R.refdrv_refi_bits(2, 1) == R.refdrv_mv_bits(mvd, 0, 2, 1), mvd
        assert O.xo_mv_bits(3, mvd) + R.refdrv_refi_bits(1, 0) == R.refdrv_mv_bits(3, mvd, 1, 0), mvd


def run_ref(c, bit_depth=10):
    R = ref_me()
    lg = c["S"].bit_length() - 1
    out = (C.c_int * 4)()
    org0, ref0 = ptr(c["org"], PAD * c["s"] + PAD), ptr(c["ref"], PAD * c["s"] + PAD)
    rng = np.array(c["range"], np.int16)
    gmvp, mvi = np.array(c["gmvp"], np.int16), np.array(c["mvi"], np.int16)
    mn, mx = np.array(c["min_clip"], np.int32), np.array(c["max_clip"], np.int32)
    # gop_size / poc chosen so that get_range_ipel derives exactly c["sr"]: (msr * |poc - ref_poc| + gop/2) / gop = sr
    gop, poc, ref_poc = c["msr"], c["sr"], 0
    cost = R.refdrv_me_ipel_diamond(org0, c["s"], ptr(c["org_bi"]), ref0, c["s"], c["x"], c["y"], lg, lg, bit_depth, ptr(rng), ptr(gmvp), ptr(mvi),
                                    c["bi"], c["faststep"], c["lambda_mv"], 2, 0, c["mot_other"], c["msr"], gop, poc, ref_poc, ptr(mn), ptr(mx),
                                    c["beststep_in"], out)
    return cost, out[0], out[1], out[2], out[3]


@pytest.mark.parametrize("bi", [0, 1, 2])
@pytest.mark.parametrize("textured", [False, True])
def test_me_ipel_diamond_matches_reference(bi, textured):
    r = np.random.default_rng(900 + bi * 2 + textured)
    steps = set()
    for it in range(60):
        c = make_case(r, int(r.choice([8, 16, 32, 64])), bi, textured)
        cost, mvx, mvy, beststep, mot = run_ref(c)
        res = run_oracle(c)
        assert (res.cost, res.mv[0], res.mv[1], res.beststep) == (cost, mvx, mvy, beststep), (it, c["S"], c["x"], c["y"])
        if bi != 1 and res.best_mv_bits > 0:
            assert mot == res.best_mv_bits
        steps.add(beststep)
    if textured and bi != 1:
        assert max(steps) >= 4  # the diamond rings were actually exercised


def run_ref_spel(c, bit_depth=10):
    from _libs import ref_spel

    R = ref_spel()
    lg = c["S"].bit_length() - 1
    out = (C.c_int * 3)()
    gmvp, mvi = np.array(c["gmvp"], np.int16), np.array(c["mvi"], np.int16)
    cost = R.refdrv_me_spel_pattern(ptr(c["org"], PAD * c["s"] + PAD), c["s"], ptr(c["org_bi"]), ptr(c["ref"], PAD * c["s"] + PAD), c["s"], c["x"], c["y"],
                                    lg, lg, bit_depth, ptr(gmvp), ptr(mvi), c["bi"], c["lambda_mv"], 2, 0, c["mot_other"], c["hpel_cnt"], c["qpel_cnt"], out)
    return cost, out[0], out[1], out[2]


@pytest.mark.parametrize("bi", [0, 1])
@pytest.mark.parametrize("textured", [False, True])
def test_me_spel_pattern_matches_reference(bi, textured):
    from _me_cases import make_planes, make_spel_job, run_oracle_spel

    r = np.random.default_rng(950 + bi * 2 + textured)
    pl = make_planes(r, textured)
    for it in range(60):
        c = make_spel_job(r, pl, int(r.choice([8, 16, 32, 64])), bi)
        cost, mvx, mvy, mot = run_ref_spel(c)
        res = run_oracle_spel(c)
        assert (res.cost, res.mv[0], res.mv[1]) == (cost, mvx, mvy), (it, c["S"], c["hpel_cnt"], c["qpel_cnt"])
        if not bi and res.best_mv_bits > 0:
            assert mot == res.best_mv_bits


@pytest.mark.parametrize("bi", [0, 1])
@pytest.mark.parametrize("textured", [False, True])
def test_me_epzs_matches_reference(bi, textured):
    """the whole per-list search of pinter_me_epzs (me_complexity 1): diamond, refinement loop, sub-pel pattern"""
    from _libs import ref_epzs
    from _me_cases import make_epzs_job, make_planes, run_oracle_epzs

    R = ref_epzs()
    r = np.random.default_rng(970 + bi * 2 + textured)
    pl = make_planes(r, textured)
    moved = 0
    for it in range(50):
        c = make_epzs_job(r, pl, int(r.choice([8, 16, 32, 64])), bi)
        lg = c["S"].bit_length() - 1
        mvp, mv = np.array(c["mvp"], np.int16), np.array(c["mv0"], np.int16)
        mn, mx = np.array(c["min_clip"], np.int32), np.array(c["max_clip"], np.int32)
        cost = R.refdrv_me_epzs(ptr(c["org"], PAD * c["s"] + PAD), c["s"], ptr(c["org_bi"]), ptr(c["ref"], PAD * c["s"] + PAD), c["s"], c["x"], c["y"], lg, lg,
                                10, ptr(mvp), ptr(mv), bi, c["lambda_mv"], 2, 0, c["mot_other"], c["msr"], c["msr"], c["sr"], 0, ptr(mn), ptr(mx),
                                c["hpel_cnt"], c["qpel_cnt"])
        R.refdrv_me_epzs_mot_bits.restype = C.c_int
        assert run_oracle_epzs(c, with_mot=True) == (cost, int(mv[0]), int(mv[1]), R.refdrv_me_epzs_mot_bits()), (it, c["S"])
        moved += (int(mv[0]), int(mv[1])) != tuple(c["mvp"])
    assert moved > 25


def test_epzs_with_raster_search_and_integer_refinement_matches_reference():
    """the branches of pinter_me_epzs the presets fast / medium do not take: me_raster (me_complexity > 1: placebo) after a first search that ended far
    from its start, with the step scaled by refi + 1, and me_ipel_refinement in place of the sub-pel pattern (me_level = ME_LEV_IPEL)"""
    from _me_cases import make_epzs_job, make_planes, run_oracle_epzs

    R = ref_me()
    R.refdrv_me_epzs_x.restype = C.c_uint32
    R.refdrv_me_epzs_x.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, C.c_uint32] + [c_int] * 7 + \
                                  [c_void_p, c_void_p, c_int, c_int, c_int]
    R.refdrv_me_epzs_mot_bits.restype = C.c_int
    r = np.random.default_rng(2024)
    rastered = refined = 0
    for it in range(160):
        pl = make_planes(r, textured=it % 4 != 0)
        S, bi = int(r.choice([8, 16, 32, 64])), int(r.choice([0, 0, 0, 1]))
        c = make_epzs_job(r, pl, S, bi)
        c["raster"], c["refi"] = int(r.random() < 0.75), int(r.integers(0, 2))
        if r.random() < 0.4:
            c["hpel_cnt"], c["qpel_cnt"] = 0, 0
            refined += 1
        c["mvp"] = (int(r.integers(-160, 161)), int(r.integers(-160, 161)))  # far from the true motion: the first search walks, beststep grows
        lg = S.bit_length() - 1
        mvp, mv = np.array(c["mvp"], np.int16), np.array(c["mv0"], np.int16)
        mn, mx = np.array(c["min_clip"], np.int32), np.array(c["max_clip"], np.int32)
        cost = R.refdrv_me_epzs_x(ptr(c["org"], PAD * c["s"] + PAD), c["s"], ptr(c["org_bi"]), ptr(c["ref"], PAD * c["s"] + PAD), c["s"], c["x"], c["y"], lg, lg, 10,
                                  ptr(mvp), ptr(mv), bi, c["lambda_mv"], 2, c["refi"], c["mot_other"], c["msr"], c["msr"], c["sr"], 0, ptr(mn), ptr(mx), c["hpel_cnt"],
                                  c["qpel_cnt"], 2 if c["raster"] else 1)
        got = run_oracle_epzs(c, with_mot=True)
        assert got == (cost, int(mv[0]), int(mv[1]), R.refdrv_me_epzs_mot_bits()), (it, S, bi, c["raster"], c["refi"], c["hpel_cnt"], got, cost, mv)
        c0 = dict(c, raster=0)
        rastered += c["raster"] and bi == 0 and run_oracle_epzs(c0, with_mot=True) != got
    assert rastered > 10 and refined > 30, (rastered, refined)


# ---- degenerate content: the oracle must break ties and clip windows as xeve_pinter.c does, or HIP == oracle proves nothing there ------------------------------------
from _me_cases import EPZS_VARIANTS, GOLDEN_SETS, degenerate_golden_jobs, epzs_variant_of, make_degenerate_jobs, spel_case_of  # noqa: E402


def run_ref_epzs(c, bit_depth=10):
    """(cost, mv x, mv y, pi->mot_bits[lidx]) of the reference's pinter_me_epzs; c["raster"]: me_complexity 2, c["refi"]: the raster step's factor"""
    R = ref_me()
    R.refdrv_me_epzs_x.restype = C.c_uint32
    R.refdrv_me_epzs_x.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, C.c_uint32] + [c_int] * 7 + \
                                  [c_void_p, c_void_p, c_int, c_int, c_int]
    R.refdrv_me_epzs_mot_bits.restype = C.c_int
    lg = c["S"].bit_length() - 1
    mvp, mv = np.array(c["mvp"], np.int16), np.array(c["mv0"], np.int16)
    mn, mx = np.array(c["min_clip"], np.int32), np.array(c["max_clip"], np.int32)
    cost = R.refdrv_me_epzs_x(ptr(c["org"], PAD * c["s"] + PAD), c["s"], ptr(c["org_bi"]), ptr(c["ref"], PAD * c["s"] + PAD), c["s"], c["x"], c["y"], lg, lg, bit_depth,
                              ptr(mvp), ptr(mv), c["bi"], c["lambda_mv"], 2, c.get("refi", 0), c["mot_other"], c["msr"], c["msr"], c["sr"], 0, ptr(mn), ptr(mx), c["hpel_cnt"],
                              c["qpel_cnt"], 2 if c.get("raster", 0) else 1)
    return cost, int(mv[0]), int(mv[1]), R.refdrv_me_epzs_mot_bits()


@pytest.mark.parametrize("key", [g[0] for g in GOLDEN_SETS])
def test_searches_match_reference_where_candidates_tie_and_windows_clip(key):
    """flat, periodic, outward and static content at every S and bi (the rows of tests/golden/me_degenerate_v1.npz) and 20 further jobs per S and bi: me_ipel_diamond (bi 0, 1, 2),
    me_spel_pattern with all 8 + 8 points around an integer-pel predictor, pinter_me_epzs plain, with the raster search (refi 0 / 1) and with the integer refinement; the
    sets *_bd8 / *_bd12 at bit depth 8 and 12 (the SAD loses bit_depth - 8 bits: more ties)"""
    from _me_cases import run_oracle_epzs, run_oracle_spel

    _, family, bd, kind = GOLDEN_SETS[[g[0] for g in GOLDEN_SETS].index(key)]
    pl, _, cases = degenerate_golden_jobs(key)
    r = np.random.default_rng(7300 + len(key) + bd)
    for S in (8, 16, 32, 64):
        for bi in (0, 1, 2):
            cases += make_degenerate_jobs(r, family, S, bi, 20, bd, vertical=bool((S.bit_length() + bi) % 2), static_kind=kind)[1]
    rastered = 0
    for it, c in enumerate(cases):
        cost, mvx, mvy, beststep, mot = run_ref(c, bd)
        res = run_oracle(c, bd)
        assert (res.cost, res.mv[0], res.mv[1], res.beststep) == (cost, mvx, mvy, beststep), (key, it, c["S"], c["bi"], c["x"], c["y"])
        if c["bi"] != 1 and res.best_mv_bits > 0:
            assert mot == res.best_mv_bits, (key, it)
        sc = spel_case_of(c)
        cost, mvx, mvy, mot = run_ref_spel(sc, bd)
        res = run_oracle_spel(sc, bd)
        assert (res.cost, res.mv[0], res.mv[1]) == (cost, mvx, mvy), (key, it, "spel", c["S"], c["bi"])
        if not sc["bi"] and res.best_mv_bits > 0:
            assert mot == res.best_mv_bits, (key, it, "spel")
        for v in EPZS_VARIANTS:
            ec = epzs_variant_of(c, v)
            got = run_oracle_epzs(ec, with_mot=True, bit_depth=bd)
            assert got == run_ref_epzs(ec, bd), (key, it, "epzs", v, c["S"], c["bi"])
            rastered += bool(v[0] and not ec["bi"] and got != run_oracle_epzs(dict(ec, raster=0), with_mot=True, bit_depth=bd))
    # (the raster search runs when the first search ended beyond step 5: never on flat content, where all SADs are equal and the dense round wins; always on periodic16 / 32,
    # whose first search ends at step 8 / 16 -- there its grid of step S / 2 sees one SAD at every point from S = 32 on, 81 points for refi 0, but cannot beat the exact match)
    print(key, "raster search changed the result of", rastered, "jobs")
    if family == "outward" and bd == 10:
        assert rastered > 0


def test_degenerate_fixture_holds_what_the_reference_gives():
    """tests/golden/me_degenerate_v1.npz (what the GPU suite holds the device code to, where there is no reference) against the reference itself"""
    from _me_golden import golden_degenerate_cases

    n = 0
    for key, bd, c, dia, sp, ep in golden_degenerate_cases():
        assert run_ref(c, bd)[:4] == dia and run_ref_spel(spel_case_of(c), bd)[:3] == sp, (key, n)
        assert [run_ref_epzs(epzs_variant_of(c, v), bd) for v in EPZS_VARIANTS] == ep, (key, n)
        n += 1
    assert n == 24 * len(GOLDEN_SETS)


# ---- the last CTU column of an 8192-wide picture: gmvp, mvi, cx, mv_x and every returned vector are s16 in the reference, and there they wrap --------------------------------
from _me_cases import RE_SIZES  # noqa: E402


@pytest.mark.parametrize("S", RE_SIZES)
def test_searches_match_reference_where_frame_coordinates_pass_an_s16(S):
    """_me_cases' right-edge family, the 60 jobs of one block size: me_ipel_diamond (bi 0, 1, 2), me_spel_pattern around the true motion and around the diamond's result,
    pinter_me_epzs with the preset's sub-pel counts (placebo: me_complexity 2, the raster search) and with the integer refinement, and all of it for each job's twin
    256 samples further left.  (a) three jobs of five per launch wrap; (b) each of them differs from its twin in the reference's results.  The same rows, recorded, are
    tests/golden/me_right_edge_v1.npz (held to the reference below)."""
    from _me_cases import (RE_LAUNCHES, assert_right_edge_conditions, right_edge_epzs_case, right_edge_jobs, right_edge_spel_case, run_oracle_epzs, run_oracle_spel)

    entries = []
    for L in [t for t in RE_LAUNCHES if t[0] == S]:
        for twin in (False, True):
            for k, c in enumerate(right_edge_jobs(*L, twin=twin)):
                cost, mvx, mvy, beststep, mot = dia = run_ref(c)
                res = run_oracle(c)
                assert (res.cost, res.mv[0], res.mv[1], res.beststep) == dia[:4], (L, twin, k)
                if c["bi"] != 1 and res.best_mv_bits > 0:
                    assert mot == res.best_mv_bits, (L, twin, k)
                for sc in (right_edge_spel_case(c), right_edge_spel_case(c, (mvx, mvy))):
                    cost, sx, sy, mot = run_ref_spel(sc)
                    res = run_oracle_spel(sc)
                    assert (res.cost, res.mv[0], res.mv[1]) == (cost, sx, sy), (L, twin, k, "spel", sc["mvi"])
                    if not sc["bi"] and res.best_mv_bits > 0:
                        assert mot == res.best_mv_bits, (L, twin, k, "spel")
                ep = None
                for ipel in (True, False):
                    ec = right_edge_epzs_case(c, ipel=ipel)
                    ep = run_ref_epzs(ec)
                    assert run_oracle_epzs(ec, with_mot=True) == ep, (L, twin, k, "epzs", ipel)
                if twin:
                    entries[len(entries) - 5 + k] += (dia[:4], ep)
                else:
                    entries.append((L, c, dia[:4], ep))
    assert_right_edge_conditions([(L, c, dia, tdia, ep, tep) for L, c, dia, ep, tdia, tep in entries])


def test_right_edge_fixture_holds_what_the_reference_gives():
    """tests/golden/me_right_edge_v1.npz (what the CPU suite holds the oracle to and the GPU suite the device code, where there is no reference) against the reference itself"""
    from _me_cases import RE_JOBS, right_edge_epzs_case, right_edge_jobs, right_edge_spel_case
    from _me_golden import golden_right_edge_cases

    n = 0
    for L, t, c, g in golden_right_edge_cases():
        w = right_edge_jobs(*L, twin=True)[t]
        assert run_ref(c)[:4] == g["dia"] and run_ref(w)[:4] == g["twin_dia"], (L, t)
        assert run_ref_spel(right_edge_spel_case(c))[:3] == g["spel"] and run_ref_spel(right_edge_spel_case(c, g["dia"][1:3]))[:3] == g["spel_at_dia"], (L, t)
        assert run_ref_epzs(right_edge_epzs_case(c)) == g["epzs"] and run_ref_epzs(right_edge_epzs_case(c, ipel=True)) == g["epzs_ipel"], (L, t)
        assert run_ref_epzs(right_edge_epzs_case(w)) == g["twin_epzs"], (L, t)
        n += 1
    assert n == RE_JOBS
