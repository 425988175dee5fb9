"""CPU suite: the motion searches where candidates tie and search windows clip, on the oracle alone.  The families of _me_cases (flat, periodic, outward, static) are
built for properties the noise and texture generators do not reach; here every launch the GPU suite uses is checked for its property BEFORE anything goes to the GPU
(the counters are numpy SADs and xo_mv_bits, no search code), and the oracle is held to the reference's recorded results (tests/golden/me_degenerate_v1.npz)."""
import pytest

from _me_cases import (BATCH_STEPS, EPZS_VARIANTS, GOLDEN_SETS, ME_FAMILIES, assert_family_condition, batch_launches, epzs_variant_of, run_oracle, run_oracle_epzs,
                       run_oracle_spel, spel_case_of)
from _me_golden import golden_degenerate_cases

LAUNCHES = [(f, S, bi) for f in ME_FAMILIES for S in (8, 16, 32, 64) for bi in (0, 1, 2) if bi != 1 or f in ("flat", "periodic4", "outward")]
BIT_DEPTH_LAUNCHES = [(f, S, bi, bd) for f in ("periodic8", "outward") for S in (8, 64) for bi in (0, 2) for bd in (8, 12)]


def test_oracle_reproduces_the_references_results_on_degenerate_content():
    n = 0
    for key, bd, c, dia, sp, ep in golden_degenerate_cases():
        e = run_oracle(c, bd)
        assert (e.cost, e.mv[0], e.mv[1], e.beststep) == dia, (key, n)
        s = run_oracle_spel(spel_case_of(c), bd)
        assert (s.cost, s.mv[0], s.mv[1]) == sp, (key, n)
        assert [run_oracle_epzs(epzs_variant_of(c, v), True, bd) for v in EPZS_VARIANTS] == ep, (key, n)
        n += 1
    assert n == 24 * len(GOLDEN_SETS)


@pytest.mark.parametrize("family,S,bi", LAUNCHES, ids=["%s-%d-%d" % t for t in LAUNCHES])
def test_every_family_shows_its_property_on_the_oracle(family, S, bi):
    assert_family_condition(family, S, bi)


@pytest.mark.parametrize("family,S,bi,bd", BIT_DEPTH_LAUNCHES, ids=["%s-%d-%d-bd%d" % t for t in BIT_DEPTH_LAUNCHES])
def test_every_family_shows_its_property_at_bit_depth_8_and_12(family, S, bi, bd):
    assert_family_condition(family, S, bi, bd)


@pytest.mark.parametrize("S,bi,textured", sorted(BATCH_STEPS))
def test_the_noise_and_texture_batches_end_at_as_many_steps_as_recorded(S, bi, textured):
    """test_hip_me.py::test_me_batches_vs_oracle asserts _me_cases.BATCH_STEPS, the number of distinct beststep values of each of its 24 settings: the oracle's, counted here"""
    steps = set(run_oracle(c).beststep for cases in batch_launches(S, bi, textured) for c in cases)
    assert len(steps) == BATCH_STEPS[(S, bi, textured)], sorted(steps)
    assert bi == 1 or len(steps) >= 3


# ---- the last CTU column of an 8192-wide picture: quarter-pel frame coordinates beyond an s16 (_me_cases: the right-edge family) ------------------------------------------
def test_oracle_reproduces_the_references_results_where_frame_coordinates_pass_an_s16():
    """every row of tests/golden/me_right_edge_v1.npz: S 64 / 32 / 16 / 8 at x = 8192 - S, bi 0 / 1 / 2, the ranges of presets fast / medium / slow / placebo, predictors with
    (x << 2) + mvp_x = 32 764, 32 767, 32 768, 32 800, 33 500 -- the diamond, the sub-pel pattern, pinter_me_epzs with the preset's sub-pel counts (placebo: with the raster
    search) and with the integer refinement.  (a) 144 of the 240 jobs wrap, three of five in every launch; (b) every one of them differs from its twin 256 samples further
    left in the reference's own results.

    The sub-pel stage: the pattern offsets alone cannot wrap cx / mv_x of me_spel_pattern -- an integer search ends inside [min_clip, max_clip], so cx <= 4 * 8191 = 32 764,
    a half-pel point <= 32 766 and a quarter-pel point around it <= 32 767, whatever me_sub_range says (search_range_spel is stored and never read: the patterns are the
    fixed +-2 / +-1 tables).  It IS reached through the integer stage: a wrapped start sends the diamond to the picture's left end, the vector it returns,
    ((best - x) << 2) with best near -127 and x >= 8128, has wrapped as an s16 as well, and cx = mvi + (x << 2) wraps back to the left end's coordinate (140 of the 144
    wrapped jobs; spel_at_dia runs exactly that, and so does every epzs row).

    The BI_NORMAL jobs with a wrapped start are a leaf state, NOT an encoder state.  Here bi 1 is handed mv0 = mvp rounded to integer pel, so mvi = mv0 + (x << 2) wraps,
    the one round finds no candidate, and the sub-pel pattern runs at cx near -32 768: its points lie about 8192 samples left of the block, in the plane's previous row, and
    those rows of the fixture depend on the test plane's stride (the same memory for the reference, the oracle and the device here, which is all a leaf comparison
    needs).  In an encode analyze_bi starts BI_NORMAL from the vector the uni-directional search of that list returned (xeve_pinter.c: mv of pinter_me_epzs), and that
    vector is ((best - x) << 2) + a sub-pel offset for a position best inside [min_clip, max_clip]: either it did not wrap, and mv + (x << 2) <= 4 * (w - 1) + 3 = 32 767
    fits; or it is the wrapped vector of a position at the left end, and mv + (x << 2) wraps BACK to that position's coordinate, >= 4 * min_clip - 3.  Either way mvi names
    a position inside the picture's padded rows: no encode reads the previous row, which is why the accepted width stays 8192."""
    from _me_cases import (RE_JOBS, RE_SPEL_WRAPS, RE_WRAPPED, assert_right_edge_conditions, right_edge_epzs_case, right_edge_spel_case, right_edge_wrapped,
                           spel_wraps)
    from _me_golden import golden_right_edge_cases

    entries, n, sub = [], 0, 0
    for L, t, c, g in golden_right_edge_cases():
        e = run_oracle(c)
        assert (e.cost, e.mv[0], e.mv[1], e.beststep) == g["dia"], (L, t)
        for key, sc in (("spel", right_edge_spel_case(c)), ("spel_at_dia", right_edge_spel_case(c, g["dia"][1:3]))):
            s = run_oracle_spel(sc)
            assert (s.cost, s.mv[0], s.mv[1]) == g[key], (L, t, key)
        assert run_oracle_epzs(right_edge_epzs_case(c), True) == g["epzs"], (L, t, "epzs")
        assert run_oracle_epzs(right_edge_epzs_case(c, ipel=True), True) == g["epzs_ipel"], (L, t, "epzs, integer refinement")
        entries.append((L, c, g["dia"], g["twin_dia"], g["epzs"], g["twin_epzs"]))
        sub += right_edge_wrapped(c) and spel_wraps(c, g["dia"])
        n += 1
    assert n == RE_JOBS and assert_right_edge_conditions(entries) == RE_WRAPPED and sub == RE_SPEL_WRAPS


def test_the_raster_search_runs_on_wrapped_jobs():
    """preset placebo, bi 0: the first search of a wrapped job ends far from its start (beststep 32 or 64), me_raster runs over the range the diamond left at the picture's
    left end and changes the result of some of them"""
    from _me_cases import RE_SIZES, right_edge_epzs_case, right_edge_jobs, right_edge_wrapped

    cases = [right_edge_epzs_case(c) for S in RE_SIZES for c in right_edge_jobs(S, 0, "placebo") if right_edge_wrapped(c)]
    changed = sum(run_oracle_epzs(c, True) != run_oracle_epzs(dict(c, raster=0), True) for c in cases)
    print(changed, "of", len(cases))
    assert len(cases) == 12 and changed >= 4
