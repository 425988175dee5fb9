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
