"""xeve_pinter_analyze_cu: the oracle's restatement against the committed reference goldens (runs without the reference)."""
import numpy as np

from _inter_cases import mask_unobservable
from _inter_golden import CASES, RIGHT_EDGE_CASES, golden
from _libs import INTER_RESULT_DTYPE, SBAC_DTYPE, oracle_inter, ptr
from _mc_cases import refpic_table


def oracle_against(right_edge):
    O = oracle_inter()
    n, modes = 0, set()
    for c in golden(right_edge):
        refs, org = c["refs"], c["org"]
        tab = refpic_table(refs, lambda a, off: int(a.ctypes.data) + 2 * off)
        org_ptrs = np.array([int(org[0].ctypes.data) + 2 * refs["org_l"], int(org[1].ctypes.data) + 2 * refs["org_c"],
                             int(org[2].ctypes.data) + 2 * refs["org_c"]], np.uint64)
        for i in range(len(c["jobs"])):
            res, best = np.zeros(1, INTER_RESULT_DTYPE), np.zeros(1, SBAC_DTYPE)
            co = [np.zeros(c["coef"][k].shape[1], np.int16) for k in range(3)]
            rc = [np.zeros(c["coef"][k].shape[1], np.int16) for k in range(3)]
            O.xo_pinter_analyze_cu(ptr(org_ptrs), refs["s_l"], refs["s_c"], ptr(tab), refs["s_l"], refs["s_c"], ptr(c["states"]), c["P"], ptr(c["jobs"][i:i + 1]),
                                   ptr(res), ptr(co[0]), ptr(co[1]), ptr(co[2]), ptr(rc[0]), ptr(rc[1]), ptr(rc[2]), ptr(best))
            modes.add(int(res["best_idx"][0]))
            assert mask_unobservable(res, c["slice_type"]).tobytes() == c["res"][i:i + 1].tobytes(), (n, i, res, c["res"][i])
            for k in range(3 if c["idc"] else 1):
                assert np.array_equal(co[k], c["coef"][k][i]) and np.array_equal(rc[k], c["rec"][k][i]), (n, i, k)
            assert best.tobytes() == c["best"][i:i + 1].tobytes(), (n, i)
        n += 1
    return n, modes


def test_oracle_pinter_analyze_cu_matches_reference_goldens():
    n, modes = oracle_against(False)
    assert n == len(CASES) and modes == {0, 1, 2, 3, 4}, modes


RIGHT_EDGE_WRAPPED = [12, 11, 11, 0, 12, 11, 7]  # per case of _inter_golden.RIGHT_EDGE_CASES, of 12 jobs each


def test_the_right_edge_jobs_wrap():
    """how many jobs of each right-edge case have a neighbour vector with (x << 2) + mv_x > 32 767 (pinter_me_epzs' gmvp / mvi for it wrap): 64 of 84, none at CU size 64,
    whose only position is x = 8128 (4 * 8128 + 252 = 32 764)"""
    from _inter_cases import right_edge_wrapped
    from _inter_golden import case_inputs

    got = [int(right_edge_wrapped(case_inputs(case, True)[4], case[6]).sum()) for case in RIGHT_EDGE_CASES]
    assert got == RIGHT_EDGE_WRAPPED and 3 * sum(got) >= 12 * len(RIGHT_EDGE_CASES), got


def test_oracle_pinter_analyze_cu_matches_reference_goldens_in_the_last_ctu_of_an_8192_wide_picture():
    """tests/golden/inter_right_edge_v1.npz: CUs of 8 to 64 in the last CTU of an 8192 x 64 picture, B and P slices, neighbour vectors pointing up to 63 samples right --
    merge / skip candidates (through xeve_mv_clip), both lists' searches from predictors whose frame coordinate wraps, check_best_mvp, analyze_bi, the reconstruction"""
    n, modes = oracle_against(True)
    assert n == len(RIGHT_EDGE_CASES) and len(modes) >= 3, modes
