"""Iterator over tests/golden/inter_v1.npz (reference results of xeve_pinter_analyze_cu); pictures / states regenerated from the seed."""
import os

import numpy as np

from _inter_cases import make_inter_jobs, make_inter_params, make_inter_picture
from _libs import INTER_RESULT_DTYPE, SBAC_DTYPE, sbac_from_golden
from _rdo_cases import states

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inter_v1.npz")
N_JOBS = 20
# seed, w, h, bit depth, reference pictures per list, chroma_format_idc, slice type (0 B, 1 P), log2 CU size, skip_th
CASES = [(901, 128, 96, 10, 2, 1, 0, 3, 0.0), (902, 128, 96, 10, 2, 1, 0, 4, 0.0), (903, 128, 96, 10, 2, 1, 0, 5, 0.0), (904, 128, 128, 10, 2, 1, 0, 6, 0.0),
         (905, 128, 64, 10, 2, 1, 1, 4, 0.0), (906, 96, 64, 8, 1, 1, 0, 4, 0.0), (907, 64, 64, 10, 2, 0, 0, 3, 0.0), (908, 192, 128, 10, 3, 1, 0, 4, 0.0),
         (909, 128, 96, 10, 2, 1, 0, 4, 6.0), (910, 128, 128, 10, 4, 1, 1, 5, 0.0)]


# the same in the last CTU of an 8192 x 64 picture (tests/golden/inter_right_edge_v1.npz; `make_inter_golden.py right_edge`): every CU size, B and P slices, neighbour vectors
# pointing up to 63 samples right -- the frame coordinates of predictors and start vectors pass an s16 from x = 8136 on (CUs of 64 cannot get there: 4 * 8128 + 252)
GOLD_RIGHT_EDGE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inter_right_edge_v1.npz")
N_RIGHT_EDGE_JOBS = 12
RIGHT_EDGE_CASES = [(921, 8192, 64, 10, 1, 1, 0, 3, 0.0), (922, 8192, 64, 10, 2, 1, 0, 4, 0.0), (923, 8192, 64, 10, 1, 1, 0, 5, 0.0), (924, 8192, 64, 10, 1, 1, 0, 6, 0.0),
                    (925, 8192, 64, 10, 2, 1, 1, 3, 0.0), (926, 8192, 64, 10, 1, 1, 1, 4, 0.0), (927, 8192, 64, 10, 1, 1, 1, 5, 0.0)]


def case_inputs(case, right_edge=False):
    """pictures, coder states, parameters and jobs of one case, from its seed"""
    seed, w, h, bd, nref, idc, st_type, lw, skip_th = case
    r = np.random.default_rng(seed)
    refs, org = make_inter_picture(r, w, h, bd, nref, idc, st_type)
    st = states(r, 6)
    P = make_inter_params(r, lw, w, h, bd, nref, idc, st_type, refs, skip_th)
    if right_edge:
        from _inter_cases import RIGHT_EDGE_H, RIGHT_EDGE_W, make_right_edge_inter_jobs

        assert (w, h) == (RIGHT_EDGE_W, RIGHT_EDGE_H)
        jobs = make_right_edge_inter_jobs(r, N_RIGHT_EDGE_JOBS, 1 << lw, len(st), refs, st_type)
    else:
        jobs = make_inter_jobs(r, N_JOBS, w, h, 1 << lw, len(st), refs, st_type)
    return refs, org, st, P, jobs


def golden(right_edge=False, only=None):
    g = np.load(GOLD_RIGHT_EDGE if right_edge else GOLD)
    for k, case in enumerate(RIGHT_EDGE_CASES if right_edge else CASES):
        if only is not None and k != only:
            continue
        seed, w, h, bd, nref, idc, st_type, lw, skip_th = case
        refs, org, st, P, jobs = case_inputs(case, right_edge)
        assert bytes(P) == np.ascontiguousarray(g["params%d" % k]).tobytes() and jobs.tobytes() == np.ascontiguousarray(g["jobs%d" % k]).tobytes()
        yield dict(refs=refs, org=org, states=st, P=P, jobs=jobs, res=np.ascontiguousarray(g["res%d" % k]).view(INTER_RESULT_DTYPE),
                   best=sbac_from_golden(g["best%d" % k], st[jobs["sbac"]]), coef=[g["coef%d_%d" % (k, c)] for c in range(3)],
                   rec=[g["rec%d_%d" % (k, c)] for c in range(3)], idc=idc, lw=lw, slice_type=st_type)
