"""Iterates tests/golden/me_v1.npz (results of the reference's own me_ipel_diamond) as case dicts."""
import os

import numpy as np

from _me_cases import PAD

ME_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "me_v1.npz")


def golden_cases():
    g = np.load(ME_GOLDEN)
    for t in (0, 1):
        org, ref = np.ascontiguousarray(g["org%d" % t]), np.ascontiguousarray(g["ref%d" % t])
        W, H = 128, 96
        for row, obi in zip(g["jobs%d" % t], g["org_bi%d" % t]):
            (S, bi, x, y, r0, r1, r2, r3, gx, gy, ix, iy, msr, sr, lam, fast, mot, bs_in, cost, mvx, mvy, beststep) = (int(v) for v in row)
            c = dict(org=org, ref=ref, s=W + 2 * PAD, x=x, y=y, S=S, bi=bi, min_clip=(-127, -127), max_clip=(W - 1, H - 1),
                     range=[r0, r1, r2, r3], gmvp=(gx, gy), mvi=(ix, iy), msr=msr, sr=sr, lambda_mv=lam, faststep=fast, mot_other=mot,
                     org_bi=np.ascontiguousarray(obi[:S * S]), beststep_in=bs_in)
            yield c, (cost, mvx, mvy, beststep)


def golden_spel_cases():
    g = np.load(ME_GOLDEN)
    for t in (0, 1):
        org, ref = np.ascontiguousarray(g["org%d" % t]), np.ascontiguousarray(g["ref%d" % t])
        W = 128
        for row, obi in zip(g["spel_jobs%d" % t], g["spel_org_bi%d" % t]):
            (S, bi, x, y, gx, gy, ix, iy, lam, mot, hc, qc, cost, mvx, mvy) = (int(v) for v in row)
            c = dict(org=org, ref=ref, s=W + 2 * PAD, x=x, y=y, S=S, bi=bi, gmvp=(gx, gy), mvi=(ix, iy), lambda_mv=lam, mot_other=mot,
                     org_bi=np.ascontiguousarray(obi[:S * S]), hpel_cnt=hc, qpel_cnt=qc)
            yield c, (cost, mvx, mvy)


ME_DEGENERATE_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "me_degenerate_v1.npz")


def golden_degenerate_cases():
    """tests/golden/me_degenerate_v1.npz (the reference's results where candidates tie and windows clip; make_me_degenerate_golden.py) ->
    (set key, bit depth, diamond case, (cost, mv x, mv y, beststep), (cost, mv x, mv y) of the 8 + 8 point sub-pel pattern around the case's centre,
    [(cost, mv x, mv y, mot_bits) of pinter_me_epzs per _me_cases.EPZS_VARIANTS])"""
    from _me_cases import EPZS_VARIANTS, GOLDEN_SETS

    g = np.load(ME_DEGENERATE_GOLDEN)
    W = H = 64
    for key, _, _, _ in GOLDEN_SETS:
        ref = np.ascontiguousarray(g["ref_" + key])
        org = np.zeros_like(ref)
        org[PAD:PAD + H, PAD:PAD + W] = g["org_" + key]  # (stored without its padding, which no search reads)
        for row, obi in zip(g["jobs_" + key], g["org_bi_" + key]):
            v = [int(t) for t in row]
            (bd, S, bi, x, y, r0, r1, r2, r3, gx, gy, ix, iy, msr, sr, lam, fast, mot, bs_in), rest = v[:19], v[19:]
            c = dict(org=org, ref=ref, s=W + 2 * PAD, x=x, y=y, S=S, bi=bi, min_clip=(-127, -127), max_clip=(W - 1, H - 1), range=[r0, r1, r2, r3], gmvp=(gx, gy),
                     mvi=(ix, iy), msr=msr, sr=sr, lambda_mv=lam, faststep=fast, mot_other=mot, org_bi=np.ascontiguousarray(obi[:S * S]), beststep_in=bs_in)
            assert len(rest) == 4 + 3 + 4 * len(EPZS_VARIANTS)
            yield key, bd, c, tuple(rest[:4]), tuple(rest[4:7]), [tuple(rest[7 + 4 * k:11 + 4 * k]) for k in range(len(EPZS_VARIANTS))]
