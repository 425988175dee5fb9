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


ME_RIGHT_EDGE_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "me_right_edge_v1.npz")
RIGHT_EDGE_INPUTS = 27


def golden_right_edge_cases():
    """tests/golden/me_right_edge_v1.npz (the reference's results in the last CTU column of an 8192-wide picture; make_me_right_edge_golden.py) -> per job
    ((S, bi, preset), index in the launch, diamond case, dict of results): dia (cost, mv x, mv y, beststep); spel / spel_at_dia (cost, mv x, mv y) of the sub-pel pattern
    around the true motion / around the diamond's result; epzs / epzs_ipel (cost, mv x, mv y, mot_bits) of pinter_me_epzs with the preset's sub-pel pattern / with the
    integer refinement; twin_dia, twin_epzs: the same search 256 samples further left, where nothing wraps.  The planes are rebuilt from their closed form and held to
    the recorded CRCs, every job's inputs to the recorded row."""
    from _me_cases import RE_LAUNCHES, RE_PRESETS, right_edge_crc, right_edge_jobs

    g = np.load(ME_RIGHT_EDGE_GOLDEN)
    assert right_edge_crc() == [int(v) for v in g["crc"]], "the planes of the right-edge family are not the ones the fixture was recorded on"
    rows = iter(g["jobs"])
    for S, bi, preset in RE_LAUNCHES:
        for t, c in enumerate(right_edge_jobs(S, bi, preset)):
            v = [int(e) for e in next(rows)]
            assert v[:RIGHT_EDGE_INPUTS] == [S, bi, list(RE_PRESETS).index(preset), t, c["x"], c["y"], *c["range"], *c["gmvp"], *c["mvi"], *c["mvp"], *c["mv0"], c["msr"], c["sr"],
                                             c["lambda_mv"], c["faststep"], c["mot_other"], c["beststep_in"], c["hpel_cnt"], c["qpel_cnt"], c["raster"]], (S, bi, preset, t)
            r = v[RIGHT_EDGE_INPUTS:]
            assert len(r) == 26
            yield (S, bi, preset), t, c, dict(dia=tuple(r[0:4]), spel=tuple(r[4:7]), spel_at_dia=tuple(r[7:10]), epzs=tuple(r[10:14]), epzs_ipel=tuple(r[14:18]),
                                              twin_dia=tuple(r[18:22]), twin_epzs=tuple(r[22:26]))
    assert next(rows, None) is None
