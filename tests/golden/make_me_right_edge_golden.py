#!/usr/bin/env python3
"""Writes tests/golden/me_right_edge_v1.npz: the results of the REFERENCE's static me_ipel_diamond, me_spel_pattern and pinter_me_epzs (src_base/xeve_pinter.c, via
oracle/ref_me_driver.c) in the last CTU column of an 8192-wide picture, where quarter-pel frame coordinates pass an s16: _me_cases.RE_LAUNCHES, five jobs each, and
each job's twin 256 samples further left, where nothing wraps.  The planes are closed-form integer textures: the file holds their CRCs, not the samples.  Build
container only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _me_cases import RE_LAUNCHES, RE_PRESETS, right_edge_crc, right_edge_epzs_case, right_edge_jobs, right_edge_spel_case  # noqa: E402
from test_me_oracle_vs_ref import run_ref, run_ref_epzs, run_ref_spel  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "me_right_edge_v1.npz")
rows = []
for S, bi, preset in RE_LAUNCHES:
    for t, (c, w) in enumerate(zip(right_edge_jobs(S, bi, preset), right_edge_jobs(S, bi, preset, twin=True))):
        row = [S, bi, list(RE_PRESETS).index(preset), t, c["x"], c["y"], *c["range"], *c["gmvp"], *c["mvi"], *c["mvp"], *c["mv0"], c["msr"], c["sr"], c["lambda_mv"],
               c["faststep"], c["mot_other"], c["beststep_in"], c["hpel_cnt"], c["qpel_cnt"], c["raster"]]
        dia = run_ref(c)
        row += dia[:4]
        row += run_ref_spel(right_edge_spel_case(c))[:3]
        row += run_ref_spel(right_edge_spel_case(c, (dia[1], dia[2])))[:3]
        row += run_ref_epzs(right_edge_epzs_case(c))
        row += run_ref_epzs(right_edge_epzs_case(c, ipel=True))
        row += run_ref(w)[:4]
        row += run_ref_epzs(right_edge_epzs_case(w))
        rows.append(row)
np.savez_compressed(OUT, jobs=np.array(rows, np.int64), crc=np.array(right_edge_crc(), np.int64))
print("wrote", OUT, os.path.getsize(OUT), len(rows))
