#!/usr/bin/env python3
"""Writes tests/golden/me_degenerate_v1.npz: inputs and the results of the REFERENCE's static me_ipel_diamond, me_spel_pattern and pinter_me_epzs
(src_base/xeve_pinter.c, via oracle/ref_me_driver.c) on content where candidates tie and search windows clip: _me_cases.GOLDEN_SETS -- flat, periodic, outward and
static planes of 64x64 plus padding, two jobs for every S and bi, two families also at bit depth 8 and 12.  Build container only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _me_cases import EPZS_VARIANTS, GOLDEN_SETS, PAD, degenerate_golden_jobs, epzs_variant_of, spel_case_of  # noqa: E402
from test_me_oracle_vs_ref import run_ref, run_ref_epzs, run_ref_spel  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "me_degenerate_v1.npz")
d = {}
for key, _, _, _ in GOLDEN_SETS:
    pl, bd, cases = degenerate_golden_jobs(key)
    d["org_" + key], d["ref_" + key] = pl["org"][PAD:PAD + 64, PAD:PAD + 64], pl["ref"]  # (the searches read the original inside the picture only: its padding is not stored)
    rows, bis = [], []
    for c in cases:
        cost, mvx, mvy, beststep, _ = run_ref(c, bd)
        row = [bd, c["S"], c["bi"], c["x"], c["y"], *c["range"], *c["gmvp"], *c["mvi"], c["msr"], c["sr"], c["lambda_mv"], c["faststep"], c["mot_other"], c["beststep_in"],
               cost, mvx, mvy, beststep]
        row += run_ref_spel(spel_case_of(c), bd)[:3]
        for v in EPZS_VARIANTS:
            row += run_ref_epzs(epzs_variant_of(c, v), bd)
        rows.append(row)
        bis.append(np.pad(c["org_bi"], (0, 4096 - len(c["org_bi"]))))
    d["jobs_" + key] = np.array(rows, np.int64)
    d["org_bi_" + key] = np.array(bis, np.int16)
np.savez_compressed(OUT, **d)
print("wrote", OUT, os.path.getsize(OUT))
