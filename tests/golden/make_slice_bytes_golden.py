#!/usr/bin/env python3
"""Writes tests/golden/slice_bytes_v1.json, or with the argument `binary` tests/golden/slice_bytes_binary_v1.json, from the UNMODIFIED reference application
(oracle/_ref/xeveb_app).  Build container only.
What a picture of i.i.d. noise costs at every QP the encoder accepts: seed-21 uniform noise or seed-9301 binary noise (every sample 0 or 255; tests/_e2e.py make_yuv),
128x64, --preset fast -I 1 -b 0, 2 frames, -q 0 .. 51; per q the bytes of each picture's slice NAL unit (header included) and the larger of the two per sample.  The binary
table also holds one low-delay run of two frames per q (-I 0 -b 0): the bytes of its I and of its inter picture with the slice QP the application reports for each --
what an inter picture costs whose references are as noisy as itself.  The device encoder's slice buffers are sized against both tables (xeve_amd/csrc/enc_plan.h
slice_capacity; tests/test_enc_batches.py)."""
import json
import os
import re
import struct
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _e2e import make_yuv  # noqa: E402
from _libs import REF_APP, ROOT  # noqa: E402
import subprocess  # noqa: E402

BINARY = sys.argv[1:] == ["binary"]
assert BINARY or not sys.argv[1:], sys.argv
W, H, FRAMES, SEED, CLI = 128, 64, 2, 9301 if BINARY else 21, ["--preset", "fast", "-I", "1", "-b", "0"]
LDB = ["--preset", "fast", "-I", "0", "-b", "0"]
out = {"w": W, "h": H, "frames": FRAMES, "seed": SEED, "cli": CLI, "samples_per_picture": W * H * 3 // 2, "per_q": []}
if BINARY:
    out["low_delay_cli"] = LDB


def run(yuv, evc, q, cli):
    """-> (bytes of every slice NAL unit, the slice QP the application reports per coded picture)"""
    cmd = [REF_APP, "-i", yuv, "-w", str(W), "-h", str(H), "-z", "30", "--frames", str(FRAMES), "-m", "1", "-v", "3", "-o", evc, "-q", str(q)] + cli
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, (cmd, p.stdout[-1500:], p.stderr[-1500:])
    data, pos, slices = open(evc, "rb").read(), 0, []
    while pos < len(data):  # the application's output: a 4-byte big-endian length in front of every NAL unit
        n = struct.unpack_from(">I", data, pos)[0]
        if ((data[pos + 4] >> 1) & 0x3F) - 1 in (0, 1):  # nal_unit_type_plus1: non-IDR and IDR slices
            slices.append(n)
        pos += 4 + n
    assert pos == len(data) and len(slices) == FRAMES, (q, slices)
    qps = []
    for line in p.stdout.replace("[ ", "\n[ ").split("\n"):  # (the picture table, as tests/golden/make_enc_golden.py reads it)
        m = re.search(r"(\d+)\s+(\d+)\s+\((.)\)\s+(\d+)\s+[\d.]+\s+[\d.]+\s+[\d.]+\s+\d+\s+\d+\s*(.*)$", line)
        if m and "frame/sec" not in m.group(0)[:m.start(3) - m.start(0)]:
            qps.append(int(m.group(4)))
    assert len(qps) == FRAMES, (q, p.stdout[-1500:])
    return slices, qps


with tempfile.TemporaryDirectory() as d:
    yuv, evc = os.path.join(d, "n.yuv"), os.path.join(d, "n.evc")
    make_yuv(yuv, W, H, FRAMES, SEED)
    for q in range(52):
        slices, qps = run(yuv, evc, q, CLI)
        assert qps == [q] * FRAMES, (q, qps)  # (all-intra: every slice QP is -q)
        row = {"q": q, "slice_bytes": slices, "bytes_per_sample": max(slices) / (W * H * 3 // 2)}
        if BINARY:
            row["low_delay_slice_bytes"], row["low_delay_slice_qp"] = run(yuv, evc, q, LDB)
        out["per_q"].append(row)
        print(row)
json.dump(out, open(os.path.join(ROOT, "tests", "golden", "slice_bytes_binary_v1.json" if BINARY else "slice_bytes_v1.json"), "w"), indent=1)
