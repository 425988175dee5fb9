#!/usr/bin/env python3
"""Writes tests/golden/recon_v1.json from the UNMODIFIED reference application (oracle/_ref/xeveb_app ... -v 3 -r).  Build container only.
Per case of CASES (tests/_enc.py's tables), every GOP coded as a run of its own (--seek g * F --frames F), the golden holds
  "per_gop":  the md5 and size of the run's reconstruction file (-r: display order, cropped, planar Y U V, 16-bit little-endian samples at the codec's 10 bits);
  "pictures": per GOP and picture, in coding order, [frame, poc, type, tid, qp, bits, psnr_y, psnr_u, psnr_v] as the application prints them and "sse": the three sums
              of squared differences THIS script computes with numpy from the reconstruction file and the input at 10 bits;
  "whole":    for cases of several GOPs the md5 and size of the whole-sequence run's reconstruction file.
The golden checks itself while it is made: the bitstream of every run has the md5 enc_v1.json records (-r changes nothing); the application's PSNR formula on the
recorder's SSE gives every printed value within the print's rounding; bits / 8 sums to the bitstream's size; the per-GOP files concatenate to the whole-sequence file.
usage: make_recon_golden.py [case names ...] -- without arguments everything is (re)made."""
import json
import math
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _enc  # noqa: E402
from _e2e import make_yuv  # noqa: E402
from _enc import app_args_and_env, md5, widen10  # noqa: E402
from _libs import REF_APP, ROOT  # noqa: E402

RECON_GOLDEN = os.path.join(ROOT, "tests", "golden", "recon_v1.json")
CASES = ["gops_128x64_noise", "gops_128x128_moving_m2", "size_120x72_noise_3gops", "size_8x8_noise", "size_24x40_moving", "size_200x8_moving", "size_72x120_moving",
         "size_88x80_slow", "gops_128x64_10bit_m2"]
TABLES = dict(list(_enc.BATCH_CASES.items()) + list(_enc.PICTURE_SIZE_CASES.items()) + list(_enc.DEPTH10_CASES.items()))
ROW = re.compile(r"(\d+)\s+(\d+)\s+\((.)\)\s+(\d+)\s+([\d.]+)\s+([\d.]+)\s+([\d.]+)\s+(\d+)\s+(\d+)")
HALF_ULP = 0.5e-4  # of the four printed decimals


def psnr(sse, n):  # find_psnr_16bit at 10 bits
    return 100.0 if sse == 0 else abs(10 * math.log10(255 * 255 * 16 / (sse / n)))


def app(yuv, evc, rec, w, h, frames, cli, threads, seek=0):
    args, pin = app_args_and_env(cli)
    cmd = [REF_APP, "-i", yuv, "-w", str(w), "-h", str(h), "-z", "30", "--frames", str(frames), "-m", str(threads), "-v", "3", "-o", evc, "-r", rec] + args
    if seek:
        cmd += ["--seek", str(seek)]
    p = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **pin))
    assert p.returncode == 0, (cmd, p.stdout[-1500:], p.stderr[-2000:])
    rows = []
    for line in p.stdout.split("\n"):
        m = ROW.search(line)
        if m and "frame/sec" not in line:
            rows.append([int(m.group(1)), int(m.group(2)), m.group(3), int(m.group(4)), float(m.group(5)), float(m.group(6)), float(m.group(7)), int(m.group(8))])
    assert len(rows) == frames, (cmd, rows, p.stdout[-3000:])
    return rows


def planes(buf, w, h, frame):
    """the three planes of picture `frame` of a planar 4:2:0 file of 16-bit samples, as int64"""
    a = np.frombuffer(buf, dtype="<u2", count=w * h * 3 // 2, offset=frame * w * h * 3).astype(np.int64)
    return a[:w * h], a[w * h:w * h * 5 // 4], a[w * h * 5 // 4:]


only = sys.argv[1:]
out = json.load(open(RECON_GOLDEN)) if only and os.path.exists(RECON_GOLDEN) else {}
enc = _enc.golden()["batches"]
with tempfile.TemporaryDirectory() as d:
    for name in CASES:
        if only and name not in only:
            continue
        w, h, gops, frames, seed, cli, threads = TABLES[name]
        yuv, evc, rec = os.path.join(d, name + ".yuv"), os.path.join(d, name + ".evc"), os.path.join(d, name + "_rec.yuv")
        make_yuv(yuv, w, h, gops * frames, seed)
        data = open(yuv, "rb").read()
        if "-d" in cli:  # (the application reads 16-bit samples with -d 10 and hands them to the codec as they are)
            assert cli[cli.index("-d") + 1] == "10"
            org10 = widen10(data)
            open(yuv, "wb").write(org10)
        else:  # 8-bit input reaches the codec shifted up by two bits (imgb_cpy_conv_8b_to_16b)
            org10 = (np.frombuffer(data, dtype=np.uint8).astype("<u2") << 2).tobytes()
        per, pictures, joined = [], [], b""
        for g in range(gops):
            rows = app(yuv, evc, rec, w, h, frames, cli, threads, seek=g * frames)
            bits, r = open(evc, "rb").read(), open(rec, "rb").read()
            assert md5(bits) == enc[name]["per_gop"][g]["md5"], (name, g, "-r changed the bitstream")
            assert len(r) == frames * w * h * 3, (name, g, len(r))
            assert sorted(row[0] for row in rows) == list(range(frames)), (name, g, "a run of one closed GOP / one low-delay run: POC = display position")
            assert sum(row[7] for row in rows) == 8 * len(bits), (name, g, "Bits / 8 must sum to the bitstream's size")
            pics = []
            for poc, tid, typ, qp, py, pu, pv, nbits in rows:
                frame = poc
                sse = [int(((a - b) ** 2).sum()) for a, b in zip(planes(r, w, h, frame), planes(org10, w, h, g * frames + frame))]
                for s, n, printed in zip(sse, (w * h, w * h // 4, w * h // 4), (py, pu, pv)):
                    assert abs(psnr(s, n) - printed) <= HALF_ULP + 1e-9, (name, g, poc, s, psnr(s, n), printed)
                pics.append({"row": [frame, poc, typ, tid, qp, nbits, py, pu, pv], "sse": sse})
            per.append({"md5": md5(r), "bytes": len(r)})
            pictures.append(pics)
            joined += r
        out[name] = {"w": w, "h": h, "gops": gops, "frames": frames, "per_gop": per, "pictures": pictures}
        if gops > 1:
            app(yuv, evc, rec, w, h, gops * frames, cli, threads)
            r = open(rec, "rb").read()
            assert r == joined, (name, "the per-GOP reconstruction files must concatenate to the whole-sequence run's")
            assert md5(open(evc, "rb").read()) == enc[name]["whole"]["md5"], name
            out[name]["whole"] = {"md5": md5(r), "bytes": len(r)}
        print(name, per, out[name].get("whole"))
json.dump(out, open(RECON_GOLDEN, "w"), indent=None, separators=(",", ":"))
