#!/usr/bin/env python3
"""Writes tests/golden/crop_v1.json from the UNMODIFIED reference application (oracle/_ref/xeveb_app ... -v 3 -r [--hash]).  Build container only.
The cases are tests/_crop.py CASES: picture sizes that are even but no multiple of 8, which the reference codes at ALIGN8 of both directions with a cropping window in
the SPS.  Every GOP is coded as a run of its own (--seek g * F --frames F) and the whole clip once more as one run; the golden holds per case
  "per_gop":  the md5 and size of each run's bitstream;         "whole": the same of the whole-sequence run (= the per-GOP bitstreams joined);
  "pictures": per GOP and picture, in coding order, {"row": [frame, poc, type, tid, qp, bits, psnr_y, psnr_u, psnr_v]} as the application prints them.  The PSNRs run
              over the CODED planes, zero padding included, so they cannot be recomputed from the cropped -r file: only the printed values are recorded;
  "recon":    {"per_gop": [...], "whole": ...}: the md5 and size of the -r files (display order, CROPPED to w x h, planar Y U V, 16-bit samples at the codec's 10 bits);
  "hash":     for _crop.HASH_CASE the same runs with --hash: {"per_gop", "whole"} of the bitstreams with the picture-signature SEI units and "pictures": per GOP and
              picture in coding order {"frame", "tid", "md5": [Y, U, V]} read from those units.  The digests are over the CODED planes (xeve_md5_imgb hashes the aligned
              size): they are NOT the md5 of the -r file's planes, and nothing here checks them against it.
The golden checks itself while it is made: every run is made twice and gives the same bytes; the -r file is frames * w * h * 3 bytes; Bits / 8 sums to the bitstream's
size; the SPS carries the aligned size and the cropping offsets; the per-GOP files join to the whole-sequence run's; with --hash the -r file and the table stay what they
were, and without the signature units and with hash=1 put back to hash=0 the bitstream is the plain run's.
crop_2x2: the reference codes it (an 8x8 picture of which one luma 2x2 and one chroma sample per plane are input); were it ever refused, 2x10 / 10x2 would stand in.
usage: make_crop_golden.py [case names ...] -- without arguments everything is (re)made."""
import json
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _crop  # noqa: E402
from _enc import app_args_and_env, md5  # noqa: E402
from _libs import REF_APP  # noqa: E402

ROW = re.compile(r"(\d+)\s+(\d+)\s+\((.)\)\s+(\d+)\s+([\d.]+)\s+([\d.]+)\s+([\d.]+)\s+(\d+)\s+(\d+)")
NUT_SPS, NUT_SEI = 24, 28


def app(yuv, evc, rec, w, h, frames, cli, threads, seek=0, extra=()):
    args, pin = app_args_and_env(cli)
    cmd = [REF_APP, "-i", yuv, "-w", str(w), "-h", str(h), "-z", "30", "--frames", str(frames), "-m", str(threads), "-v", "3", "-o", evc, "-r", rec] + args + list(extra)
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
    return rows, open(evc, "rb").read(), open(rec, "rb").read()


def units(bits):
    """[(whole unit with its length field, nal unit type, temporal id)]"""
    out, at = [], 0
    while at < len(bits):
        size = int.from_bytes(bits[at:at + 4], "big")
        head = int.from_bytes(bits[at + 4:at + 6], "big")
        assert size >= 2 and at + 4 + size <= len(bits), (at, size, len(bits))
        out.append((bits[at:at + 4 + size], ((head >> 9) & 0x3F) - 1, (head >> 6) & 7))
        at += 4 + size
    return out


class BitReader:
    def __init__(self, data):
        self.d, self.at = data, 0

    def u(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | ((self.d[self.at >> 3] >> (7 - (self.at & 7))) & 1)
            self.at += 1
        return v

    def ue(self):
        z = 0
        while self.u(1) == 0:
            z += 1
        return (1 << z) - 1 + (self.u(z) if z else 0)


def sps_size_and_crop(bits):
    """(coded width, coded height, cropping flag, [left, right, top, bottom]) of the bitstream's first SPS (Baseline: xeve_eco_sps with every tool flag 0)"""
    payload = [u for u, nut, _ in units(bits) if nut == NUT_SPS][0][6:]
    r = BitReader(payload)
    r.ue(), r.u(8), r.u(8), r.u(32), r.u(32)  # sps id, profile, level, toolset_idc_h / _l
    assert r.ue() == 1  # 4:2:0
    w, h = r.ue(), r.ue()
    r.ue(), r.ue(), r.u(13)  # bit depths, the tool flags
    if r.ue() == 0:  # log2_sub_gop_length
        r.ue()  # log2_ref_pic_gap_length
    r.ue()  # max_num_ref_pics
    flag = r.u(1)
    return w, h, flag, [r.ue() for _ in range(4)] if flag else [0, 0, 0, 0]


def twice(*a, **k):
    one, two = app(*a, **k), app(*a, **k)
    assert one == two, (a, "the reference gives different output on two runs")
    return one


only = sys.argv[1:]
out = json.load(open(_crop.GOLDEN_PATH)) if only and os.path.exists(_crop.GOLDEN_PATH) else {}
with tempfile.TemporaryDirectory() as d:
    for name, (w, h, gops, frames, seed, cli, threads) in _crop.CASES.items():
        if only and name not in only:
            continue
        yuv, _ = _crop.clip(d, name)
        evc, rec = os.path.join(d, name + ".evc"), os.path.join(d, name + "_rec.yuv")
        W, H = _crop.align8(w), _crop.align8(h)
        per, rper, pictures, joined, rjoined, plain_runs = [], [], [], b"", b"", []
        for g in range(gops):
            rows, bits, r = twice(yuv, evc, rec, w, h, frames, cli, threads, seek=g * frames)
            assert len(r) == frames * w * h * 3, (name, g, len(r))
            assert sorted(row[0] for row in rows) == list(range(frames)), (name, g, "a run of one closed GOP: POC = display position")
            assert sum(row[7] for row in rows) == 8 * len(bits), (name, g, "Bits / 8 must sum to the bitstream's size")
            assert sps_size_and_crop(bits) == (W, H, 1, [0, (W - w + 1) >> 1, 0, (H - h + 1) >> 1]), (name, g, sps_size_and_crop(bits))
            per.append({"md5": md5(bits), "bytes": len(bits)}), rper.append({"md5": md5(r), "bytes": len(r)})
            pictures.append([{"row": [poc, poc, typ, tid, qp, nbits, py, pu, pv]} for poc, tid, typ, qp, py, pu, pv, nbits in rows])
            joined += bits
            rjoined += r
            plain_runs.append((rows, bits, r))
        _, bits, r = twice(yuv, evc, rec, w, h, gops * frames, cli, threads)
        assert bits == joined and r == rjoined, (name, "the per-GOP files must concatenate to the whole-sequence run's")
        out[name] = {"w": w, "h": h, "coded": [W, H], "gops": gops, "frames": frames, "seed": seed, "options": cli, "threads": threads, "per_gop": per,
                     "whole": {"md5": md5(bits), "bytes": len(bits)}, "pictures": pictures, "recon": {"per_gop": rper, "whole": {"md5": md5(r), "bytes": len(r)}}}
        if name == _crop.HASH_CASE:
            hper, hpics, hjoined = [], [], b""
            for g in range(gops):
                rows, bits, r = twice(yuv, evc, rec, w, h, frames, cli, threads, seek=g * frames, extra=["--hash"])
                prows, pbits, pr = plain_runs[g]
                assert rows == prows and r == pr, (name, g, "--hash changed the table or the reconstruction")
                pics, plain, prev = [], b"", None
                for unit, nut, tid in units(bits):
                    if nut == NUT_SEI and unit[6:8] == b"\x10\x10":
                        assert len(unit) == 56 and prev is not None and prev[0] in (0, 1) and prev[1] == tid, (name, g, "a signature unit follows its picture's slice unit")
                        assert rows[len(pics)][1] == tid, (name, g)
                        pics.append({"frame": rows[len(pics)][0], "tid": tid, "md5": [unit[8 + 16 * c:24 + 16 * c].hex() for c in range(3)]})
                    else:
                        plain += unit
                    prev = (nut, tid)
                assert len(pics) == frames and plain.count(b" hash=1 ") == 1 and plain.replace(b" hash=1 ", b" hash=0 ") == pbits, (name, g)
                hper.append({"md5": md5(bits), "bytes": len(bits)}), hpics.append(pics)
                hjoined += bits
            _, bits, _ = twice(yuv, evc, rec, w, h, gops * frames, cli, threads, extra=["--hash"])
            assert bits == hjoined, name
            out[name]["hash"] = {"per_gop": hper, "whole": {"md5": md5(bits), "bytes": len(bits)}, "pictures": hpics}
        print(name, per, rper)
json.dump(out, open(_crop.GOLDEN_PATH, "w"), indent=None, separators=(",", ":"))
