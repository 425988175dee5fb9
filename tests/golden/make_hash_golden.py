#!/usr/bin/env python3
"""Writes tests/golden/hash_v1.json from the UNMODIFIED reference application (oracle/_ref/xeveb_app ... --hash -v 3 -r).  Build container only.
Per case of make_recon_golden.py's CASES, every GOP coded as a run of its own (--seek g * F --frames F), the golden holds
  "per_gop":  the md5 and size of the run's bitstream WITH the picture-signature SEI units;
  "pictures": per GOP and picture, in coding order, {"frame", "tid", "md5": [Y, U, V] as hex, "unit": the 56-byte signature NAL unit as hex};
  "whole":    for cases of several GOPs the md5 and size of the whole-sequence run's bitstream;
  "stream":   for size_8x8_noise the complete bitstream of GOP 0 as hex (under 2 KB).
The golden checks itself while it is made: every digest in the stream is hashlib.md5 of the corresponding plane of the -r file; every signature unit is 56 bytes,
sits right behind its picture's slice NAL unit and carries the picture's temporal id; the -r file has recon_v1.json's md5 (--hash changes no sample); with the signature
units taken out and hash=1 put back to hash=0 the bitstream has enc_v1.json's md5; the table's rows -- Bits included -- are recon_v1.json's; the per-GOP bitstreams
concatenate to the whole-sequence run's.
usage: make_hash_golden.py [case names ...] -- without arguments everything is (re)made."""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _enc  # noqa: E402
from _e2e import make_yuv  # noqa: E402
from _enc import app_args_and_env, md5, widen10  # noqa: E402
from _libs import REF_APP, ROOT  # noqa: E402

HASH_GOLDEN = os.path.join(ROOT, "tests", "golden", "hash_v1.json")
RECON_GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "recon_v1.json")))
CASES = ["gops_128x64_noise", "gops_128x128_moving_m2", "size_120x72_noise_3gops", "size_8x8_noise", "size_24x40_moving", "size_200x8_moving", "size_72x120_moving",
         "size_88x80_slow", "gops_128x64_10bit_m2"]
TABLES = dict(list(_enc.BATCH_CASES.items()) + list(_enc.PICTURE_SIZE_CASES.items()) + list(_enc.DEPTH10_CASES.items()))
ROW = re.compile(r"(\d+)\s+(\d+)\s+\((.)\)\s+(\d+)\s+([\d.]+)\s+([\d.]+)\s+([\d.]+)\s+(\d+)\s+(\d+)")
NUT_SEI, SLICE_NUTS = 28, (0, 1)


def app(yuv, evc, rec, w, h, frames, cli, threads, seek=0):
    args, pin = app_args_and_env(cli)
    cmd = [REF_APP, "-i", yuv, "-w", str(w), "-h", str(h), "-z", "30", "--frames", str(frames), "-m", str(threads), "-v", "3", "-o", evc, "-r", rec, "--hash"] + args
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


def units(bits):
    """[(offset, whole unit with its length field, nal unit type, temporal id)]"""
    out, at = [], 0
    while at < len(bits):
        size = int.from_bytes(bits[at:at + 4], "big")
        head = int.from_bytes(bits[at + 4:at + 6], "big")
        assert size >= 2 and at + 4 + size <= len(bits), (at, size, len(bits))
        out.append((at, bits[at:at + 4 + size], ((head >> 9) & 0x3F) - 1, (head >> 6) & 7))
        at += 4 + size
    return out


def plane_md5s(rec, w, h, frame):
    n, at = w * h * 2, frame * w * h * 3
    return [hashlib.md5(rec[at:at + n]).hexdigest(), hashlib.md5(rec[at + n:at + n + n // 4]).hexdigest(), hashlib.md5(rec[at + n + n // 4:at + n + n // 2]).hexdigest()]


def signatures(bits, rec, rows, w, h, where):
    """the signature units of one run, checked against the run's -r file and table; returns (the golden's picture records, the bitstream without the units)"""
    pics, plain, prev = [], b"", None
    for at, unit, nut, tid in units(bits):
        if nut == NUT_SEI and unit[6:8] == b"\x10\x10":
            assert len(unit) == 56 and unit[:4] == bytes([0, 0, 0, 0x34]), (where, at, len(unit))
            assert prev is not None and prev[0] in SLICE_NUTS and prev[1] == tid, (where, at, "a signature unit follows its picture's slice unit at the same temporal id")
            poc, row_tid = rows[len(pics)][0], rows[len(pics)][1]
            digests = [unit[8 + 16 * c:24 + 16 * c].hex() for c in range(3)]
            assert row_tid == tid and digests == plane_md5s(rec, w, h, poc), (where, at, poc, digests)
            pics.append({"frame": poc, "tid": tid, "md5": digests, "unit": unit.hex()})
        else:
            plain += unit
        prev = (nut, tid)
    assert len(pics) == len(rows), (where, len(pics))
    assert plain.count(b" hash=1 ") == 1, where
    return pics, plain.replace(b" hash=1 ", b" hash=0 ")


only = sys.argv[1:]
out = json.load(open(HASH_GOLDEN)) if only and os.path.exists(HASH_GOLDEN) else {}
enc = _enc.golden()["batches"]
with tempfile.TemporaryDirectory() as d:
    for name in CASES:
        if only and name not in only:
            continue
        w, h, gops, frames, seed, cli, threads = TABLES[name]
        yuv, evc, rec = os.path.join(d, name + ".yuv"), os.path.join(d, name + ".evc"), os.path.join(d, name + "_rec.yuv")
        make_yuv(yuv, w, h, gops * frames, seed)
        if "-d" in cli:  # (the application reads 16-bit samples with -d 10 and hands them to the codec as they are)
            assert cli[cli.index("-d") + 1] == "10"
            data = widen10(open(yuv, "rb").read())
            open(yuv, "wb").write(data)
        want = RECON_GOLDEN[name]
        per, pictures, joined = [], [], b""
        for g in range(gops):
            rows = app(yuv, evc, rec, w, h, frames, cli, threads, seek=g * frames)
            bits, r = open(evc, "rb").read(), open(rec, "rb").read()
            assert (md5(r), len(r)) == (want["per_gop"][g]["md5"], want["per_gop"][g]["bytes"]), (name, g, "--hash changed the reconstruction")
            for row, p in zip(rows, want["pictures"][g]):  # POC Tid Ftype QP PSNR-Y PSNR-U PSNR-V Bits: the signature unit is not counted
                frame, poc, typ, tid, qp, nbits, py, pu, pv = p["row"]
                assert row == [poc, tid, typ, qp, py, pu, pv, nbits], (name, g, row, p["row"])
            pics, plain = signatures(bits, r, rows, w, h, (name, g))
            assert (md5(plain), len(plain)) == (enc[name]["per_gop"][g]["md5"], enc[name]["per_gop"][g]["bytes"]), (name, g, "without the signatures the bitstream is the plain run's")
            assert len(bits) == len(plain) + 56 * frames and sum(row[7] for row in rows) == 8 * len(plain), (name, g)
            per.append({"md5": md5(bits), "bytes": len(bits)})
            pictures.append(pics)
            joined += bits
        out[name] = {"w": w, "h": h, "gops": gops, "frames": frames, "per_gop": per, "pictures": pictures}
        if gops > 1:
            app(yuv, evc, rec, w, h, gops * frames, cli, threads)
            bits = open(evc, "rb").read()
            assert bits == joined, (name, "the per-GOP bitstreams must concatenate to the whole-sequence run's")
            assert md5(open(rec, "rb").read()) == want["whole"]["md5"], name
            out[name]["whole"] = {"md5": md5(bits), "bytes": len(bits)}
        if name == "size_8x8_noise":
            assert len(joined) < 2048
            out[name]["stream"] = joined.hex()
        print(name, per, out[name].get("whole"))
json.dump(out, open(HASH_GOLDEN, "w"), indent=None, separators=(",", ":"))
