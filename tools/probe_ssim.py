#!/usr/bin/env python3
"""What the SSIM kernel costs on the device (xeve_amd/csrc/ssim.hip): xeve_hip_ssim_planes over a stack of pictures on the encoder's geometry (stores w + 288 / w / 2 + 144
wide, originals w / w / 2) beside xeve_hip_recon_measure in sums-only mode over THE SAME PLANES in the same process -- the project's kernel that reads the same bytes.
Every call (its memset and its two launches) is timed on its own with HIP events, the two alternating; the median of `runs` calls after `warm` is reported.
usage: probe_ssim.py [--cases 1920x1080:64,3840x2160:64] [--runs 20] [--warm 3]       one JSON line per case"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3


def main(args):
    import torch

    import xeve_amd
    from xeve_amd import lib

    xeve_amd.init(0)
    L, dev = lib.load(), torch.device("cuda:0")
    for case in args.cases.split(","):
        size, n = case.split(":")
        (w, h), n = (int(v) for v in size.split("x")), int(n)
        wl = (w + 7) & ~7
        s_rec, s_org = (wl + 288, wl // 2 + 144), (wl, wl // 2)
        org = [torch.randint(0, 1024, (n, ph, s), device=dev, dtype=torch.int16) for ph, s in ((h, s_org[0]), (h // 2, s_org[1]), (h // 2, s_org[1]))]
        rec = []
        for c, (ph, s) in enumerate(((h, s_rec[0]), (h // 2, s_rec[1]), (h // 2, s_rec[1]))):  # a reconstruction a few steps off the original
            t = torch.randint(0, 1024, (n, ph, s), device=dev, dtype=torch.int16)
            pw = org[c].shape[2]
            t[:, :, :pw] = (org[c] + torch.randint(-6, 7, org[c].shape, device=dev, dtype=torch.int16)).clamp_(0, 1023)
            rec.append(t)
        pr, po = (C.c_void_p * 3)(*[t.data_ptr() for t in rec]), (C.c_void_p * 3)(*[t.data_ptr() for t in org])
        dr, do = (h * s_rec[0], h // 2 * s_rec[1]), (h * s_org[0], h // 2 * s_org[1])
        q, sse = torch.zeros((n, 3), dtype=torch.int64, device=dev), torch.zeros((n, 3), dtype=torch.int64, device=dev)
        wm, hm = w & ~7, h & ~7  # (the yardstick takes multiples of 8)

        def ssim():
            lib.check(L.xeve_hip_ssim_planes(pr, s_rec[0], s_rec[1], dr[0], dr[1], po, s_org[0], s_org[1], do[0], do[1], w, h, n, q.data_ptr(), None))

        def measure():
            lib.check(L.xeve_hip_recon_measure(pr, s_rec[0], s_rec[1], dr[0], dr[1], po, s_org[0], s_org[1], do[0], do[1], wm, hm, n, None, 0, sse.data_ptr(), None))

        for _ in range(args.warm):
            ssim(), measure()
        torch.cuda.synchronize()
        ts, tm = [], []
        for _ in range(args.runs):
            ts.append(_timed(torch, ssim)), tm.append(_timed(torch, measure))
        ms, mm = statistics.median(ts), statistics.median(tm)
        read = n * w * h * 3 // 2 * 2 * 2  # both operands' windows, 2 bytes a sample
        windows = sum(((pw >> 2) - 1) * ((ph >> 2) - 1) for pw, ph in ((w, h), (w // 2, h // 2), (w // 2, h // 2)))
        mean = (q.double().sum(dim=0) / (n * 2.0 ** 30)).cpu().tolist()
        print(json.dumps({"case": case, "ssim_median_ms": ms * 1e3, "ssim_min_ms": min(ts) * 1e3, "ssim_max_ms": max(ts) * 1e3, "measure_median_ms": mm * 1e3, "measure_min_ms": min(tm) * 1e3,
                          "measure_max_ms": max(tm) * 1e3, "ssim_vs_measure_time": ms / mm, "bytes_read": read, "ssim_GBps": read / ms * 1e-9, "measure_GBps": read / mm * 1e-9,
                          "windows_per_picture": windows, "us_per_picture": ms / n * 1e6,
                          "mean_ssim_yuv": [m / k for m, k in zip(mean, (((w >> 2) - 1) * ((h >> 2) - 1), ((w >> 3) - 1) * ((h >> 3) - 1), ((w >> 3) - 1) * ((h >> 3) - 1)))]}), flush=True)
        del org, rec, q, sse
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1920x1080:64,3840x2160:64")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    main(ap.parse_args())
