#!/usr/bin/env python3
"""What the surface scaler costs on the device (xeve_amd/csrc/scale.hip): xeve_hip_surface_to_yuv420 over a stack of decoder surfaces -- NV12 (8 bits) or P010 (10 bits in
the top bits of 16) with rows a pitch apart -- beside a device-to-device copy (tensor.copy_: one hipMemcpyAsync) that reads and writes the SAME NUMBER OF BYTES as the
leaf reads and writes together, on the same device in the same process.  Every call is timed on its own with HIP events; the median of `runs` calls after `warm` is reported.
usage: probe_scale.py [--cases nv12:3840x2160:1920x1080:64,p010:3840x2160:1280x720:64] [--runs 20] [--warm 3] [--pitch-pad 64]       one JSON line per case"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median_seconds(torch, fn, runs, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(times), min(times), max(times)


def main(args):
    import torch

    import xeve_amd
    from xeve_amd import encode, lib

    xeve_amd.init(0)
    L, dev = lib.load(), torch.device("cuda:0")
    for case in args.cases.split(","):
        fmt, src, dst, n = case.split(":")
        (sw, sh), (w, h), n = (int(v) for v in src.split("x")), (int(v) for v in dst.split("x")), int(n)
        depth, dtype = (8, torch.uint8) if fmt == "nv12" else (10, torch.int16)
        top = 256 if depth == 8 else 1024
        base_y = (torch.randint(0, top, (n, sh, sw + args.pitch_pad), device=dev) << (0 if depth == 8 else 6)).to(dtype)
        base_uv = (torch.randint(0, top, (n, sh // 2, sw // 2 + args.pitch_pad // 2, 2), device=dev) << (0 if depth == 8 else 6)).to(dtype)
        y, uv = base_y[:, :, :sw], base_uv[:, :, :sw // 2]
        s, _, _, _, _, keep = encode._surface(y, uv, depth > 8, True)
        per = w * h * 3 // 2
        out = torch.empty((n, per), dtype=dtype, device=dev)
        es = out.element_size()
        read, written = n * sw * sh * 3 // 2 * es, n * per * es
        half = (read + written) // 2  # a copy of this many bytes reads and writes read + written bytes in all
        a, b = torch.empty(half, dtype=torch.uint8, device=dev).random_(0, 256), torch.empty(half, dtype=torch.uint8, device=dev)

        def leaf():
            lib.check(L.xeve_hip_surface_to_yuv420(C.byref(s), sw, sh, 0, w, h, depth, n, out.data_ptr(), per * es, None))

        t_copy = _median_seconds(torch, lambda: b.copy_(a), args.runs, args.warm)
        t = _median_seconds(torch, leaf, args.runs, args.warm)
        print(json.dumps({"case": case, "median_ms": t[0] * 1e3, "min_ms": t[1] * 1e3, "max_ms": t[2] * 1e3, "us_per_picture": t[0] / n * 1e6, "bytes_read": read, "bytes_written": written,
                          "leaf_GBps": (read + written) / t[0] * 1e-9, "copy_bytes_each_way": half, "copy_median_ms": t_copy[0] * 1e3, "copy_GBps": 2 * half / t_copy[0] * 1e-9,
                          "leaf_vs_copy_time": t[0] / t_copy[0]}), flush=True)
        del base_y, base_uv, out, a, b
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="nv12:3840x2160:1920x1080:64,p010:3840x2160:1280x720:64")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--pitch-pad", type=int, default=64)
    main(ap.parse_args())
