#!/usr/bin/env python3
"""What the RGB front door costs on the device (xeve_amd/csrc/color.hip): xeve_hip_rgb_to_yuv420 (to 10-bit frames) and xeve_hip_yuv420_to_rgb over a stack of pictures,
for uint8 (N, H, W, 3) and float32 (N, 3, H, W) tensors, each beside a device-to-device copy (tensor.copy_: one hipMemcpyAsync) of the LARGER of its input and output on
the same device.  Every call is timed on its own with HIP events; the median of `runs` calls after `warm` is reported, with the bytes read and written per second.
usage: probe_rgb.py [--cases 1920x1080x64,3840x2160x8] [--runs 20] [--warm 3]       one JSON line per case, element type and direction"""
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
    col = lib.Color(1, 0, 0, 10)
    for case in args.cases.split(","):
        w, h, n = (int(v) for v in case.split("x"))
        per = w * h * 3 // 2
        yuv = torch.randint(0, 1024, (n, per), dtype=torch.int16, device=dev)
        for dtype, layout in ((torch.uint8, "hwc"), (torch.float32, "chw")):
            shape = (n, h, w, 3) if layout == "hwc" else (n, 3, h, w)
            rgb = torch.randint(0, 256, shape, dtype=torch.uint8, device=dev) if dtype == torch.uint8 else torch.rand(shape, dtype=dtype, device=dev)
            desc, _, _, _ = encode._rgb_desc(rgb, layout, True)
            rgb_bytes, yuv_bytes = rgb.numel() * rgb.element_size(), yuv.numel() * 2
            big = max(rgb_bytes, yuv_bytes)
            src = torch.empty(big, dtype=torch.uint8, device=dev).random_(0, 256)
            dst = torch.empty_like(src)

            def fwd():
                lib.check(L.xeve_hip_rgb_to_yuv420(rgb.data_ptr(), C.byref(desc), C.byref(col), w, h, n, yuv.data_ptr(), per * 2, None))

            def inv():
                lib.check(L.xeve_hip_yuv420_to_rgb(yuv.data_ptr(), per, C.byref(col), w, h, n, rgb.data_ptr(), C.byref(desc), None))

            t_copy = _median_seconds(torch, lambda: dst.copy_(src), args.runs, args.warm)
            for name, fn in (("rgb_to_yuv420", fwd), ("yuv420_to_rgb", inv)):
                t = _median_seconds(torch, fn, args.runs, args.warm)
                print(json.dumps({"case": case, "dtype": str(dtype).split(".")[1], "layout": layout, "leaf": name, "median_ms": t[0] * 1e3, "min_ms": t[1] * 1e3, "max_ms": t[2] * 1e3,
                                  "us_per_picture": t[0] / n * 1e6, "leaf_GBps": (rgb_bytes + yuv_bytes) / t[0] * 1e-9, "copy_bytes": big, "copy_median_ms": t_copy[0] * 1e3,
                                  "copy_GBps": 2 * big / t_copy[0] * 1e-9, "leaf_vs_copy_time": t[0] / t_copy[0]}), flush=True)
            del rgb, src, dst
            torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1920x1080x64,3840x2160x8")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    main(ap.parse_args())
