#!/usr/bin/env python3
"""What an even picture size that is no multiple of 8 costs on the device (xeve_amd/csrc/frames.hip): the padded load of the pushed frames and the cropped copy of the
reconstructed pictures, per picture of a batch, as bytes/s over their streams beside a device-to-device copy of the same OUTPUT bytes on the same device.
usage: probe_crop.py leaves [--sizes 1918x1078,3838x2158] [--frames 8] [--reps 10] [--memory-share 0.4]
           the two leaves on buffers of the encoder's geometry (originals of stride W, stores of stride W + 288 / W / 2 + 144, pictures stacked vh rows apart) with the
           GOPs plan_batches gives for the size -- fewer when `memory-share` of the free memory does not hold the probe's buffers --, HIP-event time over `reps` calls,
           the leaf and the copy alternated; one JSON line per size
       probe_crop.py encode [--sizes 1918x1078,1920x1080] [--gops 64]
           one I picture of `gops` GOPs at each size through the encoder with keep_recon: run it under a kernel trace to read the encoder's own kernels side by side --
           k_enc_load at the aligned size, k_frames_load / k_recon_crop at the cropped one"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e-3


def leaves(args):
    import torch

    import xeve_amd
    from xeve_amd import encode, lib

    xeve_amd.init(0)
    L, dev = lib.load(), torch.device("cuda:0")
    for size in args.sizes.split(","):
        sw, sh = (int(v) for v in size.split("x"))
        w, h = (sw + 7) & ~7, (sh + 7) & ~7
        cfg = encode.config(sw, sh, keyint=args.frames, closed_gop=True, threads=8, keep_recon=True, crop=True)
        free = torch.cuda.mem_get_info()[0]
        planned = encode.plan_batches(cfg, 1 << 20, args.frames, free, max_batches=1)[0][0][1]
        vh, s_l, s_c = (h + 288 + 63) & ~63, w + 288, w // 2 + 144
        org_l, org_c, pic_l, pic_c = vh * w, (vh // 2) * (w // 2), vh * s_l, (vh // 2) * s_c
        frame, kept = sw * sh * 3 // 2, sw * sh * 3 // 2
        per_gop = frame + 2 * (org_l + 2 * org_c) + 2 * (pic_l + 2 * pic_c) + 2 * kept + 4 * max(w * h * 3 // 2, kept)  # frames, originals, store, kept, the copy's two buffers
        G = int(max(1, min(planned, args.memory_share * free // per_gop, 65535)))
        frames = torch.randint(0, 256, (G * frame,), dtype=torch.uint8, device=dev)
        org = [torch.empty(G * n, dtype=torch.int16, device=dev) for n in (org_l, org_c, org_c)]
        store = [torch.randint(0, 1024, (G * n,), dtype=torch.int16, device=dev) for n in (pic_l, pic_c, pic_c)]
        out = torch.empty(G * kept, dtype=torch.int16, device=dev)
        src = torch.randint(0, 1024, (G * max(w * h * 3 // 2, kept),), dtype=torch.int16, device=dev)
        dst = torch.empty_like(src)
        p_org = (C.c_void_p * 3)(*[t.data_ptr() for t in org])
        p_rec = (C.c_void_p * 3)(org_base(store[0], 144 * s_l + 144), org_base(store[1], 72 * s_c + 72), org_base(store[2], 72 * s_c + 72))

        def load():
            lib.check(L.xeve_hip_frames_load(frames.data_ptr(), frame, 8, sw, sh, w, h, p_org, w, w // 2, org_l, org_c, G, None))

        def crop():
            lib.check(L.xeve_hip_recon_crop(p_rec, s_l, s_c, pic_l, pic_c, sw, sh, G, out.data_ptr(), kept, None))

        n_load, n_crop = G * w * h * 3 // 2, G * kept
        for fn in (load, crop, lambda: dst[:n_load].copy_(src[:n_load]), lambda: dst[:n_crop].copy_(src[:n_crop])):
            fn()  # warm
        torch.cuda.synchronize()
        t = {"load": [], "copy_load": [], "crop": [], "copy_crop": []}
        for _ in range(3):  # alternated
            t["load"].append(_timed(torch, load, args.reps)), t["copy_load"].append(_timed(torch, lambda: dst[:n_load].copy_(src[:n_load]), args.reps))
            t["crop"].append(_timed(torch, crop, args.reps)), t["copy_crop"].append(_timed(torch, lambda: dst[:n_crop].copy_(src[:n_crop]), args.reps))
        best = {k: min(v) for k, v in t.items()}
        bytes_load, bytes_crop = G * frame + 2 * n_load, 2 * 2 * n_crop  # read + written
        print(json.dumps({"size": size, "coded": [w, h], "gops": G, "gops_planned": planned, "reps": args.reps, "seconds": t,
                          "load_us_per_picture": best["load"] / G * 1e6, "load_GBps": bytes_load / best["load"] * 1e-9, "copy_of_load_output_GBps": 4 * n_load / best["copy_load"] * 1e-9,
                          "load_vs_copy_time": best["load"] / best["copy_load"],
                          "crop_us_per_picture": best["crop"] / G * 1e6, "crop_GBps": bytes_crop / best["crop"] * 1e-9, "copy_of_crop_output_GBps": 4 * n_crop / best["copy_crop"] * 1e-9,
                          "crop_vs_copy_time": best["crop"] / best["copy_crop"]}), flush=True)
        del frames, org, store, out, src, dst
        torch.cuda.empty_cache()


def org_base(t, lead):
    return t.data_ptr() + 2 * lead


def encode_once(args):
    import numpy as np

    import xeve_amd
    from xeve_amd import encode

    xeve_amd.init(0)
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        cfg = encode.config(w, h, keyint=8, closed_gop=True, threads=8, preset="fast", keep_recon=True, measure=True, crop=(w | h) & 7 != 0)
        enc = encode.BatchEncoder(cfg, args.gops, 1)
        frame = np.random.default_rng(1).integers(0, 256, size=enc.frame_bytes, dtype=np.uint8).tobytes()
        for g in range(args.gops):
            enc.push(g, 0, frame)
        streams = enc.encode()
        print(json.dumps({"size": size, "gops": args.gops, "bytes": len(streams[0]), "all_equal": len(set(streams)) == 1, "recon_bytes": len(enc.recon(0))}), flush=True)
        enc.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["leaves", "encode"])
    ap.add_argument("--sizes", default=None)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--gops", type=int, default=64)
    ap.add_argument("--memory-share", type=float, default=0.4)
    a = ap.parse_args()
    if a.sizes is None:
        a.sizes = "1918x1078,3838x2158" if a.mode == "leaves" else "1918x1078,1920x1080"
    leaves(a) if a.mode == "leaves" else encode_once(a)
