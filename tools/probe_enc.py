#!/usr/bin/env python3
"""Times the batch encoder in chunks of lockstep steps (device fence after every chunk): where a picture's time goes -- the steps of the I picture, of the inter
picture, the picture ends.  usage: probe_enc.py --width W --height H --gops G --threads T --frames F --chunk N [--content noise|moving] [--preset P] [--hash]
--hash: the run makes the decoded-picture signatures (config(hash=True)); a picture's LAST step becomes a chunk of its own, so that chunk's wall time is one step plus
the picture's end (loop filter, the 3 * G MD5s, the second writer pass, padding -- the fence waits for both streams), and after the run the MD5 leaf alone is timed on a
store of the run's geometry: what one picture end adds, and the kernel's ns per 64-byte block of its longest (luma) message."""
import argparse
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--gops", type=int, default=4)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=25)
    ap.add_argument("--max-steps", type=int, default=0, help="stop after this many lockstep steps (0: the whole job)")
    ap.add_argument("--content", default="noise")
    ap.add_argument("--preset", default="medium", help="fast | medium | slow | placebo (slow and placebo run on the fused walk at any width)")
    ap.add_argument("--same-clip", action="store_true", help="every GOP codes the SAME frames: all bitstreams must come out equal -- a lockstep chain that goes wrong anywhere in the batch shows as a second md5")
    ap.add_argument("--prof-after", type=int, default=-1, help="switch the walk's in-kernel stage profile on once this many steps are done (e.g. a picture's steps: the inter picture alone)")
    ap.add_argument("--hash", action="store_true", help="code with the picture signatures and time what a picture end adds (see above)")
    ap.add_argument("--split-end", action="store_true", help="a picture's last step as a chunk of its own, as --hash does (the same run without the signatures, to compare)")
    a = ap.parse_args()
    import torch

    import xeve_amd
    from xeve_amd import encode

    xeve_amd.init(0)
    dev = torch.device("cuda", 0)
    W, H, F, G = a.width, a.height, a.frames, a.gops
    fb = W * H * 3 // 2
    cfg = encode.config(W, H, qp=32, keyint=8, bframes=15, closed_gop=True, preset=a.preset, threads=a.threads, hash=a.hash)
    t0 = time.perf_counter()
    enc = encode.BatchEncoder(cfg, G, F)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    same = None
    for g in range(G):
        if a.same_clip and same is not None:
            d = same
        elif a.content == "noise":
            d = torch.randint(0, 256, (fb * F,), dtype=torch.uint8, device=dev, generator=gen)
        else:  # a drifting gradient + 3 bits of noise (SURVEY.md 8d's structured input)
            parts = []
            for f in range(F):
                yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
                parts.append((((xx + 3 * f + g) * 2 + (yy + f) + torch.randint(0, 8, (H, W), device=dev, generator=gen)) & 255).to(torch.uint8).reshape(-1))
                yy, xx = torch.meshgrid(torch.arange(H // 2, device=dev), torch.arange(W // 2, device=dev), indexing="ij")
                parts.append((((xx + f) * 3 + yy + torch.randint(0, 4, (H // 2, W // 2), device=dev, generator=gen)) & 255).to(torch.uint8).reshape(-1))
                parts.append(((xx + (yy + 2 * f) * 2 + torch.randint(0, 4, (H // 2, W // 2), device=dev, generator=gen)) & 255).to(torch.uint8).reshape(-1))
            d = torch.cat(parts)
        same = d
        for f in range(F):
            enc.push(g, f, d[f * fb:(f + 1) * fb])
    print(json.dumps({"setup_s": round(time.perf_counter() - t0, 2)}), flush=True)
    enc.begin()
    total = enc.advance(0)
    per_pic = total // F
    done, left = 0, total
    while left > 0 and (a.max_steps == 0 or done < a.max_steps):
        n = min(a.chunk, per_pic - done % per_pic)  # (a chunk never crosses a picture's end: its last step carries the picture end)
        if (a.hash or a.split_end) and n > 1 and done % per_pic + n == per_pic:
            n -= 1
        if a.prof_after >= 0 and done >= a.prof_after and not os.environ.get("XEVE_HIP_WALK_PROF"):
            from xeve_amd import lib
            lib.load().xeve_hip_walk_prof_enable(1)
            os.environ["XEVE_HIP_WALK_PROF"] = "runtime"
        t = time.perf_counter()
        st0 = enc.stats()
        left = enc.advance(n)
        enc.sync()
        dt = time.perf_counter() - t
        st1 = enc.stats()
        done += n
        print(json.dumps({"steps": [done - n, done], "picture": (done - 1) // per_pic, "wall_ms_per_step": round(1e3 * dt / n, 2),
                          "host_issue_ms_per_step": round(1e3 * (st1["step_seconds"] - st0["step_seconds"]) / n, 2),
                          "picture_end_s": round(st1["picture_end_seconds"] - st0["picture_end_seconds"], 2)}), flush=True)
    if os.environ.get("XEVE_HIP_WALK_PROF"):
        from tools.probe_walk import prof
        rows = prof()
        tot = sum(r[1] for r in rows) or 1
        print("walk profile of team 0 over the whole run: %.0f cycles" % tot)
        for name, cyc, marks in sorted(rows, key=lambda r: -r[1]):
            if marks:
                print("  %-12s %6.2f %%  %12d cycles  %7d marks  %8.0f cycles/mark" % (name, 100.0 * cyc / tot, cyc, marks, cyc / marks))
    print(json.dumps({"total_steps": total, "per_picture": per_pic, "chains": G * min(a.threads, (H + 63) // 64), "stats": enc.stats(),
                      "bytes": [len(s) for s in enc.bitstreams()][:4] if left == 0 else None,
                      "md5_of_all": hashlib.md5(b"".join(enc.bitstreams())).hexdigest() if left == 0 else None,
                      "distinct_bitstreams": (lambda m: {"count": len(set(m)), "gops_that_differ_from_gop_0": [i for i, x in enumerate(m) if x != m[0]][:40]})([hashlib.md5(b).hexdigest() for b in enc.bitstreams()]) if left == 0 and a.same_clip else None}), flush=True)
    enc.close()
    if a.hash:
        print(json.dumps(time_md5_leaf(torch, dev, W, H, G)), flush=True)


def time_md5_leaf(torch, dev, W, H, G, reps=3):
    """xeve_hip_md5_planes over G stacked pictures laid out as the encoder's picture stores are (luma stride W + 288, chroma W / 2 + 144, pictures a multiple of 64 rows
    apart), the 3 * G jobs in the encoder's order (every luma plane, then every U, then every V): milliseconds per launch, and per 64-byte block of a luma message"""
    import ctypes as C

    import numpy as np

    from xeve_amd import lib

    L = lib.load()
    vh, s_l, s_c = (H + 288 + 63) & ~63, W + 288, W // 2 + 144
    pic_l, pic_c = vh * s_l, (vh // 2) * s_c
    store = torch.randint(0, 1024, (G * (pic_l + 2 * pic_c),), dtype=torch.int16, device=dev)
    jobs = np.zeros(3 * G, dtype=lib.MD5_JOB_DTYPE)
    for c in range(3):
        for g in range(G):
            off = 144 * s_l + 144 + g * pic_l if c == 0 else G * pic_l + (c - 1) * G * pic_c + 72 * s_c + 72 + g * pic_c
            jobs[c * G + g] = (off, s_c if c else s_l, W // 2 if c else W, H // 2 if c else H, 0)
    d_jobs = torch.from_numpy(jobs.view(np.uint8).copy()).to(dev)
    out = torch.zeros(3 * G * 16, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps + 1):
        t = time.perf_counter()
        lib.check(L.xeve_hip_md5_planes(C.c_void_p(store.data_ptr()), C.c_void_p(d_jobs.data_ptr()), 3 * G, C.c_void_p(out.data_ptr()), None))
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t))
    import hashlib

    plane = store[144 * s_l + 144:144 * s_l + 144 + (H - 1) * s_l + W].cpu().numpy()
    want = hashlib.md5(b"".join(plane[r * s_l:r * s_l + W].astype("<i2").tobytes() for r in range(H))).digest()
    blocks = W * H * 2 // 64
    return {"md5_leaf": {"jobs": 3 * G, "launch_ms": [round(x, 3) for x in ms[1:]], "first_launch_ms": round(ms[0], 3), "luma_blocks": blocks,
                         "ns_per_block": round(1e6 * min(ms[1:]) / blocks, 1), "gop0_luma_equals_hashlib": bytes(out[:16].cpu().numpy()) == want}}


if __name__ == "__main__":
    main()
