#!/usr/bin/env python3
"""bench.py -- encoded frames/s of the closed-GOP batch encoder on MI355X (3840x2160 Baseline preset medium, FULL `-I 8` closed GOPs), next to the reference encoder on the host.

    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

THE JOB (per GPU) is a real encode: independent closed GOPs of F = 8 frames each (1 IDR + 7 hierarchical B pictures: what `xeveb_app --preset medium --closed-gop -I 8 -m 8`
codes), in --batches batches side by side (a batch ends at 2^32 original samples; the others as large as HBM still allows), of synthetic i.i.d. uniform 8-bit 4:2:0 frames
resident in HBM before the clock starts, coded by xeve_hip_enc_* (include/xeve_hip.h): CTU mode decision (quad-tree, intra + inter analysis with motion search, RDOQ,
CABAC bit counts -- the composed walk's ~7 000 / ~11 000 launches per lockstep CTU step of an I / B picture on two streams (tree.hip; the library's choice at every width
since round 6), ONE fused kernel per step with --walk fused or presets slow / placebo: xeve_amd/csrc/walk.h), entropy writer, loop filter, second writer pass, padding, parameter sets + SEI + slice NAL units.  Sixty-four GOPs (--seeded) spread over every batch of rank 0 (its first and last among them) are the reference's own seed-4 input.

BOUNDED.  A whole 8-frame 3840x2160 job is 8 x 302 lockstep steps of a few hundred ms each whatever the batch size (a CTU's mode decision is a serial chain; the width is in
the GOPs) -- a quarter of an hour.  The bench therefore runs the job's first W + K bench steps and stops.

A STEP.  One bench step is a fixed share of the job: step_ctus() lockstep CTU steps, 3/25 of a picture's (36 at 3840x2160), whatever --steps and --warmup say.  The first W
steps are the untimed warm-up, the K others are timed between device fences + barriers; `ms_per_step` = the timed seconds / K.  `value` = frames coded inside the timed steps
(GOPs x the timed share of a picture's steps) / the timed seconds, over all ranks.  With the driver's K = 20, W = 5 the timed region is the last 40 % of the IDR picture and
almost two whole B pictures (IDR share 17 %; 12.5 % in a whole GOP, and an IDR step is the cheaper one: the figure is within a few per cent of the whole-GOP rate,
`config.timed_picture_mix` says exactly what was timed).  W + K may not run past the end of the GOP (67 steps at 3840x2160).  Every rank encodes its own GOPs ("weak"); no
collective in the data path.

A plain run does only that and prints the line (metric, value, unit, ms_per_step, dtype, config, encode).  --dump-outputs DIR runs the job on, untimed, to the end of the
picture the timed steps left part way and writes what they produced (dump_outputs(): the GOPs' bitstreams) as DIR/*.npy; the inputs are the same from run to run.

--full adds, after the timed steps, the job run on (untimed) to the end of picture --pictures (default 3: the IDR picture and the first two B pictures), GOP 0's bitstream
checked byte for byte against the PREFIX of the reference's bitstream that ends with the same picture (tests/golden/cfg4_8f_v1.json, recorded from the unmodified reference
application; the WHOLE 8-frame GOP is pinned by tests/test_enc_gpu.py on the same library; --pictures 0 runs the whole GOP), and the extras below.

With --full the JSON line also carries
  roofline     : the SAD kernel of the path = k_me_epzs (composed walk; with the fused walk k_walk, the whole CTU mode decision of a step in one launch): the motion search's
                 SAD work (sample pairs counted on the device) over the kernel's HIP-event time on its own stream, against the VALU roof for v_sad_u16, with BASELINE's
                 algorithmic-bytes-over-HBM-peak figure and the PMC HBM traffic (profiles/r04_*_pmc.json) as secondary keys; `by_time` = the class that owns the GPU time:
                 k_cu_bits against a wave-instruction issue roof + every kernel class per step (composed), the kernel's own stage profile (fused);
  cpu_baseline : oracle/_ref/xeveb_app (the unmodified reference, compiled in place) on this box's host cores: -m 8 on the same 8-frame GOP (= `value`), -m 1, and
                 `all_cores`: floor(cores available / 8) concurrent -m 8 processes over distinct GOPs.
"""
import argparse
import hashlib
import json
import os
import random
import re
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# /opt/skills/guides/MI355X_MICROARCH.md
HBM_PEAK_GBS = 8000.0
CUS, SIMDS, CLOCK_GHZ = 256, 4, 2.4
VALU_SAD_PEAK_GBS = CUS * SIMDS * 32 * 8 * CLOCK_GHZ  # v_sad_u16: 2 sample pairs = 8 algorithmic bytes per lane, 32 lanes per clock and SIMD (a wave64 issues over 2 clocks)
BYTES_PER_SAMPLE_PAIR = 4  # a block SAD reads 2 x (w * h * 2 B)
BYTES_PER_SEARCH_UNIT = 256  # the composed walk's search kernel counts units of 64 sample pairs
VALU_ISSUE_PEAK_GINST = CUS * SIMDS * CLOCK_GHZ / 2  # wave64 VALU instructions/s (G): one per SIMD every 2 clocks
STAGE_NAMES = ["clear", "enter", "leaf", "child_done", "exit", "root", "mid", "i_setup", "i_nbr", "i_pred", "i_satd", "i_list", "i_bits", "i_pick", "i_cpred", "i_final", "b_diff",
               "b_t0", "b_t1", "b_rdoq", "b_dq", "b_t2", "b_t3", "b_rec", "e_cand", "e_skip", "e_me", "e_spel", "e_mc", "e_bits", "e_glue", "e_final", "m_bits", "m_sad", "m_sel",
               "q_a", "q_b"]
STAGE_GROUPS = {"cabac_bit_counts": ("i_bits", "i_final", "e_bits"), "motion_search": ("m_bits", "m_sad", "m_sel", "e_me"), "rdoq": ("q_a", "q_b", "b_rdoq"),
                "transforms_residual_recon": ("b_diff", "b_t0", "b_t1", "b_dq", "b_t2", "b_t3", "b_rec"), "tree_operations": ("clear", "enter", "leaf", "child_done", "exit", "root", "mid"),
                "prediction_satd_glue": ("i_setup", "i_nbr", "i_pred", "i_satd", "i_list", "i_pick", "i_cpred", "e_cand", "e_skip", "e_mc", "e_glue", "e_final", "e_spel")}


def reference_noise(nbytes, seed):
    """the byte stream of SURVEY.md 8(d)'s recipe -- random.seed(S); bytes(random.getrandbits(8) ...) -- without the Python loop: getrandbits(8) is the top byte of
    one MT19937 output, and numpy's legacy generator runs the same twister from the same state (checked against the loop in tests/test_bench_inputs.py)"""
    random.seed(seed)
    st = random.getstate()
    rs = np.random.RandomState()
    rs.set_state(("MT19937", np.array(st[1][:624], dtype=np.uint32), st[1][624]))
    return (rs.randint(0, 2 ** 32, size=nbytes, dtype=np.uint32) >> 24).astype(np.uint8)


def host_info():
    model, phys = "unknown", set()
    try:
        pid = cid = None
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name") and model == "unknown":
                model = line.split(":", 1)[1].strip()
            elif line.startswith("physical id"):
                pid = line.split(":", 1)[1].strip()
            elif line.startswith("core id"):
                cid = line.split(":", 1)[1].strip()
                phys.add((pid, cid))
    except Exception:
        pass
    usable = len(os.sched_getaffinity(0))
    quota = None
    try:  # the container's CPU-time quota (cgroup v2 cpu.max = "<quota> <period>" or "max ..."): what "every core" means for a process in here
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = max(1, int(q) // int(per))
    except Exception:
        pass
    physical = len(phys) if phys else max(1, (os.cpu_count() or 2) // 2)
    return {"cpu_model": model, "logical_cores": os.cpu_count(), "usable_cores": usable, "physical_cores": physical, "cgroup_cpu_quota": quota,
            "cores_available": min(physical, usable, quota) if quota else min(physical, usable)}


class CpuApp:
    """the reference encoder on this box's host cores, AFTER the GPU's timed region (the composed walk's host threads issue ~90 000 launches a second each: beside a
    9-thread baseline inside a 16-CPU container quota the GPU figure dropped 7 %): start() = -m 8 on the 8-frame seed-4 GOP and -m 1 on its first two frames, side by
    side, while the GPU runs the untimed extras; all_cores_may_start() = then floor(cores available / 8) concurrent -m 8 processes, each on a GOP of its own, once the
    GPU is idle (`all_cores`; cores available = physical cores, capped by the container's CPU quota)"""

    def __init__(self, width, height, frames, clip, with_m1=True, preset="medium"):
        self.w, self.h, self.frames, self.err, self.out, self.preset = width, height, frames, None, {}, preset
        self.exe = os.path.join(ROOT, "oracle", "_ref", "xeveb_app")
        self.host = host_info()
        if not os.path.exists(self.exe):
            self.err = "oracle/_ref/xeveb_app not built"
            return
        try:
            self.dir = tempfile.mkdtemp(prefix="xeve_bench_")
            clip.tofile(os.path.join(self.dir, "in.yuv"))
        except Exception as e:  # noqa: BLE001 -- a reported extra, never a reason to lose the GPU number
            self.err = repr(e)[:200]
            return
        self.with_m1 = with_m1
        self.go_all = threading.Event()
        self.th = threading.Thread(target=self._run, daemon=True)
        self.started = False

    def start(self):
        if not self.err and not self.started:
            self.started = True
            self.th.start()

    def _cmd(self, yuv, frames, m, out):
        return [self.exe, "-i", yuv, "-w", str(self.w), "-h", str(self.h), "-z", "30", "--preset", self.preset, "--closed-gop", "-I", "8", "--frames", str(frames), "-m", str(m), "-o", out]

    @staticmethod
    def _parse(txt, rc):
        fps = re.search(r"Average encoding speed\s*=\s*([0-9.]+)", txt)  # the app's own figure: times xeve_encode only (app/xeve_app.c:1401)
        tot = re.search(r"Total encoding time\s*=\s*[0-9.]+ msec,\s*([0-9.]+) sec", txt)
        return {"fps": float(fps.group(1)) if fps else None, "encoding_s": float(tot.group(1)) if tot else None, "rc": rc}

    def _run(self):
        try:
            yuv = os.path.join(self.dir, "in.yuv")
            p8 = subprocess.Popen(self._cmd(yuv, self.frames, 8, os.path.join(self.dir, "m8.evc")), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            p1 = subprocess.Popen(self._cmd(yuv, 2, 1, os.path.join(self.dir, "m1.evc")), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) if self.with_m1 else None
            txt, _ = p8.communicate(timeout=900)
            self.out["m8"] = self._parse(txt, p8.returncode)
            self.out["m8"]["frames"] = self.frames
            try:
                self.out["m8"]["md5"] = hashlib.md5(open(os.path.join(self.dir, "m8.evc"), "rb").read()).hexdigest()
            except Exception:
                pass
            if p1 is not None:
                txt, _ = p1.communicate(timeout=900)
                self.out["m1"] = self._parse(txt, p1.returncode)
                self.out["m1"]["frames"] = 2
            # all cores: N processes of 8 threads each, every one on its own GOP (the seed-4 GOP and N - 1 GOPs of fresh uniform bytes)
            self.go_all.wait(1800)
            n = max(1, self.host["cores_available"] // 8)
            rng = np.random.default_rng(5)
            files = [yuv]
            for i in range(1, n):
                f = os.path.join(self.dir, "g%d.yuv" % i)
                rng.integers(0, 256, size=self.w * self.h * 3 // 2 * self.frames, dtype=np.uint8).tofile(f)
                files.append(f)
            t0 = time.perf_counter()
            ps = [subprocess.Popen(self._cmd(f, self.frames, 8, os.path.join(self.dir, "a%d.evc" % i)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for i, f in enumerate(files)]
            res = []
            for p in ps:
                txt, _ = p.communicate(timeout=1200)
                res.append(self._parse(txt, p.returncode))
            wall = time.perf_counter() - t0
            enc_s = [r["encoding_s"] for r in res if r["encoding_s"]]
            self.out["all_cores"] = {"processes": n, "threads_each": 8, "cores": n * 8, "frames": n * self.frames,
                                     "fps": round(n * self.frames / max(enc_s), 4) if len(enc_s) == n else None,  # every process's frames over the slowest one's encoding time
                                     "wall_s_incl_file_io": round(wall, 2), "per_process_fps": [r["fps"] for r in res]}
        except Exception as e:  # noqa: BLE001
            self.err = repr(e)[:200]

    def all_cores_may_start(self):
        self.start()
        if not self.err:
            self.go_all.set()

    def result(self, timeout=1500):
        if self.err and not self.out:
            return {"value": None, "unit": "frames/s", "cores": 0, "kind": "reference", "sample": "failed: " + self.err}
        self.all_cores_may_start()
        self.th.join(timeout)
        try:
            import shutil
            shutil.rmtree(self.dir, ignore_errors=True)
        except Exception:
            pass
        m8 = self.out.get("m8", {})
        return {"value": m8.get("fps"), "unit": "frames/s", "cores": 8, "kind": "reference",
                "sample": "oracle/_ref/xeveb_app (the unmodified reference, AVX2 dispatch) -w %d -h %d --preset %s --closed-gop -I 8 --frames %d on the seed-4 uniform 8-bit 4:2:0 "
                          "clip = GOP 0 of the GPU job (1 IDR + 7 B pictures); `value` = -m 8 (the library's thread maximum, the setting the GPU job reproduces byte for byte); "
                          "`m1` = -m 1 on the clip's first 2 frames; `all_cores` = floor(cores available / 8) such processes side by side, each on its own GOP (cores available = "
                          "physical cores capped by the container's CPU quota, `host`); -m 8 and -m 1 ran after the GPU's timed region beside its untimed extras, all_cores with the GPU idle" % (self.w, self.h, self.preset, self.frames),
                "m8": m8, "m1": self.out.get("m1", {}), "all_cores": self.out.get("all_cores", {}), "host": self.host, "error": self.err}


def golden_prefix(width, height, frames, threads, preset="medium"):
    """the reference's bitstream of the seed clip at this size and preset, as (bytes, md5) after every coded picture (tests/golden/cfg4_8f_v1.json), or None"""
    try:
        g = json.load(open(os.path.join(ROOT, "tests", "golden", "cfg4_8f_v1.json")))
        for name, r in g.items():
            if (r["w"], r["h"], r["frames"]) == (width, height, frames) and threads == 8 and r["cli"][1] == preset:
                return name, r
    except Exception:
        pass
    try:  # the 2-frame job of rounds 1-3 (--frames 2 --pictures 0): the whole file's golden
        if (width, height, frames, threads, preset) == (3840, 2160, 2, 8, "medium"):
            r = json.load(open(os.path.join(ROOT, "tests", "golden", "e2e_v1.json")))["cfg4_2160p_closedgop_medium_m8"]
            return "e2e_v1.json:cfg4_2160p_closedgop_medium_m8", {"after_picture": [{"bytes": -1, "md5": ""}, {"bytes": r["bytes"], "md5": r["md5"]}]}
    except Exception:
        pass
    return None, None


def check_prefix(stream, gold):
    """how many coded pictures of the golden bitstream `stream` is exactly the prefix of (0: none)"""
    for k, p in enumerate(gold["after_picture"]):
        if len(stream) == p["bytes"]:
            return k + 1 if hashlib.md5(stream).hexdigest() == p["md5"] else 0
    return 0


def step_ctus(per_picture):
    """lockstep CTU steps in one bench step: 3/25 of a picture's (36 at 3840x2160) -- the slice the driver's --steps 20 --warmup 5 cut from the first three pictures
    before a step became a fixed unit -- whatever --steps and --warmup say"""
    return max(1, 3 * per_picture // 25)


def pictures_done(run_steps, per_picture):
    """(the pictures the first run_steps lockstep steps reach into, the steps still to issue to finish the last of them): --dump-outputs runs the job on, untimed, by
    that many steps, so that the picture the timed steps left part way is in the dump and a dump always holds at least one whole picture"""
    P = max(1, -(-run_steps // per_picture))
    return P, P * per_picture - run_steps


# the GOPs whose bitstreams --dump-outputs samples: GOP 0 and 15 others drawn once from GOPs 1 .. 255, whatever the batch size (those beyond it are left out)
DUMP_SAMPLE_GOPS = [0] + sorted(np.random.default_rng(20261016).choice(np.arange(1, 256), size=15, replace=False).tolist())


def dump_outputs(out_dir, encs, gops_per_batch, pictures):
    """what the timed path has produced, once the picture its last step left part way is finished: every GOP's bitstream (xeve_hip_enc_flush), written as float arrays
    -- the byte count and byte sum of every GOP (GOPs of all batches in order), and of the sample GOPs (DUMP_SAMPLE_GOPS) the CRC-32 of the whole bitstream and its bytes
    at 2^18 fixed, seeded positions -- 17 MB at most; beside them the pictures they hold and the GOPs of every batch (the batch sizes follow the free HBM)"""
    import zlib

    if pictures < 1:
        raise RuntimeError("bench.py --dump-outputs: the dump would hold no whole picture")
    for e in encs:
        e.flush()
    where = [(e, g) for e, n in zip(encs, gops_per_batch) for g in range(n)]
    pick = [g for g in DUMP_SAMPLE_GOPS if g < len(where)]
    u = np.random.default_rng(20261017).random(1 << 18)
    sizes, sums = np.zeros(len(where), np.float64), np.zeros(len(where), np.float64)
    crc, sample = np.zeros(len(pick), np.float64), np.zeros((len(pick), 1 << 18), np.float32)
    for i, (e, g) in enumerate(where):
        b = e.bitstream(g)
        if not b:
            raise RuntimeError("bench.py --dump-outputs: GOP %d has no bitstream after %d pictures" % (i, pictures))
        v = np.frombuffer(b, dtype=np.uint8)
        sizes[i], sums[i] = len(b), v.sum(dtype=np.uint64)
        if i in pick:
            k = pick.index(i)
            crc[k] = zlib.crc32(b)
            sample[k] = v[(u * len(b)).astype(np.int64)]
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "bitstream_bytes.npy"), sizes)
    np.save(os.path.join(out_dir, "bitstream_byte_sum.npy"), sums)
    np.save(os.path.join(out_dir, "bitstream_sample_gops.npy"), np.array(pick, np.float64))
    np.save(os.path.join(out_dir, "bitstream_sample_crc32.npy"), crc)
    np.save(os.path.join(out_dir, "bitstream_sample.npy"), sample)
    np.save(os.path.join(out_dir, "pictures.npy"), np.array([pictures], np.float64))
    np.save(os.path.join(out_dir, "gops_per_batch.npy"), np.array(gops_per_batch, np.float64))


def run_job(a, torch, dist, dev, rank, world, W, H, label, with_cpu, full=True, dump_dir=None):
    """one bounded encode at W x H: the --warmup + --steps bench steps of step_ctus() lockstep CTU steps each; returns the result record (rank 0) or None.
    full (--full): the roofline's HIP-event timers in the timed region and, after it, the job run on to the end of picture --pictures and checked against the golden"""
    from xeve_amd import encode, lib

    F, T = a.frames, a.threads
    fb = W * H * 3 // 2
    w_lcu, h_lcu = (W + 63) // 64, (H + 63) // 64
    seed = {(3840, 2160): 4, (1920, 1080): 3}.get((W, H), 4)
    cfg = encode.config(W, H, qp=32, keyint=8, bframes=15, closed_gop=True, preset=a.preset, threads=T)
    free0 = torch.cuda.mem_get_info(dev)[0]
    one, most = encode.footprint(cfg, 1, F)
    two, _ = encode.footprint(cfg, 2, F)
    per_gop, fixed = max(1, two - one), max(0, 2 * one - two)
    Gs, room = [], free0 - (10 << 30)
    want = a.gops or most
    for _ in range(max(1, a.batches)):
        g = int(min(want, most, (room - fixed) // per_gop))
        if g < max(1, min(want, most) // 8):
            break
        Gs.append(g)
        room -= fixed + g * per_gop
    if not Gs:
        raise SystemExit("bench.py: not enough device memory for one GOP at %dx%d" % (W, H))
    encs = [encode.BatchEncoder(cfg, g, F) for g in Gs]
    B, enc = len(encs), encs[0]

    # inputs: a.seeded GOPs (64) of every batch of rank 0 = the reference recipe's seed clip (its bitstream has a golden); every other GOP i.i.d. uniform bytes made on the
    # device.  (Round 6 raised the count from 16: it was this check -- one of the seeded GOPs coming out different from GOP 0 -- that caught a one-in-250 000 race of the
    # tree operations which every test of the suite had passed.)
    clip = reference_noise(fb * F, seed) if rank == 0 else None
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000 + rank)
    NS = max(2, a.seeded)
    seeded = [sorted({int(round(i * (g - 1) / max(1, min(g, NS) - 1))) for i in range(min(g, NS))}) for g in Gs]  # spread over every batch, its first and last among them
    for b, e in enumerate(encs):
        for g in range(Gs[b]):
            if g in seeded[b] and clip is not None:
                d = torch.from_numpy(clip).to(dev)
            else:
                d = torch.randint(0, 256, (fb * F,), dtype=torch.uint8, device=dev, generator=gen)
            for f in range(F):
                e.push(g, f, d[f * fb:(f + 1) * fb])
    del d
    cpu = CpuApp(W, H, F, clip, True, a.preset) if with_cpu else None  # (started after the timed region)

    def fence():
        for e in encs:
            e.sync()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()

    for e in encs:
        e.begin()
    total = enc.advance(0)
    per_picture = total // F
    SAMPLE_STEPS = 2
    n = a.warmup + a.steps
    per = step_ctus(per_picture)
    if n * per > total:
        raise SystemExit("bench.py: --warmup + --steps = %d steps of %d lockstep CTU steps each run past the end of the %d-frame GOP at %dx%d (%d steps at most)"
                         % (n, per, F, W, H, total // per))
    sizes = [per] * n
    run_steps = n * per
    P = pictures_done(run_steps, per_picture)[0]  # the pictures the steps reach into (the last one may be left part way)

    L = lib.load()
    # which walk every batch's steps run (walk.hip: by the chains in lockstep, or pinned by --walk; presets slow and placebo: the fused walk at any width, xh_walk_only)
    fused = [bool(L.xeve_hip_walk_fused(g * min(T, h_lcu))) or a.preset in ("slow", "placebo") for g in Gs]
    cls = "walk" if fused[0] else "search"
    live = [0.0, 0, 0]

    def drain():
        v = lib.prof_read()[cls]  # (waits for the device: only at a fence or, with one batch, between slices -- keeps the pool of timing events small)
        live[0] += v[0]
        live[1] += v[1]
        live[2] += v[2]

    def run_slices(lo, hi, timers=False):
        """slices [lo, hi) of every batch; the batches' host threads issue side by side (the library call releases the GIL).  timers: HIP events around the roofline
        kernel's launches on their own stream, live in the timed region -- the fused walk's one launch per step throughout; the composed walk's search kernel (hundreds of
        launches per step) in the last steps of every slice"""
        def one(e):
            for i in range(lo, hi):
                if timers and cls == "search":
                    # the composed walk: the search kernel's events are live in the LAST SAMPLE_STEPS steps of EVERY timed slice (batch 0's thread switches them on and
                    # off; the mask is the library's, so other batches' search launches of those moments are sampled too) -- a sample spread over every picture the timed
                    # region covers (round 4 timed the last slice only and the per-launch figures moved 27 % between two runs), ~850 event pairs per slice instead of one
                    # per launch; read out once, after the region (a read-out waits for the device)
                    k = min(SAMPLE_STEPS, sizes[i]) if e is enc else 0
                    e.advance(sizes[i] - k)
                    if k:
                        lib.prof_enable([cls])
                        e.advance(k)
                        lib.prof_enable(None)
                    continue
                if timers:
                    lib.prof_enable([cls])
                e.advance(sizes[i])
        if B == 1:
            one(enc)
            return
        import concurrent.futures as cf
        with cf.ThreadPoolExecutor(B) as ex:
            list(ex.map(one, encs))

    run_slices(0, a.warmup)
    fence()
    if full:
        lib.prof_enable(None)
        lib.prof_read()
        fence()
    t0 = time.perf_counter()
    run_slices(a.warmup, n, timers=full)
    fence()
    dt = time.perf_counter() - t0
    if full:
        drain()
        lib.prof_enable(None)
    k_ms, k_n, k_units = live
    if cpu is not None:
        cpu.start()
    timed_steps = sum(sizes[a.warmup:])
    first_timed = sum(sizes[:a.warmup])
    frames_timed = sum(Gs) * timed_steps / per_picture
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device="cpu" if os.environ.get("XEVE_BENCH_SHARE_GPU") == "1" else dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    stats = enc.stats()
    mix = {}  # which pictures (coding order) the timed steps belong to
    for s in range(first_timed, first_timed + timed_steps):
        k = s // per_picture
        mix[k] = mix.get(k, 0) + 1
    done = run_steps

    def run_on(upto):  # the job on, untimed, to the end of picture `upto`
        nonlocal done
        if upto * per_picture > done:
            for e in encs:
                e.advance(upto * per_picture - done)
            fence()
            done = upto * per_picture

    if dump_dir:  # the picture the timed steps left part way is finished first, so that the dump holds all their work
        run_on(P)
        if rank == 0:
            dump_outputs(dump_dir, encs, Gs, P)
    if full:  # to the end of picture --pictures (0: the whole GOP) or of the picture the steps left part way, whichever is later
        P = max(P, F if a.pictures <= 0 else min(F, a.pictures))
        run_on(P)
    rec = None
    if rank == 0:
        basic = {"value": round(world * frames_timed / dt, 4), "ms_per_step": round(1e3 * dt / a.steps, 3),
                 "config": {
                     "workload": "%s: %d + %d bench steps of %d lockstep CTU steps (the first %d of %d pictures) of %d batches of %s closed GOPs x %d frames per GPU, %dx%d Baseline "
                                 "preset %s (xeveb_app --preset %s --closed-gop -I 8 -m %d semantics), i.i.d. uniform 8-bit 4:2:0 input resident in HBM, QP 32"
                                 % (label, a.warmup, a.steps, per, P, F, B, "+".join(str(g) for g in Gs), F, W, H, a.preset, a.preset, T),
                     "walk": ["fused (one k_walk launch per step)" if f else "composed (~7 000 / ~11 000 launches per I / B step, on two streams)" for f in fused],
                     "walk_choice": "presets slow and placebo run on the fused walk at any width (rdo_dbk_switch, 4x4 inter CUs: xh_common.h xh_walk_only)" if a.preset in ("slow", "placebo") else
                                    "pinned by --walk / XEVE_HIP_WALK" if os.environ.get("XEVE_HIP_WALK") in ("0", "1") else
                                    "the library's choice (walk.hip: since round 6 the composed walk at every width -- with its side stream it finishes a step sooner than the fused kernel "
                                    "even at 8 chains; profiles/r06_side_stream.md)",
                     "batches_side_by_side": B, "gops_in_lockstep": Gs, "frames_per_gop": F, "pictures_run": P, "row_chains_per_picture": T,
                     "chains_in_lockstep": [g * min(T, h_lcu) for g in Gs], "lockstep_steps_per_picture": per_picture, "ctu_steps_per_step": per, "lockstep_steps_timed": timed_steps,
                     "timed_picture_mix": {"picture_%d%s" % (k, "_IDR" if k == 0 else "_B"): round(v / per_picture, 3) for k, v in sorted(mix.items())},
                     "frames_in_timed_region": round(frames_timed, 2), "ctus_per_picture": w_lcu * h_lcu,
                     "parallelism": "closed-GOP shards per GPU, no collectives" + (" [SELF-TEST: all ranks share GPU 0, gloo]" if os.environ.get("XEVE_BENCH_SHARE_GPU") == "1" else "")},
                 "encode": {"host_seconds_issuing_steps": round(stats["step_seconds"], 3), "seconds_in_picture_ends": round(stats["picture_end_seconds"], 2),
                            "note": "time the host spent inside the library's step calls (the fused walk is one launch per step) and inside the picture ends"}, "cpu": cpu}
    if rank == 0 and not full:
        rec = basic
    elif rank == 0:
        gname, gold = golden_prefix(W, H, F, T, a.preset)
        for e in encs:
            e.flush()  # (the access unit of the last picture run: appended now instead of at the next picture's end, so that every picture that was run is checked)
        streams = [[e.bitstream(g) for g in idx] for e, idx in zip(encs, seeded)]
        same = all(s == streams[0][0] for b in streams for s in b)
        check = {"gop0_bytes_so_far": len(streams[0][0]), "gop0_md5_so_far": hashlib.md5(streams[0][0]).hexdigest(),
                 "seeded_gops": {"per_batch": [len(i) for i in seeded], "what": "GOPs spread evenly over every batch (its first and its last among them) that carry the golden clip"},
                 "all_seeded_gops_same_bytes": same}
        if gold is not None:
            k = check_prefix(streams[0][0], gold)
            check.update({"reference_golden": "tests/golden/" + (gname if gname.startswith("e2e") else "cfg4_8f_v1.json:" + gname), "pictures_of_the_golden_gop_matched": k,
                          "byte_identical_to_the_reference": bool(k > 0 and same),
                          "note": "the bitstream GOP 0 has produced when the bounded job stops (every picture that was run: xeve_hip_enc_flush) against the reference's "
                                  "bitstream after the same picture; whole 8-frame GOPs: tests/test_enc_gpu.py (1920x1080) and profiles/r05_bench_whole_gop.json (3840x2160)"})
        alg = k_units * (BYTES_PER_SAMPLE_PAIR if cls == "walk" else BYTES_PER_SEARCH_UNIT)
        alg_gbs = alg / (k_ms * 1e-3) / 1e9 if k_ms > 0 else 0.0
        roof = {"kernel": "k_walk (xeve_amd/csrc/walk.h: the whole CTU mode decision of a lockstep step in ONE launch; the motion search's SAD rounds run inside it)" if cls == "walk" else
                          "k_me_epzs<8|16|32|64, uni|bi> (the integer motion search inside xeve_hip_mode_analyze_ctu_jobs; the SAD kernel of the path)",
                "bound": "valu", "achieved": round(alg_gbs, 2), "peak": VALU_SAD_PEAK_GBS, "unit": "GB/s", "frac": round(alg_gbs / VALU_SAD_PEAK_GBS, 6),
                "how": ("algorithmic bytes of the motion search (4 per sample pair compared, counted on the device) over the HIP-event time of the kernel's launches in the timed "
                        "region (events on the walk's own streams), against the rate at which the chip's VALUs can issue v_sad_u16.  The kernel is the whole analysis: the search is "
                        "one stage class of it (`by_time`), so this is the SAD work per second of a kernel that spends most of its time elsewhere") if cls == "walk" else
                       ("algorithmic bytes (256 per 64 sample pairs evaluated, counted on the device) over the kernel's HIP-event time in the timed region (the launch's own start / stop events, hipExtLaunchKernelGGL: the dispatch's begin and end, not the stream's wait in front of it), against the rate at "
                        "which the chip's VALUs can issue v_sad_u16 (8 algorithmic bytes per lane and instruction)"),
                "launches_in_region": k_n, "avg_launch_ms": round(k_ms / max(1, k_n), 4), "algorithmic_bytes_per_launch": int(alg / max(1, k_n)),
                "hbm_algorithmic_frac": round(alg_gbs / HBM_PEAK_GBS, 6), "traffic": None}
        # from the committed PMC passes (rocprofv3 --pmc in runs of their own, profiles/: the newest round's file that exists): physical HBM bytes per launch of the same
        # kernel (`traffic`), what its wave cycles were spent on, and the matrix-core kernels' utilisation
        def committed(*names):
            for nm in names:
                try:
                    return json.load(open(os.path.join(ROOT, "profiles", nm))), nm
                except Exception:
                    continue
            return None, None
        pmc, src = committed(*(("r05_walk_pmc.json", "r04_walk_pmc.json") if cls == "walk" else ("r07_search_pmc.json", "r06_search_pmc.json", "r05_search_pmc.json", "r04_search_pmc.json")))
        if pmc:
            roof["pmc_from_committed_profile"] = True  # (the counters below were taken by rocprofv3 --pmc runs of their own and committed; this run measured the time)
            roof["traffic"] = pmc.get("hbm_bytes_per_launch") or pmc.get("hbm_bytes_per_launch_x2")
            roof["traffic_is"] = pmc.get("what")
            roof["pmc_file"] = "profiles/" + src
            for k in ("valu_insts_per_launch", "valu_issue_frac", "wait_any_frac", "active_lane_frac", "waves_per_launch", "avg_launch_s"):
                if k in pmc:
                    roof[k] = pmc[k]
            if roof["traffic"] is None:  # (a pass without FETCH_SIZE: the traffic figure of the last pass that took it)
                old, osrc = committed("r04_walk_pmc.json" if cls == "walk" else "r04_search_pmc.json")
                if old:
                    roof["traffic"], roof["traffic_is"] = old.get("hbm_bytes_per_launch") or old.get("hbm_bytes_per_launch_x2"), old.get("what")
        mf, msrc = committed("r07_mfma_pmc.json", "r06_mfma_pmc.json", "r05_mfma_pmc.json")
        if mf:
            roof["mfma"] = {"kernels": "k_rdo_mfma<32|64>, k_dct_mfma<32|64> (v_mfma_i32_32x32x32_i8, exact byte-limb split: the residual chain of the 32x32 / 64x64 luma blocks)",
                            "bound": "mfma", "achieved": mf.get("achieved_TOPS"), "peak": mf.get("peak_TOPS_i8_dense"), "unit": "TOP/s", "frac": mf.get("mfma_utilisation"),
                            "mfma_busy_over_all_simd_cycles": mf.get("mfma_busy_over_all_simd_cycles"), "avg_launch_s": mf.get("avg_launch_s"),
                            "mfma_i8_insts_per_launch": mf.get("mfma_i8_insts_per_launch"), "pmc_file": "profiles/" + msrc, "what": mf.get("what"),
                            "note": "a 32x32 / 64x64 transform is the only dense matrix product on the path; those blocks are < 1 % of a step's kernel time"}
        rec = dict(basic, bitstream_check=check, roofline=roof)
    for e in encs:  # (the job's HBM goes back; an unfinished run is abandoned)
        e.close()
    return rec, (cfg, Gs, per_picture, fb, cls)


def stage_profile(torch, dev, cfg, gops, frames, per_picture, fb, steps=4):
    """the kernel's own stage profile: a short untimed encode with the in-kernel cycle marks on -- thread 0 of team 0, steps of the first B picture"""
    from xeve_amd import encode, lib
    import ctypes as C

    L = lib.load()
    e = encode.BatchEncoder(cfg, gops, frames)
    gen = torch.Generator(device=dev)
    gen.manual_seed(77)
    d = torch.randint(0, 256, (fb * frames,), dtype=torch.uint8, device=dev, generator=gen)
    for g in range(gops):
        for f in range(frames):
            e.push(g, f, d[f * fb:(f + 1) * fb])
    e.begin()
    e.advance(per_picture)  # the IDR picture
    e.sync()
    L.xeve_hip_walk_prof_enable(1)
    buf = (C.c_uint64 * (2 * len(STAGE_NAMES) + 8))()
    e.advance(1)
    e.sync()
    L.xeve_hip_walk_prof(buf, len(buf))  # (the first profiled step allocates the counters: dropped)
    e.advance(steps)
    e.sync()
    n = L.xeve_hip_walk_prof(buf, len(buf))
    L.xeve_hip_walk_prof_enable(0)
    e.close()
    if n <= 0:
        return None
    cyc = {STAGE_NAMES[i]: int(buf[i]) for i in range(min(n, len(STAGE_NAMES)))}
    tot = sum(cyc.values()) or 1
    groups = {g: round(sum(cyc.get(k, 0) for k in ks) / tot, 4) for g, ks in STAGE_GROUPS.items()}
    top = max(groups, key=groups.get)
    return {"kernel": "k_walk, its own stage classes (shader cycles of team 0's thread 0 between stage marks; %d lockstep steps of the first B picture, %d GOPs)" % (steps, gops),
            "share_of_kernel_time": groups, "dominant": top, "bound": "latency of serial lanes (a CABAC bit count is a recurrence per bin: ~170 cycles per bin and lane, "
            "tools/cod_bench.hip; the stage lasts as long as its longest lane)", "cycles_per_step_team0": tot // max(1, steps)}


def class_profile(torch, dev, cfg, gops, frames, per_picture, fb, steps=6):
    """the composed walk per kernel class: a short untimed encode with every class's HIP-event timer on, steps of the first B picture"""
    from xeve_amd import encode, lib

    e = encode.BatchEncoder(cfg, gops, frames)
    gen = torch.Generator(device=dev)
    gen.manual_seed(77)
    d = torch.randint(0, 256, (fb * frames,), dtype=torch.uint8, device=dev, generator=gen)
    for g in range(gops):
        for f in range(frames):
            e.push(g, f, d[f * fb:(f + 1) * fb])
    e.begin()
    e.advance(per_picture + 16)  # the IDR picture and the first B picture's ramp (a picture's first steps carry one or two row chains per GOP)
    e.sync()
    lib.prof_enable([c for c in lib.PROF_CLASSES if c != "walk"])
    lib.prof_read()
    lib.prof_cu_bits_hist(reset=True)
    e.advance(steps)
    e.sync()
    allc = lib.prof_read()
    hist = lib.prof_cu_bits_hist()
    lib.prof_enable(None)
    e.close()
    kern = {c: {"ms_per_step": round(v[0] / steps, 3), "launches_per_step": v[1] // steps} for c, v in allc.items() if c != "walk"}
    cb = allc["cu_bits"]
    bins_s = cb[2] / (cb[0] * 1e-3) if cb[0] > 0 else 0.0
    kern["cu_bits"].update({"bins_per_step": int(cb[2] / steps), "Gbin_per_s": round(bins_s / 1e9, 3), "bins_per_job_histogram": hist,
                            "bins_per_job_note": "jobs (lanes) of the %d steps by their bin count: most lanes of a launch carry a handful of header bins (candidate indices, "
                                                 "all-zero alternatives, mode bits), a few carry a CU's coefficients -- a launch lasts as long as its longest lane" % steps})
    tot = sum(v[0] for c, v in allc.items() if c not in ("cu_bits_slow", "walk"))
    # The instruction rate comes from the PMC pass over the same kernel at the bench's width (profiles/, committed: SQ_INSTS_VALU per launch over the launch's duration) --
    # not from a per-bin constant: a launch's lanes carry 0 .. ~25 000 bins each and a wave runs as long as its longest lane, so "instructions per bin" is not a
    # property of the code (profiles/r06_cu_bits_bins.md has the histogram)
    lanes, ginst = {}, None
    for nm in ("r07_cu_bits_pmc.json", "r06_cu_bits_pmc.json", "r05_cu_bits_pmc.json"):
        try:  # (how many of a wave's lanes its VALU work keeps busy, what its cycles wait for)
            pm = json.load(open(os.path.join(ROOT, "profiles", nm)))
            lanes = {k: pm[k] for k in ("active_lane_frac", "active_lane_frac_note", "wait_any_frac", "valu_issue_frac", "waves_per_launch", "valu_insts_per_launch", "avg_launch_s") if k in pm}
            lanes["pmc_file"], lanes["pmc_from_committed_profile"] = "profiles/" + nm, True
            ginst = pm["valu_insts_per_launch"] / pm["avg_launch_s"] / 1e9
            break
        except Exception:
            continue
    return {"kernel": "k_cu_bits (CABAC bit counting, one lane per job): the class with the largest share of the GPU time", "share_of_timed_classes": round(cb[0] / tot, 3) if tot else None, **lanes,
            "bound": "valu-issue", "achieved": round(ginst, 3) if ginst else None, "peak": round(VALU_ISSUE_PEAK_GINST, 1), "unit": "G wave-instructions/s",
            "frac": round(ginst / VALU_ISSUE_PEAK_GINST, 6) if ginst else None,
            "how": "VALU wave-instructions per launch over the launch's duration (PMC pass, committed profile) against one wave64 VALU instruction per SIMD every 2 clocks on "
                   "%d CUs x %d SIMDs at %.1f GHz; a serial chain per lane and a few hundred waves per launch, so the roof is only reachable with every SIMD holding busy waves" % (CUS, SIMDS, CLOCK_GHZ),
            "kernels": kern, "kernels_note": "HIP-event time per lockstep step of the first B picture (steps 16 .. %d: all 8 row chains of every GOP active) with %d GOPs in lockstep, all class timers on (untimed extra encode)" % (16 + steps, gops)}


def width_sweep(torch, dev, preset, threads, headline):
    """What the headline depends on: the same encoder with 1, 8 and 64 closed GOPs in lockstep instead of everything HBM holds.  Measured at 1920x1080
    (IDR + one B picture of each: 180 lockstep steps, seconds); a lockstep step's time depends on the chains it carries and the slice type, not on the picture, so the
    3840x2160 figures follow from the same per-step times with 302 steps per picture."""
    from xeve_amd import encode

    W, H, F = 1920, 1080, 2
    fb = W * H * 3 // 2
    cfg = encode.config(W, H, qp=32, keyint=8, bframes=15, closed_gop=True, preset=preset, threads=threads)
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    rows = []
    for G in (1, 8, 64):
        e = encode.BatchEncoder(cfg, G, F)
        for g in range(G):
            d = torch.randint(0, 256, (fb * F,), dtype=torch.uint8, device=dev, generator=gen)
            for f in range(F):
                e.push(g, f, d[f * fb:(f + 1) * fb])
        e.begin()
        per = e.advance(0) // F
        t = []
        for _ in range(F):
            e.sync()
            t0 = time.perf_counter()
            e.advance(per)
            e.sync()
            t.append(time.perf_counter() - t0)
        e.close()
        ms_i, ms_b = 1e3 * t[0] / per, 1e3 * t[1] / per
        gop_ms = lambda steps: steps * (ms_i + 7 * ms_b)  # an 8-frame closed GOP: 1 IDR + 7 B pictures
        rows.append({"gops_in_lockstep": G, "chains_in_lockstep": G * min(threads, (H + 63) // 64), "ms_per_step_idr": round(ms_i, 2), "ms_per_step_b": round(ms_b, 2),
                     "frames_per_s_1920x1080": round(8 * G / (gop_ms(per) * 1e-3), 4), "frames_per_s_3840x2160_from_step_times": round(8 * G / (gop_ms(302) * 1e-3), 4),
                     "gop_latency_s_3840x2160": round(gop_ms(302) * 1e-3, 1)})
    out = {"what": "the batch encoder with 1, 8 and 64 closed GOPs in lockstep (8 row chains each): per-step times measured at 1920x1080 (IDR + first B picture, %d steps each); an "
                   "8-frame GOP = 1 IDR + 7 B pictures; the 3840x2160 columns = the same per-step times x 302 steps per picture (a step's time follows the chains in lockstep "
                   "and the slice type, not the picture size)" % per,
           "rows": rows, "headline": headline}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--gops", type=int, default=0, help="closed GOPs in lockstep per batch (0: as many as a batch holds at this picture size)")
    ap.add_argument("--frames", type=int, default=8, help="frames per GOP (8: the full -I 8 closed GOP, 1 IDR + 7 B pictures)")
    ap.add_argument("--pictures", type=int, default=3, help="--full: after the timed steps the job runs on, untimed, to the end of this picture of every GOP (0: the whole GOP) "
                    "and GOP 0 is checked against the reference's golden prefix")
    ap.add_argument("--threads", type=int, default=8, help="row chains per picture = the reference's -m")
    ap.add_argument("--batches", type=int, default=3, help="batches encoded side by side on this GPU (a host thread and a HIP stream each)")
    ap.add_argument("--walk", default=os.environ.get("XEVE_BENCH_WALK", "auto"), choices=["auto", "fused", "composed"],
                    help="the CTU walk: one kernel per step (fused), ~10 000 launches per step (composed), or the library's choice by the chains in lockstep (auto)")
    ap.add_argument("--preset", default="medium", choices=["fast", "medium", "slow", "placebo"],
                    help="the headline is preset medium (BASELINE.json); slow and placebo run on the fused walk at any width, their lines are secondary records (profiles/)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="skip the untimed extra (the per-class / per-stage profile of the walk)")
    ap.add_argument("--seeded", type=int, default=64, help="GOPs of every batch that carry the reference's clip and are compared with its golden bitstream after the run")
    ap.add_argument("--no-width-sweep", action="store_true", help="skip the untimed extra that runs 1, 8 and 64 GOPs in lockstep (what the headline depends on; ~40 s)")
    ap.add_argument("--no-1080p", action="store_true", help="skip the same bounded job at 1920x1080 that follows the headline (north_star names both sizes; ~2 more minutes, after the timed region)")
    ap.add_argument("--with-1080p", action="store_true", help="(the default since round 5; kept so that older command lines still parse)")
    ap.add_argument("--full", action="store_true", help="everything beyond the headline: the roofline's timers in the timed region, the bitstream check, the per-class / per-stage "
                    "profile, the width sweep, the job at 1920x1080 and the CPU baseline (each --no-* option above still drops its part)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, finish the picture they left part way (untimed) and write what they "
                    "produced (the GOPs' bitstreams: sizes, sums, a seeded sample; the pictures they hold) as DIR/*.npy")
    a = ap.parse_args()
    if a.walk == "composed":
        os.environ["XEVE_HIP_WALK"] = "0"
    elif a.walk == "fused":
        os.environ["XEVE_HIP_WALK"] = "1"

    import torch
    import torch.distributed as dist

    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    if world != a.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d (launch N>1 with torch.distributed.run)" % (a.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X; there is no CPU fallback for the product path")
    # harness self-test only: XEVE_BENCH_SHARE_GPU=1 runs every rank on GPU 0 with the gloo backend, so that the N > 1 control path (barriers, max-over-ranks, rank-0
    # JSON) can be exercised on a one-GPU box; never used for numbers
    share = os.environ.get("XEVE_BENCH_SHARE_GPU") == "1"
    if share:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if share:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)
    lib_path = os.path.join(ROOT, "xeve_amd", "lib", "libxeve_hip.so")
    built_here = False
    if not os.path.exists(lib_path) and local == 0:
        import __graft_entry__

        __graft_entry__.build()  # fresh checkout on the GPU box: compile once (hipcc is in the image)
        built_here = True
    if world > 1:
        dist.barrier()
    import xeve_amd

    xeve_amd.init(local)
    solo = rank == 0 and world == 1
    rec, (cfg, Gs, per_picture, fb, cls) = run_job(a, torch, dist, dev, rank, world, a.width, a.height, "headline", a.full and solo and not a.no_cpu_baseline,
                                                   a.full, a.dump_outputs)
    line = None
    if rank == 0:
        cpu = rec.pop("cpu")
        line = {"metric": "encoded frames/sec @ 2160p Baseline %s; SAD-kernel HBM GB/s vs peak" % a.preset, "value": rec["value"], "unit": "frames/s", "n_gpus": world, "steps": a.steps,
                "warmup": a.warmup, "ms_per_step": rec["ms_per_step"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                "dtype": "s16 samples, s32/s64 accumulation, f64 cost comparisons (bit-exact)", "data": "synthetic",
                "value_is": "encoded frames/s of the closed-GOP batch encoder on full 8-frame closed GOPs: a real encode to EVC bitstreams (every stage of the reference's xeve_pic "
                            "on the device, NAL assembly on the host), byte-identical to the reference encoder; frames = the timed share of the pictures that were run",
                "config": rec["config"], "encode": rec["encode"]}
        if a.full:
            line.update(bitstream_check=rec["bitstream_check"], roofline=rec["roofline"])
        line["config"]["library_built_in_this_run"] = built_here
    if a.full and solo and not a.no_secondary:
        try:
            line["roofline"]["by_time"] = (stage_profile if cls == "walk" else class_profile)(torch, dev, cfg, max(8, Gs[0] // 4) if cls == "walk" else max(136, Gs[0] // 2), a.frames, per_picture, fb)
        except Exception as e:  # noqa: BLE001
            line["roofline"]["by_time"] = {"error": repr(e)[:300]}
        if not a.no_width_sweep and a.preset in ("fast", "medium"):
            try:
                lat = rec["ms_per_step"] * a.steps / max(1, rec["config"]["lockstep_steps_timed"]) * rec["config"]["lockstep_steps_per_picture"] * a.frames * 1e-3
                line["width_sweep"] = width_sweep(torch, dev, a.preset, a.threads,
                                                  {"gops_in_lockstep": sum(Gs), "frames_per_s": rec["value"], "gop_latency_s": round(lat, 1),
                                                   "gop_latency_is": "every GOP of the batch is finished when the batch is: %d lockstep steps per GOP at the timed region's mean step time" % (rec["config"]["lockstep_steps_per_picture"] * a.frames)})
            except Exception as e:  # noqa: BLE001
                line["width_sweep"] = {"error": repr(e)[:300]}
        if not a.no_1080p and (a.width, a.height) == (3840, 2160):  # north_star names both sizes: the same bounded job at 1920x1080 (untimed by the driver's clock, reported beside the headline)
            try:
                r2, _ = run_job(a, torch, dist, dev, rank, world, 1920, 1080, "secondary", False)
                r2.pop("cpu")
                line["at_1920x1080"] = {"value": r2["value"], "unit": "frames/s", "ms_per_step": r2["ms_per_step"], "config": r2["config"], "bitstream_check": r2["bitstream_check"],
                                        "roofline_frac": r2["roofline"]["frac"]}
            except Exception as e:  # noqa: BLE001
                line["at_1920x1080"] = {"error": repr(e)[:300]}
    if rank == 0:
        if cpu is not None:
            line["cpu_baseline"] = cpu.result()
            try:
                ac = line["cpu_baseline"].get("all_cores", {}).get("fps")
                line["vs_cpu"] = {"gpu_over_m8": round(line["value"] / line["cpu_baseline"]["value"], 2) if line["cpu_baseline"].get("value") else None,
                                  "gpu_over_all_cores": round(line["value"] / ac, 2) if ac else None}
                m8 = line["cpu_baseline"].get("value")
                rows = line.get("width_sweep", {}).get("rows")
                if m8 and rows:  # the width at which the GPU overtakes `xeveb_app -m 8` on one GOP at a time: linear between the measured widths
                    pts = [(r["gops_in_lockstep"], r["frames_per_s_3840x2160_from_step_times"]) for r in rows] + [(line["width_sweep"]["headline"]["gops_in_lockstep"], line["value"])]
                    be = None
                    for (g0, f0), (g1, f1) in zip([(0, 0.0)] + pts, pts):
                        if f0 < m8 <= f1:
                            be = g0 + (g1 - g0) * (m8 - f0) / (f1 - f0)
                            break
                    line["width_sweep"]["break_even_gops_vs_xeveb_app_m8"] = round(be, 1) if be is not None else None
                    line["width_sweep"]["break_even_note"] = "GOPs in lockstep at which the GPU's 3840x2160 frames/s equal the reference application's -m 8 on this host (%.3f frames/s), interpolated between the measured widths" % m8
            except Exception:
                pass
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
