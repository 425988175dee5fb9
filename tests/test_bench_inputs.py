"""bench.py's input for GOP 0 must be the very clip whose reference bitstream is the committed golden (tests/golden/e2e_v1.json cfg4_*): SURVEY.md 8(d)'s recipe
random.seed(S); bytes(random.getrandbits(8) ...), which bench.py reproduces without the Python loop."""
import random

import numpy as np


def test_reference_noise_is_the_python_loop():
    import bench

    for seed, n in ((4, 50000), (1234, 7777)):
        random.seed(seed)
        want = bytes(random.getrandbits(8) for _ in range(n))
        assert bench.reference_noise(n, seed).tobytes() == want
    a = bench.reference_noise(4096, 4)
    assert a.dtype == np.uint8 and a.tobytes() == bench.reference_noise(8192, 4)[:4096].tobytes()


def test_golden_prefixes_of_the_full_gops():
    """tests/golden/cfg4_8f_v1.json (what bench.py checks a bounded job against): one prefix per coded picture, growing, the IDR first, the last one the whole file"""
    import hashlib
    import json
    import os

    import bench

    g = json.load(open(os.path.join(bench.ROOT, "tests", "golden", "cfg4_8f_v1.json")))
    assert {"cfg3_1080p_closedgop_medium_8f_m8", "cfg4_2160p_closedgop_medium_8f_m8"} <= set(g)  # (+ the same clips at presets slow / placebo: bench.py --preset)
    for name, r in g.items():
        p = r["after_picture"]
        assert len(p) == r["frames"] == 8 and [q["idr"] for q in p] == [1] + [0] * 7
        assert all(a["bytes"] < b["bytes"] for a, b in zip(p, p[1:])) and (p[-1]["bytes"], p[-1]["md5"]) == (r["bytes"], r["md5"])
        preset = r["cli"][1]
        assert name.split("_")[3] == preset and bench.golden_prefix(r["w"], r["h"], 8, 8, preset)[0] == name and bench.golden_prefix(r["w"], r["h"], 8, 1, preset) == (None, None)
        fake = {"after_picture": [{"bytes": 3, "md5": hashlib.md5(b"abc").hexdigest()}, {"bytes": 5, "md5": hashlib.md5(b"abcde").hexdigest()}]}
        assert bench.check_prefix(b"abc", fake) == 1 and bench.check_prefix(b"abcde", fake) == 2 and bench.check_prefix(b"abd", fake) == 0 and bench.check_prefix(b"abcd", fake) == 0


def test_the_cpu_baseline_counts_the_cores_the_container_grants():
    import bench

    h = bench.host_info()
    assert 1 <= h["cores_available"] <= h["usable_cores"] and (h["cgroup_cpu_quota"] is None or h["cores_available"] <= h["cgroup_cpu_quota"])


def test_a_bench_step_is_a_fixed_share_of_a_picture():
    """--steps sets how many timed steps run: a step's lockstep CTU steps follow from the picture alone (36 at 3840x2160, 10 at 1920x1080), never from --steps / --warmup"""
    import bench

    assert bench.step_ctus(302) == 36 and bench.step_ctus(90) == 10 and bench.step_ctus(6) == 1


def test_a_dump_always_holds_the_picture_the_steps_left_part_way():
    """--dump-outputs runs on to the end of the picture the last step reached into: never zero pictures, never a picture cut short"""
    import bench

    for per_picture in (6, 90, 302):
        for run_steps in range(1, 8 * per_picture + 1):
            P, rest = bench.pictures_done(run_steps, per_picture)
            assert P >= 1 and 0 <= rest < per_picture and (run_steps + rest) == P * per_picture
    assert bench.pictures_done(900, 302) == (3, 6) and bench.pictures_done(72, 302) == (1, 230)


class _Enc:
    def __init__(self, streams):
        self.streams, self.flushed = streams, 0

    def flush(self):
        self.flushed += 1

    def bitstream(self, g):
        return self.streams[g]


def test_dump_outputs_writes_small_float_arrays(tmp_path):
    """--dump-outputs: float arrays only, the same for the same bitstreams, well under 64 MB; the sample GOPs do not depend on the batch size"""
    import bench

    r = np.random.default_rng(0)
    encs = [_Enc([r.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in r.integers(1, 500, 150)]) for _ in range(2)]
    bench.dump_outputs(str(tmp_path / "a"), encs, [150, 150], 3)
    bench.dump_outputs(str(tmp_path / "b"), encs, [150, 150], 3)
    assert all(e.flushed == 2 for e in encs)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["bitstream_byte_sum.npy", "bitstream_bytes.npy", "bitstream_sample.npy", "bitstream_sample_crc32.npy", "bitstream_sample_gops.npy",
                     "gops_per_batch.npy", "pictures.npy"]
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)
        total += a.nbytes
    assert total < 64 << 20
    flat = [s for e in encs for s in e.streams]
    assert np.load(tmp_path / "a" / "bitstream_bytes.npy").tolist() == [len(s) for s in flat]
    assert np.load(tmp_path / "a" / "pictures.npy").tolist() == [3] and np.load(tmp_path / "a" / "gops_per_batch.npy").tolist() == [150, 150]
    gops = np.load(tmp_path / "a" / "bitstream_sample_gops.npy").astype(int).tolist()
    assert gops[0] == 0 and len(set(gops)) == 16 and gops == [g for g in bench.DUMP_SAMPLE_GOPS if g < 300]
    sample = np.load(tmp_path / "a" / "bitstream_sample.npy")
    for k, g in enumerate(gops):
        assert set(sample[k].astype(int).tolist()) <= set(flat[g])
    # a smaller batch keeps the same sample GOPs, those it still has
    bench.dump_outputs(str(tmp_path / "c"), encs[:1], [150], 3)
    assert np.load(tmp_path / "c" / "bitstream_sample_gops.npy").astype(int).tolist() == [g for g in gops if g < 150]


def test_a_dump_never_silently_holds_nothing(tmp_path):
    import pytest

    import bench

    with pytest.raises(RuntimeError):
        bench.dump_outputs(str(tmp_path / "a"), [_Enc([b"abc", b"de"])], [2], 0)
    with pytest.raises(RuntimeError):
        bench.dump_outputs(str(tmp_path / "b"), [_Enc([b"abc", b""])], [2], 1)
