"""The messages the MD5 leaf is held to hashlib on (xeve_hip_md5_planes on the GPU: tests/test_md5_gpu.py; the same lane code on the host: tests/test_md5_core_host.py).
A job is (offset, stride, w, h) in 16-bit samples over one pool of random samples; its message is the h rows of w samples, joined."""
import hashlib

import numpy as np

# (w, h): message lengths around the padding branches -- 2, 54, 56, 62, 64, 66, 120 and 128 bytes: one block, the two-block finish (from 56 bytes on the bit count
# needs a block of its own), an exact multiple of the block
PADDING_SHAPES = [(1, 1), (27, 1), (28, 1), (31, 1), (32, 1), (33, 1), (60, 1), (64, 1)]
# rows that straddle blocks: the chroma planes of 8x8, 24x40, 200x8, 72x120 and 120x72 pictures (at 8x8 a chroma row is 8 bytes: one block spans eight rows)
STRADDLE_SHAPES = [(4, 4), (12, 20), (100, 4), (36, 60), (60, 36)]
JOB_DTYPE = [("offset", "<i8"), ("stride", "<i4"), ("w", "<i4"), ("h", "<i4"), ("reserved", "<i4")]  # xeve_hip_md5_job


class Pool:
    """jobs laid one behind the other over random samples; every sample between and around the rows is random fill no digest may see"""

    def __init__(self, seed):
        self.rng, self.jobs, self.size = np.random.default_rng(seed), [], 1  # (sample 0 stays free: the list can be rebased by one sample)

    def add(self, w, h, stride=None, align=1, phase=0):
        """a job of h rows of w samples, rows `stride` apart, its first sample at an offset that is `phase` modulo `align`"""
        stride = w if stride is None else stride
        assert stride >= w >= 1 and h >= 1
        off = self.size + (phase - self.size) % align
        self.jobs.append((off, stride, w, h))
        self.size = off + (h - 1) * stride + w + int(self.rng.integers(0, 4))
        return self

    def finish(self):
        samples = self.rng.integers(0, 65536, size=self.size, dtype=np.uint16)
        return self.jobs, samples


def expected(samples, job):
    off, stride, w, h = job
    return hashlib.md5(b"".join(samples[off + r * stride:off + r * stride + w].astype("<u2").tobytes() for r in range(h))).digest()


def records(jobs, shift=0):
    a = np.zeros(len(jobs), dtype=JOB_DTYPE)
    for i, (off, stride, w, h) in enumerate(jobs):
        a[i] = (off - shift, stride, w, h, 0)
    return a


def small_cases(seed=11):
    """every listed shape three ways -- dense rows on a 16-byte boundary, rows `stride` > w apart with fill between them, rows at an odd sample offset -- and rows that
    take each of the reader's paths: whole blocks on 16-byte boundaries, on 4-byte boundaries only, on 2-byte boundaries only"""
    p = Pool(seed)
    for w, h in PADDING_SHAPES + STRADDLE_SHAPES:
        p.add(w, h, align=8)
        p.add(w, h, stride=w + 3, align=2)
        p.add(w, h, stride=w + (w & 1) + 2, align=2, phase=1)
    p.add(64, 3, stride=72, align=8)            # 16-byte aligned rows of two whole blocks
    p.add(96, 5, stride=104, align=8)           # three blocks per row
    p.add(64, 3, stride=66, align=8, phase=2)   # 4-byte aligned rows
    p.add(64, 3, stride=66, align=8, phase=3)   # 2-byte aligned rows
    p.add(80, 4, stride=88, align=8)            # a row of two and a half blocks: whole blocks and straddling ones in turn
    return p.finish()


def mixed_cases(n=130, seed=12):
    """n jobs of mixed lengths in one launch: partial last wave, lanes that end at different times"""
    p = Pool(seed)
    r = np.random.default_rng(seed + 1)
    for _ in range(n):
        w, h = int(r.integers(1, 71)), int(r.integers(1, 10))
        p.add(w, h, stride=w + int(r.integers(0, 6)), align=int(r.choice([1, 2, 8])))
    return p.finish()


def luma_1080p_case(seed=13):
    """one 1920x1080 luma plane inside a padded store (stride 1920 + 288, rows of 60 whole blocks on 16-byte boundaries): 64800 blocks, many rows, a plane of more
    than 2^22 bytes; beside it the same shape one sample further on (2-byte alignment only: the sample-by-sample reader over the same length)"""
    p = Pool(seed).add(1920, 1080, stride=1920 + 288, align=8)
    off, stride, w, h = p.jobs[0]
    p.jobs.append((off + 1, stride, w, h))
    p.size += 8
    return p.finish()
