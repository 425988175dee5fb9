"""GPU suite: the batched device API (planes resident in HBM, many blocks per launch) against the oracle on
seeded inputs, and -- at the full 3840x2160 size of the headline config -- through size-independent properties."""
import numpy as np
import pytest

from _libs import oracle, ptr

pytestmark = pytest.mark.gpu

PAD = 144  # luma padding of a reference picture plane (reference: src_base/xeve_def.h:380)


@pytest.fixture(scope="module")
def dev():
    import torch

    import xeve_amd

    xeve_amd.init(0)
    return torch.device("cuda:0")


def make_planes(r, W, H, bd=10, pad=PAD):
    s = W + 2 * pad
    org = r.integers(0, 1 << bd, size=(H + 2 * pad, s), dtype=np.int16)
    ref = r.integers(0, 1 << bd, size=(H + 2 * pad, s), dtype=np.int16)
    return org, ref, s


def diamond(s_ref, rng_steps=(4, 8, 16, 32, 64)):
    """candidate geometry of one me_ipel_diamond pass (reference: src_base/xeve_pinter.c:363-551): dense 5x5,
    then 4-point / 8-point / 16-point diamonds at growing L1 radius"""
    c = [(dx, dy) for dy in range(-2, 3) for dx in range(-2, 3)]
    for st in rng_steps:
        if st == 4:
            c += [(0, -4), (-4, 0), (4, 0), (0, 4), (0, 0)]
        else:
            n = 8 if st == 8 else 16
            q = n // 4
            for i in range(n):
                a, b = i % q, i // q
                dx, dy = [(a, -(q - a)), (q - a, a), (-a, q - a), (-(q - a), -a)][b]
                c.append((dx * st // q, dy * st // q))
            c.append((0, 0))
    return np.array([dy * s_ref + dx for dx, dy in c], np.int32), c


@pytest.mark.parametrize("size", [8, 16, 32, 64])
@pytest.mark.parametrize("signed", [False, True])
def test_sad_jobs_vs_oracle(dev, size, signed):
    import torch

    from xeve_amd import device as D

    r = np.random.default_rng(100 + size)
    W, H, bd = 256, 192, 10
    org, ref, s = make_planes(r, W, H, bd)
    if signed:
        org = (2 * org.astype(np.int32) - r.integers(0, 1024, size=org.shape)).astype(np.int16)
    cand, _ = diamond(s)
    offs1, offs2 = [], []
    for y in range(0, H, size):
        for x in range(0, W, size):
            offs1.append((PAD + y) * s + PAD + x)
            offs2.append((PAD + y + int(r.integers(-8, 9))) * s + PAD + x + int(r.integers(-8, 9)))
    jobs = D.make_jobs(offs1, offs2, dev)
    got = D.sad_jobs(torch.from_numpy(org).to(dev), s, torch.from_numpy(ref).to(dev), s, jobs, torch.from_numpy(cand).to(dev),
                     size, size, bd, signed=signed).cpu().numpy()
    d_ref = torch.from_numpy(ref).to(dev)
    dual = D.sad_jobs_dual(torch.from_numpy(org).to(dev), s, d_ref, D.plane_shift1(d_ref), s, jobs, torch.from_numpy(cand).to(dev),
                           size, size, bd, signed=signed).cpu().numpy()
    assert np.array_equal(dual, got)  # alignment-optimised form: same numbers
    O = oracle()
    pick = r.choice(len(offs1), size=min(24, len(offs1)), replace=False)
    for j in pick:
        for c in range(len(cand)):
            exp = O.xo_sad(size, size, ptr(org, offs1[j]), ptr(ref, offs2[j] + int(cand[c])), s, s, bd)
            assert got[j, c] == exp, (size, j, c)


@pytest.mark.parametrize("w,h", [(8, 8), (16, 16), (32, 32), (64, 64), (4, 4), (16, 8), (8, 32), (4, 8), (2, 2), (128, 64)])
def test_ssd_satd_diff_jobs_vs_oracle(dev, w, h):
    import torch

    from xeve_amd import device as D

    r = np.random.default_rng(200 + w * 7 + h)
    org, ref, s = make_planes(r, 256, 128, 10, pad=16)
    offs1 = [(16 + int(r.integers(0, 128 - h))) * s + 16 + int(r.integers(0, 256 - w)) for _ in range(40)]
    offs2 = [(16 + int(r.integers(0, 128 - h))) * s + 16 + int(r.integers(0, 256 - w)) for _ in range(40)]
    cand = np.array([0, 1, -1, s, -s, 3 * s + 2], np.int32)
    d_org, d_ref = torch.from_numpy(org).to(dev), torch.from_numpy(ref).to(dev)
    jobs, d_cand = D.make_jobs(offs1, offs2, dev), torch.from_numpy(cand).to(dev)
    ssd = D.ssd_jobs(d_org, s, d_ref, s, jobs, d_cand, w, h, 10).cpu().numpy()
    satd = D.satd_jobs(d_org, s, d_ref, s, jobs, d_cand, w, h, 10).cpu().numpy()
    sad = D.sad_jobs(d_org, s, d_ref, s, jobs, d_cand, w, h, 10).cpu().numpy()
    diff = D.diff_jobs(d_org, s, d_ref, s, jobs, w, h).cpu().numpy()
    O = oracle()
    for j in range(40):
        for c in range(len(cand)):
            a, b = ptr(org, offs1[j]), ptr(ref, offs2[j] + int(cand[c]))
            assert sad[j, c] == O.xo_sad(w, h, a, b, s, s, 10)
            assert ssd[j, c] == O.xo_ssd(w, h, a, b, s, s, 10)
            assert satd[j, c] == O.xo_satd(w, h, a, b, s, s, 10), (w, h, j, c)
        e = np.zeros((h, w), np.int16)
        O.xo_diff(w, h, ptr(org, offs1[j]), ptr(ref, offs2[j]), s, s, w, ptr(e))
        assert np.array_equal(diff[j], e)


@pytest.mark.parametrize("luma", [True, False])
def test_mc_jobs_vs_oracle(dev, luma):
    import torch

    from xeve_amd import device as D

    r = np.random.default_rng(300 + luma)
    O = oracle()
    pad = 72
    W, H = 192, 128
    s = W + 2 * pad
    ref = r.integers(0, 1024, size=(H + 2 * pad, s), dtype=np.int16)
    d_ref = torch.from_numpy(ref).to(dev)
    unit = 16 if luma else 32
    for (w, h) in ([(8, 8), (16, 16), (32, 32), (64, 64), (64, 16)] if luma else [(4, 4), (8, 8), (16, 16), (32, 32), (8, 32)]):
        n = 48
        gx = [(pad + int(r.integers(-40, W + 40 - w))) * unit + int(r.integers(0, unit // 4)) * 4 for _ in range(n)]
        gy = [(pad + int(r.integers(-40, H + 40 - h))) * unit + int(r.integers(0, unit // 4)) * 4 for _ in range(n)]
        frac = [int((x & (unit - 1)) != 0) | (int((y & (unit - 1)) != 0) << 1) for x, y in zip(gx, gy)]
        pred = torch.full((n, h, w), -1, dtype=torch.int16, device=dev)
        D.mc_jobs(luma, d_ref, s, pred, w, D.make_mc_jobs(gx, gy, [i * w * h for i in range(n)], frac, dev), w, h, 10)
        got = pred.cpu().numpy()
        for i in range(n):
            e = np.zeros((h, w), np.int16)
            (O.xo_mc_l if luma else O.xo_mc_c)(frac[i] & 1, frac[i] >> 1, ptr(ref), gx[i], gy[i], s, w, ptr(e), w, h, 10,
                                               O.mc_l_coeff if luma else O.mc_c_coeff)
            assert np.array_equal(got[i], e), (luma, w, h, i, gx[i] & (unit - 1), gy[i] & (unit - 1))


@pytest.mark.parametrize("lw,lh", [(1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (6, 6), (3, 5), (6, 3), (4, 6)])
def test_tq_chain_vs_oracle(dev, lw, lh):
    import torch

    from xeve_amd import device as D

    r = np.random.default_rng(400 + lw * 8 + lh)
    O = oracle()
    n, nblk, bd = 1 << (lw + lh), 24, 10
    resid = r.integers(-1023, 1024, size=(nblk, n), dtype=np.int16)
    resid[0] = 0
    resid[1] = 1023
    resid[2] = -1023
    resid[3, :] = r.integers(-3, 4, size=n)  # a block the RDOQ pre-test zeroes
    for qp, intra in ((22, 0), (32, 1), (45, 0)):
        qs, dqs = D.QUANT_SCALE[0][qp % 6], D.DQ_SCALE[qp % 6] << (qp // 6)
        d = torch.from_numpy(resid).to(dev)
        D.trans(d, lw, lh, bd)
        fwd = d.cpu().numpy().copy()
        d2 = d.clone()
        coded = D.rdoq_zero_test(d2, lw, lh, qp, qs, intra, bd).cpu().numpy()
        zt = d2.cpu().numpy()
        nnz = D.quant(d, lw, lh, qp, qs, intra, bd).cpu().numpy()
        q = d.cpu().numpy().copy()
        D.dquant(d, lw, lh, dqs, bd)
        dq = d.cpu().numpy().copy()
        D.itrans(d, lw, lh, bd)
        inv = d.cpu().numpy()
        for b in range(nblk):
            e = resid[b].copy()
            O.xo_trans(ptr(e), lw, lh, bd)
            assert np.array_equal(fwd[b], e), ("trans", b)
            c_exp = O.xo_rdoq_zero_test(ptr(e), lw, lh, qp, qs, intra, bd)
            assert coded[b] == c_exp
            assert np.array_equal(zt[b], e if c_exp else np.zeros_like(e))
            assert nnz[b] == O.xo_quant(ptr(e), lw, lh, qp, qs, intra, bd)
            assert np.array_equal(q[b], e), ("quant", b)
            O.xo_dquant(ptr(e), lw, lh, dqs, bd)
            assert np.array_equal(dq[b], e), ("dquant", b)
            O.xo_itrans(ptr(e), lw, lh, bd)
            assert np.array_equal(inv[b], e), ("itrans", b)


def test_avg_recon_vs_oracle(dev):
    import torch

    from xeve_amd import device as D

    r = np.random.default_rng(500)
    O = oracle()
    a = r.integers(0, 1024, size=4099, dtype=np.int16)
    b = r.integers(0, 1024, size=4099, dtype=np.int16)
    got = D.avg(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)).cpu().numpy()
    e = np.zeros_like(a)
    O.xo_avg(ptr(a), ptr(b), ptr(e), 4099, 4099, 4099, 4099, 1)
    assert np.array_equal(got, e)
    nblk, w = 10, 16
    coef = r.integers(-40000, 40000, size=(nblk, w * w)).astype(np.int16)
    pred = r.integers(0, 1024, size=(nblk, w * w), dtype=np.int16)
    is_coef = np.array([i % 3 != 0 for i in range(nblk)], np.uint8)
    s_rec = 200
    rec_off = np.array([i * w for i in range(nblk)], np.int32)
    rec = torch.zeros((w, s_rec), dtype=torch.int16, device=dev)
    D.recon(torch.from_numpy(coef).to(dev), torch.from_numpy(pred).to(dev), torch.from_numpy(is_coef).to(dev), w, w,
            torch.from_numpy(rec_off).to(dev), s_rec, rec, 10)
    got = rec.cpu().numpy()
    for i in range(nblk):
        e = np.zeros((w, s_rec), np.int16)
        O.xo_recon(ptr(coef, i * w * w), ptr(pred, i * w * w), int(is_coef[i]), w, w, s_rec, ptr(e), 10)
        assert np.array_equal(got[:, i * w:(i + 1) * w], e[:, :w])


# ---------------------------------------------------------------------------------------------------------
# full-size (3840x2160) properties: no oracle at this size, identities of the arithmetic instead
# ---------------------------------------------------------------------------------------------------------
def test_full_size_properties_4k(dev):
    import torch

    from xeve_amd import device as D

    W, H, bd = 3840, 2160, 10
    s = W + 2 * PAD
    g = torch.Generator(device=dev).manual_seed(4)
    org = torch.randint(0, 1024, (H + 2 * PAD, s), generator=g, device=dev, dtype=torch.int16)
    ref = torch.randint(0, 1024, (H + 2 * PAD, s), generator=g, device=dev, dtype=torch.int16)
    ys, xs = np.meshgrid(np.arange(0, H - 63, 64), np.arange(0, W, 64), indexing="ij")
    off64 = ((PAD + ys) * s + PAD + xs).ravel().astype(np.int32)
    cand = torch.tensor([0, 1, -s, 5 * s - 3, -64 * s + 64], dtype=torch.int32, device=dev)
    jobs64 = D.make_jobs(off64, off64, dev)
    # (1) a block against itself has zero distortion, for every size class
    z = torch.zeros(1, dtype=torch.int32, device=dev)
    for size in (8, 16, 32, 64):
        sad0 = D.sad_jobs(org, s, org, s, jobs64, z, size, size, bd)
        assert int(sad0.abs().sum()) == 0
        assert int(D.satd_jobs(org, s, org, s, jobs64, z, size, size, bd).abs().sum()) == 0
        assert int(D.ssd_jobs(org, s, org, s, jobs64, z, size, size, bd).abs().sum()) == 0
    # (2) SAD is additive over a quad-tree split BEFORE the final shift: at bit depth 8 (shift 0) the 64x64 SAD
    #     equals the sum of its four 32x32 SADs, which equal the sums of their 16x16 and 8x8 SADs  
    sad64 = D.sad_jobs(org, s, ref, s, jobs64, cand, 64, 64, 8).to(torch.int64)
    for size in (32, 16, 8):
        k = 64 // size
        sub = (off64[:, None, None] + (np.arange(k)[None, :, None] * size * s) + np.arange(k)[None, None, :] * size).reshape(-1)
        jobs = D.make_jobs(sub, sub, dev)
        part = D.sad_jobs(org, s, ref, s, jobs, cand, size, size, 8).to(torch.int64)
        assert torch.equal(part.view(len(off64), k * k, -1).sum(1), sad64), size
    # (3) SSD at bit depth 8 equals the sum of squares of DIFF; recon(diff, pred) returns the original
    ssd64 = D.ssd_jobs(org, s, ref, s, jobs64, z, 64, 64, 8)
    diff = D.diff_jobs(org, s, ref, s, jobs64, 64, 64)
    assert torch.equal((diff.to(torch.int64) ** 2).sum((1, 2)), ssd64[:, 0])
    pred = torch.empty((len(off64), 64, 64), dtype=torch.int16, device=dev)
    mcj = D.make_mc_jobs(((off64 % s)) * 16, (off64 // s) * 16, np.arange(len(off64)) * 4096, np.zeros(len(off64)), dev)
    D.mc_jobs(True, ref, s, pred, 64, mcj, 64, 64, bd)  # integer-pel MC is a copy
    rec = torch.zeros_like(org)
    D.recon(diff.view(len(off64), -1), pred.view(len(off64), -1), None, 64, 64, torch.from_numpy(off64).to(dev), s, rec, bd)
    tiles = lambda p: torch.stack([p[PAD + y:PAD + y + 64, PAD + x:PAD + x + 64] for y, x in zip(ys.ravel()[:50], xs.ravel()[:50])])
    assert torch.equal(tiles(rec), tiles(org))
    assert torch.equal(pred[:50], tiles(ref))
    # (4) transform linearity / structure on all 64x64 residual tiles of the picture: T(0) = 0, the 64-point
    #     transform only populates the 32x32 low-frequency corner, and T(-x) = -T(x) up to the rounding offset
    x = diff.view(len(off64), -1).clone()
    D.trans(x, 6, 6, bd)
    c = x.view(-1, 64, 64)
    assert int(c[:, 32:, :].abs().sum()) == 0 and int(c[:, :, 32:].abs().sum()) == 0 and int(c[:, :32, :32].abs().sum()) > 0
    xn = (-diff).view(len(off64), -1).clone()
    D.trans(xn, 6, 6, bd)
    assert int((x.to(torch.int32) + xn.to(torch.int32)).abs().max()) <= 1
    zero = torch.zeros((4, 4096), dtype=torch.int16, device=dev)
    assert int(D.trans(zero, 6, 6, bd).abs().sum()) == 0
    # (5) avg(a, a) = a over the whole padded plane
    assert torch.equal(D.avg(org.view(-1), org.view(-1)), org.view(-1))
    torch.cuda.synchronize()


@pytest.mark.parametrize("lg", [5, 6])
def test_dct_matrix_core_path_full_int16_range(dev, lg):
    """32x32 / 64x64 run on v_mfma_i32_32x32x32_i8 with byte-split operands (xeve_amd/csrc/dct_mfma.hip): exact for
    EVERY int16 input, including the extremes that stress the byte split and the offset-binary correction terms."""
    import torch

    from xeve_amd import device as D

    r = np.random.default_rng(600 + lg)
    O = oracle()
    n = 1 << (2 * lg)
    x = r.integers(-32768, 32768, size=(12, n), dtype=np.int16)
    x[0], x[1], x[2], x[3] = 32767, -32768, 0, 1
    x[4, ::2], x[4, 1::2] = 32767, -32768
    x[5] = (np.arange(n) % 251 - 125) * 262  # smooth-ish, asymmetric: catches transposed layouts
    d = torch.from_numpy(x).to(dev)
    D.trans(d, lg, lg, 10)
    got = d.cpu().numpy()
    for b in range(12):
        e = x[b].copy()
        O.xo_trans(ptr(e), lg, lg, 10)
        assert np.array_equal(got[b], e), ("fwd", lg, b)
    d = torch.from_numpy(x).to(dev)
    D.itrans(d, lg, lg, 10)
    got = d.cpu().numpy()
    for b in range(12):
        e = x[b].copy()
        O.xo_itrans(ptr(e), lg, lg, 10)
        assert np.array_equal(got[b], e), ("inv", lg, b)


@pytest.mark.parametrize("lw,lh", [(1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (6, 6), (2, 4), (5, 3), (6, 5)])
def test_fused_residual_rdo_vs_oracle(dev, lw, lh):
    """xeve_hip_residual_rdo = DIFF, SSD, DCT, zero pre-test, quant, dequant, IDCT, recon, SSD in one launch
    (matrix cores for 32x32 / 64x64) against the oracle's step-by-step chain."""
    import torch

    from xeve_amd import device as D

    r = np.random.default_rng(700 + lw * 8 + lh)
    O = oracle()
    w, h, bd = 1 << lw, 1 << lh, 10
    n, nblk = w * h, 21
    s = 4 * 64 + 32
    org = r.integers(0, 1024, size=(6 * 64 + 16, s), dtype=np.int16)
    pred = r.integers(0, 1024, size=(nblk, n), dtype=np.int16)
    offs = [(8 + (b // 4) * h) * s + 8 + (b % 4) * w for b in range(nblk)]
    for b in (0, 1, 2):  # near-perfect predictions: exercise the all-zero pre-test and small levels
        blk = org.reshape(-1)[np.add.outer(np.arange(h) * s, np.arange(w)).ravel() + offs[b]]
        pred[b] = np.clip(blk + r.integers(-b - 1, b + 2, size=n), 0, 1023)
    for qp, intra, zt in ((27, 0, 1), (37, 1, 1), (32, 0, 0)):
        d_org, d_pred = torch.from_numpy(org).to(dev), torch.from_numpy(pred).to(dev)
        jobs = D.make_jobs(offs, np.arange(nblk) * n, dev)
        coef = torch.full((nblk, n), 77, dtype=torch.int16, device=dev)
        rec = torch.zeros_like(d_org)
        nnz = torch.zeros(nblk, dtype=torch.int32, device=dev)
        ssd = torch.zeros((nblk, 2), dtype=torch.int64, device=dev)
        D.residual_rdo(d_org, s, d_pred, w, jobs, lw, lh, bd, qp, intra, zt, coef, rec, s, nnz, ssd)
        coef, rec, nnz, ssd = coef.cpu().numpy(), rec.cpu().numpy(), nnz.cpu().numpy(), ssd.cpu().numpy()
        qs, dqs = D.QUANT_SCALE[0][qp % 6], D.DQ_SCALE[qp % 6] << (qp // 6)
        for b in range(nblk):
            c = np.zeros(n, np.int16)
            O.xo_diff(w, h, ptr(org, offs[b]), ptr(pred, b * n), s, w, w, ptr(c))
            assert ssd[b, 0] == O.xo_ssd(w, h, ptr(org, offs[b]), ptr(pred, b * n), s, w, bd)
            O.xo_trans(ptr(c), lw, lh, bd)
            if zt and not O.xo_rdoq_zero_test(ptr(c), lw, lh, qp, qs, intra, bd):
                c[:] = 0
                e_nnz = 0
            else:
                e_nnz = O.xo_quant(ptr(c), lw, lh, qp, qs, intra, bd)
            assert nnz[b] == e_nnz and np.array_equal(coef[b], c), ("levels", lw, lh, qp, b)
            O.xo_dquant(ptr(c), lw, lh, dqs, bd)
            O.xo_itrans(ptr(c), lw, lh, bd)
            e = np.zeros((h, s), np.int16)
            O.xo_recon(ptr(c), ptr(pred, b * n), 1, w, h, s, ptr(e), bd)
            y0, x0 = offs[b] // s, offs[b] % s
            assert np.array_equal(rec[y0:y0 + h, x0:x0 + w], e[:, :w]), ("rec", lw, lh, qp, b)
            assert ssd[b, 1] == O.xo_ssd(w, h, ptr(org, offs[b]), ptr(rec, offs[b]), s, s, bd)


@pytest.mark.parametrize("luma", [True, False])
def test_fused_mc_distortion_vs_oracle(dev, luma):
    """xeve_hip_mc_l_sad_jobs / xeve_hip_mc_ssd_jobs: interpolate and compare with the original in one launch."""
    import torch

    from xeve_amd import device as D

    r = np.random.default_rng(800 + luma)
    O = oracle()
    pad, W, H = 72, 192, 128
    s = W + 2 * pad
    ref = r.integers(0, 1024, size=(H + 2 * pad, s), dtype=np.int16)
    org = r.integers(0, 1024, size=(H + 2 * pad, s), dtype=np.int16)
    d_ref, d_org = torch.from_numpy(ref).to(dev), torch.from_numpy(org).to(dev)
    unit = 16 if luma else 32
    for (w, h) in ([(8, 8), (16, 16), (32, 32), (64, 64)] if luma else [(4, 4), (8, 8), (16, 16), (32, 32)]):
        n = 70
        gx = [(pad + int(r.integers(-30, W + 30 - w))) * unit + int(r.integers(0, unit // 4)) * 4 for _ in range(n)]
        gy = [(pad + int(r.integers(-30, H + 30 - h))) * unit + int(r.integers(0, unit // 4)) * 4 for _ in range(n)]
        frac = [int((x & (unit - 1)) != 0) | (int((y & (unit - 1)) != 0) << 1) for x, y in zip(gx, gy)]
        ooff = [(pad + int(r.integers(0, H - h))) * s + pad + int(r.integers(0, W - w)) for _ in range(n)]
        jobs = D.make_mc_jobs(gx, gy, ooff, frac, dev)
        ssd = D.mc_ssd_jobs(luma, d_ref, s, d_org, s, jobs, w, h, 10, torch.zeros(n, dtype=torch.int64, device=dev)).cpu().numpy()
        sad = D.mc_l_sad_jobs(d_ref, s, d_org, s, jobs, w, h, 10, torch.zeros(n, dtype=torch.int32, device=dev)).cpu().numpy() if luma else None
        for i in range(n):
            e = np.zeros((h, w), np.int16)
            (O.xo_mc_l if luma else O.xo_mc_c)(frac[i] & 1, frac[i] >> 1, ptr(ref), gx[i], gy[i], s, w, ptr(e), w, h, 10,
                                               O.mc_l_coeff if luma else O.mc_c_coeff)
            assert ssd[i] == O.xo_ssd(w, h, ptr(org, ooff[i]), ptr(e), s, w, 10), (luma, w, i)
            if luma:
                assert sad[i] == O.xo_sad(w, h, ptr(org, ooff[i]), ptr(e), s, w, 10), (w, i)


# ---------------------------------------------------------------------------------------------------------
# far offsets: every kernel that decodes a job record (xh_common.h xh_job / xh_pred_off), at blocks of plane 1 that
# lie 2^31, 2^32 and almost 2^33 samples in -- where the stacked originals of a real batch are (tests/test_job_records.py
# holds the decode itself to its domain on the CPU)
# ---------------------------------------------------------------------------------------------------------
FAR_GUARD = 2 ** 31  # samples in front of plane 1: a sign-extended off1 lands here, inside the allocation -- a mismatch, not a fault
FAR_SPAN = 2 ** 33   # what the halved records address
FAR_TAIL = 1 << 16   # behind it: room for the window the residual tests watch behind the last block
FAR_S1 = 1312        # stride of plane 1: the padded 1024-wide picture's
HALF2, HALFF = 1 << 30, 1 << 8  # XH_OFF2_HALF, XH_FRAC_HALF


class FarPlane:
    """an int16 buffer of 2^31 + 2^33 samples that nothing fills; positions are samples relative to p1 = base + 2^31"""

    def __init__(self, dev):
        import torch

        self.dev = dev
        self.base = torch.empty(FAR_GUARD + FAR_SPAN + FAR_TAIL, dtype=torch.int16, device=dev)
        self.p1 = self.base[FAR_GUARD:]

    def inside(self, pos, w, h):
        return pos >= -FAR_GUARD and pos + (h - 1) * FAR_S1 + w <= FAR_SPAN

    def put(self, pos, blk):
        import torch

        h, w = blk.shape
        self.base.as_strided((h, w), (FAR_S1, 1), FAR_GUARD + pos).copy_(torch.from_numpy(np.ascontiguousarray(blk)).to(self.dev))

    def get(self, pos, w, h):
        return self.base.as_strided((h, w), (FAR_S1, 1), FAR_GUARD + pos).cpu().numpy().copy()

    def put_flat(self, pos, a):
        import torch

        self.base[FAR_GUARD + pos:FAR_GUARD + pos + len(a)].copy_(torch.from_numpy(a).to(self.dev))

    def get_flat(self, pos, n):
        return self.base[FAR_GUARD + pos:FAR_GUARD + pos + n].cpu().numpy().copy()

    def free(self):
        self.base = self.p1 = None


def _far_fixture(dev):
    import torch

    f = FarPlane(dev)
    yield f
    f.free()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()  # (the 4K encodes at the end of the suite need the memory)


@pytest.fixture(scope="module")
def far(dev):
    yield from _far_fixture(dev)


@pytest.fixture(scope="module")
def far_rec(dev):
    """the reconstruction's plane of the residual chains: off1 addresses both, so it has the original's geometry"""
    yield from _far_fixture(dev)


def far_probes(w, h):
    """block positions (plain records, records marked as the library marks them); block extent = (h - 1) * s1 + w"""
    ext = (h - 1) * FAR_S1 + w
    return [(2 ** 31 - ext) & ~1, 2 ** 31 + 6, 2 ** 32 - ext - 1], [2 ** 31 + 8, 2 ** 32 + 8, (2 ** 33 - ext) & ~1]


def far_aliases(P):
    """where a wrong decode of the record for P reads: sign extension (P mod 2^32, P - 2^32; of a halved off1: P - 2^33), the doubling forgotten (P / 2), an unmarked
    record doubled (2P mod 2^33), an offset kept in 31 bits (P mod 2^31)"""
    return sorted({P % 2 ** 32, P - 2 ** 32, P - 2 ** 33, P // 2, (2 * P) % 2 ** 33, P % 2 ** 31} - {P})


def far_setup(plane, r, w, h, lo=0, hi=1024):
    """seeded blocks at every probe and OTHER seeded blocks at each of its aliases that lies inside the allocation; returns the probes and what the plane holds there
    (blocks that overlap end as the later write left them, so the reference reads them back)"""
    plain, marked = far_probes(w, h)
    assert plain[2] % 2 == 1 and all(p % 2 == 0 for p in marked) and all(plane.inside(p, w, h) for p in plain + marked)
    for P in plain + marked:
        for A in far_aliases(P):
            if plane.inside(A, w, h):
                plane.put(A, r.integers(lo, hi, size=(h, w), dtype=np.int16))
    for P in plain + marked:
        plane.put(P, r.integers(lo, hi, size=(h, w), dtype=np.int16))
    blocks = {P: plane.get(P, w, h) for P in plain + marked}
    n_alias = 0
    for P in plain + marked:
        for A in far_aliases(P):
            if plane.inside(A, w, h):
                assert not np.array_equal(plane.get(A, w, h), blocks[P]), (P, A)  # a wrong decode reads OTHER data
                n_alias += 1
    assert n_alias >= 12
    return plain, marked, blocks


def far_records(plain, marked, off2s):
    """one record per (probe, off2): (off1, off2) as the uint32 / int32 words, and the probe each belongs to"""
    rec1, rec2, where = [], [], []
    for k, P in enumerate(plain + marked):
        for o2 in off2s[k]:
            half = P in marked
            assert not half or o2 >= 0
            rec1.append(P // 2 if half else P), rec2.append(o2 | HALF2 if half else o2), where.append(P)
    assert max(rec1) >= 2 ** 31
    return rec1, rec2, where


FAR_SIZES = [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (128, 64), (16, 8), (4, 8), (8, 32)]  # one per path of sad.hip's dispatch: tiny, the four squares, any + SATD tiles 8x8 / 16x8 / 4x8 / 8x16


@pytest.mark.parametrize("w,h", FAR_SIZES)
def test_distortions_at_far_offsets_vs_oracle(dev, far, w, h):
    import torch

    from xeve_amd import device as D

    r = np.random.default_rng(900 + w * 7 + h)
    O = oracle()
    bd, pad, s2 = 10, 24, 320
    ref = r.integers(0, 1 << bd, size=(64 + 2 * pad + 16, s2), dtype=np.int16)
    mid = (pad + 8) * s2 + pad + 8  # plane 2 is handed over from here: a caller's record may carry a negative off2
    d_ref = torch.from_numpy(ref).to(dev).view(-1)
    d_p2 = d_ref[mid:]
    assert d_p2.data_ptr() % 4 == 0
    d_sh = D.plane_shift1(d_ref)[mid:]
    few = np.array([0, 1, -1, s2, -s2, 3 * s2 + 2], np.int32)
    many = diamond(s2)[0][:33]  # (>= 32 candidates: the split form of the square SAD kernels)
    assert np.abs(many).max() <= 8 * s2 + 8
    for signed in (False, True):
        plain, marked, blocks = far_setup(far, r, w, h, *((-1023, 2047) if signed else (0, 1024)))
        off2s = [[int(r.integers(0, 16)) * s2 + int(r.integers(0, 64)) for _ in range(3)] for _ in range(6)]
        for k in range(3):
            off2s[k][0] = -int(r.integers(1, 8)) * s2 - int(r.integers(0, 8))  # (plain records only: bit 31 set, never taken for the mark)
        rec1, rec2, where = far_records(plain, marked, off2s)
        jobs = D.make_jobs(rec1, rec2, dev)
        o2 = [x & (HALF2 - 1) if P in marked else x for x, P in zip(rec2, where)]
        got = {}
        for name, cand in (("few", few), ("many", many)):
            d_cand = torch.from_numpy(cand).to(dev)
            got["sad", name] = D.sad_jobs(far.p1, FAR_S1, d_p2, s2, jobs, d_cand, w, h, bd, signed=signed).cpu().numpy()
            got["dual", name] = D.sad_jobs_dual(far.p1, FAR_S1, d_p2, d_sh, s2, jobs, d_cand, w, h, bd, signed=signed).cpu().numpy()
        if not signed:
            d_cand = torch.from_numpy(few).to(dev)
            got["ssd"] = D.ssd_jobs(far.p1, FAR_S1, d_p2, s2, jobs, d_cand, w, h, bd).cpu().numpy()
            got["satd"] = D.satd_jobs(far.p1, FAR_S1, d_p2, s2, jobs, d_cand, w, h, bd).cpu().numpy()
            got["diff"] = D.diff_jobs(far.p1, FAR_S1, d_p2, s2, jobs, w, h).cpu().numpy()
        for j, P in enumerate(where):
            a = ptr(blocks[P])
            for name, cand in (("few", few), ("many", many)):
                exp = [O.xo_sad(w, h, a, ptr(ref, mid + o2[j] + int(c)), w, s2, bd) for c in cand]
                assert list(got["sad", name][j]) == exp, ("sad", signed, name, P, j)
                assert list(got["dual", name][j]) == exp, ("dual", signed, name, P, j)
            if not signed:
                assert list(got["ssd"][j]) == [O.xo_ssd(w, h, a, ptr(ref, mid + o2[j] + int(c)), w, s2, bd) for c in few], ("ssd", P, j)
                assert list(got["satd"][j]) == [O.xo_satd(w, h, a, ptr(ref, mid + o2[j] + int(c)), w, s2, bd) for c in few], ("satd", P, j)
                e = np.zeros((h, w), np.int16)
                O.xo_diff(w, h, a, ptr(ref, mid + o2[j]), w, s2, w, ptr(e))
                assert np.array_equal(got["diff"][j], e), ("diff", P, j)


def _chain_expect(O, blk, pred, lw, lh, bd, qp, intra, quantise):
    """the oracle's step-by-step residual chain of one block: levels, their count, the reconstruction and both SSDs"""
    w, h = 1 << lw, 1 << lh
    dqs = _DQ_SCALE[qp % 6] << (qp // 6)
    c = np.zeros(w * h, np.int16)
    O.xo_diff(w, h, ptr(blk), ptr(pred), w, w, w, ptr(c))
    ssd0 = O.xo_ssd(w, h, ptr(blk), ptr(pred), w, w, bd)
    O.xo_trans(ptr(c), lw, lh, bd)
    nnz = quantise(c)
    lev = c.copy()
    O.xo_dquant(ptr(c), lw, lh, dqs, bd)
    O.xo_itrans(ptr(c), lw, lh, bd)
    e = np.zeros((h, w), np.int16)
    O.xo_recon(ptr(c), ptr(pred), 1, w, h, w, ptr(e), bd)
    return lev, nnz, e, ssd0, O.xo_ssd(w, h, ptr(blk), ptr(e), w, w, bd)


_DQ_SCALE = (40, 45, 51, 57, 64, 71)


@pytest.mark.parametrize("rdoq", [False, True])
@pytest.mark.parametrize("lw,lh", [(3, 3), (5, 5), (6, 6)])  # tq.hip's chain; dct_mfma.hip's at 32x32 and at 64x64
def test_residual_chains_at_far_offsets_vs_oracle(dev, far, far_rec, lw, lh, rdoq):
    """off1 addresses the original AND the reconstruction: the reconstructed block lands at the far position of a second plane of the same geometry, and not one sample
    around it -- a stride and 16 samples before the block to a stride and 16 behind it -- nor at any alias of the position changes"""
    import ctypes as C

    import torch

    from _libs import oracle_rdoq
    from _rdoq_cases import make_est
    from xeve_amd import device as D
    from xeve_amd import lib

    r = np.random.default_rng(1000 + lw * 8 + lh + 64 * rdoq)
    O, OR = oracle(), oracle_rdoq()
    w, h, bd, n = 1 << lw, 1 << lh, 10, 1 << (lw + lh)
    ext = (h - 1) * FAR_S1 + w
    plain, marked, blocks = far_setup(far, r, w, h)
    qp, intra, lam, luma = (27, 0, 38.5, 1) if rdoq else (32, 1, 0.0, 1)
    qs = D.QUANT_SCALE[0][qp % 6]
    est = make_est(r) if rdoq else None

    def quantise(c):
        if not O.xo_rdoq_zero_test(ptr(c), lw, lh, qp, qs, intra, bd):
            c[:] = 0
            return 0
        return OR.xo_rdoq(ptr(c), lw, lh, qp, lam, luma, bd, 0, C.byref(est)) if rdoq else O.xo_quant(ptr(c), lw, lh, qp, qs, intra, bd)

    coded = 0
    for probes, half in ((plain, False), (marked, True)):  # (a launch each: the blocks at 2^31 + 6 and 2^31 + 8 overlap)
        # predictions: a near-perfect one (the zero pre-test and small levels), a fair one, and one that has nothing to do with the block (large levels)
        pred = np.stack([np.clip(blocks[P] + r.integers(-40 * k - 2, 40 * k + 3, size=(h, w)), 0, 1023).astype(np.int16).reshape(-1) for k, P in enumerate(probes)])
        pred[2] = r.integers(0, 1024, size=n, dtype=np.int16)
        jobs = D.make_jobs([P // 2 if half else P for P in probes], [k * n | (HALF2 if half else 0) for k in range(3)], dev)
        # what is watched in the reconstruction's plane: a window around every block and every alias block inside the allocation
        windows = [(P - FAR_S1 - 16, ext + 2 * FAR_S1 + 32) for P in probes]
        windows += [(A, ext) for P in probes for A in far_aliases(P) if far_rec.inside(A, w, h)]
        for start, length in windows:
            far_rec.put_flat(start, r.integers(-3000, -2000, size=length, dtype=np.int16))
        before = [far_rec.get_flat(start, length) for start, length in windows]
        coef = torch.full((3, n), 77, dtype=torch.int16, device=dev)
        nnz = torch.zeros(3, dtype=torch.int32, device=dev)
        ssd = torch.zeros((3, 2), dtype=torch.int64, device=dev)
        d_pred = torch.from_numpy(pred).to(dev)
        if rdoq:
            D.residual_rdoq(far.p1, FAR_S1, d_pred, w, jobs, lw, lh, bd, qp, intra, lam, luma, lib.RdoqEst.from_buffer_copy(bytes(est)), coef, far_rec.p1, FAR_S1, nnz, ssd)
        else:
            D.residual_rdo(far.p1, FAR_S1, d_pred, w, jobs, lw, lh, bd, qp, intra, 1, coef, far_rec.p1, FAR_S1, nnz, ssd)
        coef, nnz, ssd = coef.cpu().numpy(), nnz.cpu().numpy(), ssd.cpu().numpy()
        recs = {}
        for k, P in enumerate(probes):
            lev, e_nnz, e, ssd0, ssd1 = _chain_expect(O, blocks[P], pred[k], lw, lh, bd, qp, intra, quantise)
            assert nnz[k] == e_nnz and np.array_equal(coef[k], lev), ("levels", half, P)
            assert (ssd[k, 0], ssd[k, 1]) == (ssd0, ssd1), ("ssd", half, P)
            assert np.array_equal(far_rec.get(P, w, h), e), ("rec", half, P)
            recs[P] = e
            coded += e_nnz
        idx = (np.arange(h)[:, None] * FAR_S1 + np.arange(w)[None, :]).ravel()
        for (start, length), b in zip(windows, before):
            exp = b.copy()
            for P in probes:
                at = P + idx - start
                ok = (at >= 0) & (at < length)
                exp[at[ok]] = recs[P].ravel()[ok]
            assert np.array_equal(far_rec.get_flat(start, length), exp), ("around", half, start)
    assert coded > 0


@pytest.mark.parametrize("luma", [True, False])
def test_fused_mc_distortion_at_far_offsets_vs_oracle(dev, far, luma):
    """pred_off, the block's offset in the original, in its plain form (unsigned) and in the halved form the sub-pel search builds (frac | XH_FRAC_HALF)"""
    import torch

    from xeve_amd import device as D

    r = np.random.default_rng(1100 + luma)
    O = oracle()
    pad, W, H = 72, 192, 128
    s = W + 2 * pad
    ref = r.integers(0, 1024, size=(H + 2 * pad, s), dtype=np.int16)
    d_ref = torch.from_numpy(ref).to(dev)
    unit = 16 if luma else 32
    for (w, h) in ([(8, 8), (16, 16), (32, 32), (64, 64)] if luma else [(4, 4), (8, 8), (16, 16), (32, 32)]):
        plain, marked, blocks = far_setup(far, r, w, h)
        where = [P for P in plain + marked for _ in range(4)]
        n = len(where)
        gx = [(pad + int(r.integers(-30, W + 30 - w))) * unit + (int(r.integers(1, unit // 4)) * 4 if i & 1 else 0) for i in range(n)]  # (the four filters at every probe)
        gy = [(pad + int(r.integers(-30, H + 30 - h))) * unit + (int(r.integers(1, unit // 4)) * 4 if i & 2 else 0) for i in range(n)]
        frac = [int((x & (unit - 1)) != 0) | (int((y & (unit - 1)) != 0) << 1) for x, y in zip(gx, gy)]
        assert frac == [i & 3 for i in range(n)]
        jobs = D.make_mc_jobs(gx, gy, [P // 2 if P in marked else P for P in where], [f | (HALFF if P in marked else 0) for f, P in zip(frac, where)], dev)
        ssd = D.mc_ssd_jobs(luma, d_ref, s, far.p1, FAR_S1, jobs, w, h, 10, torch.zeros(n, dtype=torch.int64, device=dev)).cpu().numpy()
        sad = D.mc_l_sad_jobs(d_ref, s, far.p1, FAR_S1, jobs, w, h, 10, torch.zeros(n, dtype=torch.int32, device=dev)).cpu().numpy() if luma else None
        for i, P in enumerate(where):
            e = np.zeros((h, w), np.int16)
            (O.xo_mc_l if luma else O.xo_mc_c)(frac[i] & 1, frac[i] >> 1, ptr(ref), gx[i], gy[i], s, w, ptr(e), w, h, 10, O.mc_l_coeff if luma else O.mc_c_coeff)
            assert ssd[i] == O.xo_ssd(w, h, ptr(blocks[P]), ptr(e), w, w, 10), (luma, w, P, i)
            if luma:
                assert sad[i] == O.xo_sad(w, h, ptr(blocks[P]), ptr(e), w, w, 10), (w, P, i)


# ---- the 16-bit wrap zone: full-scale residuals at QP 1, 3, 4, 9 (tests/_rdoq_cases.py saturated_residuals) -------------------------------------------------------------
WRAP_QPS = (1, 3, 4, 9)
WRAP_SIZES = [(4, 4), (5, 5), (6, 6), (4, 5), (6, 5)]  # 16 points: the control (nothing wraps); 32 and 64 points: dct_mfma.hip


def _plain_wrap_count(coef_fwd, levels_out, lw, lh, qp, intra):
    """positions whose plain level is above 32767 before the (s16) cast and whose output IS the wrapped value"""
    from _rdoq_cases import plain_levels

    lev = plain_levels(coef_fwd, lw, lh, qp, 10, intra)
    return int(((lev > 32767) & (np.abs(levels_out.astype(np.int64)) == np.abs(lev.astype(np.int16).astype(np.int64)))).sum())


@pytest.mark.parametrize("lw,lh", WRAP_SIZES)
def test_tq_chain_where_16_bit_levels_wrap(dev, lw, lh):
    """D.trans / D.quant / D.dquant / D.itrans on nine full-scale residual blocks per QP: the reference's plain quantiser stores its level through an (s16) cast
    (xeve_tq.c:723-724; the oracle is held to it on these blocks by tests/test_oracle_vs_ref.py), so on 32-point blocks at QP 1 and 3 and on 64-point blocks at every QP
    here the level wraps, and the wrapped level is what is dequantised and inverse-transformed.  Asserted: the wrap happened wherever a full-scale residual gets there."""
    import torch

    from _rdoq_cases import plain_wraps_expected, saturated_residuals
    from xeve_amd import device as D

    O = oracle()
    for qp in WRAP_QPS:
        resid = saturated_residuals(lw, lh, qp, 10)
        qs, dqs = D.QUANT_SCALE[0][qp % 6], D.DQ_SCALE[qp % 6] << (qp // 6)
        for intra in (0, 1):
            d = torch.from_numpy(resid.copy()).to(dev)
            D.trans(d, lw, lh, 10)
            fwd = d.cpu().numpy().copy()
            nnz = D.quant(d, lw, lh, qp, qs, intra, 10).cpu().numpy()
            q = d.cpu().numpy().copy()
            D.dquant(d, lw, lh, dqs, 10)
            dq = d.cpu().numpy().copy()
            D.itrans(d, lw, lh, 10)
            inv = d.cpu().numpy()
            for b in range(len(resid)):
                e = resid[b].copy()
                O.xo_trans(ptr(e), lw, lh, 10)
                assert np.array_equal(fwd[b], e), ("trans", qp, b)
                assert nnz[b] == O.xo_quant(ptr(e), lw, lh, qp, qs, intra, 10) and np.array_equal(q[b], e), ("quant", qp, intra, b)
                O.xo_dquant(ptr(e), lw, lh, dqs, 10)
                assert np.array_equal(dq[b], e), ("dquant", qp, intra, b)
                O.xo_itrans(ptr(e), lw, lh, 10)
                assert np.array_equal(inv[b], e), ("itrans", qp, intra, b)
            assert (_plain_wrap_count(fwd, q, lw, lh, qp, intra) > 0) == plain_wraps_expected(lw, lh, qp, 10), (lw, lh, qp, intra)


@pytest.mark.parametrize("rdoq", [0, 1], ids=["residual_rdo", "residual_rdoq"])
@pytest.mark.parametrize("lw,lh", WRAP_SIZES)
def test_fused_residual_chains_where_16_bit_levels_wrap(dev, lw, lh, rdoq):
    """xeve_hip_residual_rdo and xeve_hip_residual_rdoq (DIFF, SSD, DCT -- the matrix cores at 32 and 64 points --, zero pre-test, quantiser or RDOQ, dequant, IDCT,
    recon with its clip to 0 .. 1023, SSD) on original / prediction pairs whose difference is a full-scale residual block, QP 1, 3, 4, 9: every output = the oracle's
    step-by-step chain, and where a level can pass 32767 the coded levels show the wrapped value (RDOQ estimates capped for the reference's s32 rate)"""
    import ctypes as C

    import torch

    from _libs import oracle_rdoq
    from _rdoq_cases import cap_est, make_est, plain_wraps_expected, saturated_residuals, unwrapped_levels, wrapped_outputs, wraps_expected
    from xeve_amd import device as D
    from xeve_amd import lib

    O, OR = oracle(), oracle_rdoq()
    w, h, bd = 1 << lw, 1 << lh, 10
    n, s = w * h, 4 * 64 + 32
    for qp in WRAP_QPS:
        resid = saturated_residuals(lw, lh, qp, bd)
        nblk = len(resid)
        offs = [(8 + (b // 4) * h) * s + 8 + (b % 4) * w for b in range(nblk)]
        org = np.full((3 * 64 + 16, s), 512, np.int16)
        pred = np.where(resid < 0, -resid, 0).astype(np.int16)  # org - pred = the residual, both inside 0 .. 1023
        for b in range(nblk):
            y0, x0 = offs[b] // s, offs[b] % s
            org[y0:y0 + h, x0:x0 + w] = np.where(resid[b] > 0, resid[b], 0).reshape(h, w)
        fwd = resid.copy()
        for b in range(nblk):
            O.xo_trans(ptr(fwd, b * n), lw, lh, bd)
        est, lam = make_est(np.random.default_rng(4500 + (lw * 8 + lh) * 16 + qp)), 0.57 * 2.0 ** ((qp - 12) / 3.0)
        levels = unwrapped_levels(fwd, lw, lh, qp, bd)
        cap_est(est, levels)
        for intra in (0, 1):
            d_org, d_pred = torch.from_numpy(org).to(dev), torch.from_numpy(pred).to(dev)
            jobs = D.make_jobs(offs, np.arange(nblk) * n, dev)
            coef = torch.full((nblk, n), 77, dtype=torch.int16, device=dev)
            rec = torch.zeros_like(d_org)
            nnz = torch.zeros(nblk, dtype=torch.int32, device=dev)
            ssd = torch.zeros((nblk, 2), dtype=torch.int64, device=dev)
            if rdoq:
                D.residual_rdoq(d_org, s, d_pred, w, jobs, lw, lh, bd, qp, intra, lam, 1, lib.RdoqEst.from_buffer_copy(bytes(est)), coef, rec, s, nnz, ssd)
            else:
                D.residual_rdo(d_org, s, d_pred, w, jobs, lw, lh, bd, qp, intra, 1, coef, rec, s, nnz, ssd)
            coef, rec, nnz, ssd = coef.cpu().numpy(), rec.cpu().numpy(), nnz.cpu().numpy(), ssd.cpu().numpy()
            qs, dqs = D.QUANT_SCALE[0][qp % 6], D.DQ_SCALE[qp % 6] << (qp // 6)
            for b in range(nblk):
                c = np.zeros(n, np.int16)
                O.xo_diff(w, h, ptr(org, offs[b]), ptr(pred, b * n), s, w, w, ptr(c))
                assert np.array_equal(c, resid[b]) and ssd[b, 0] == O.xo_ssd(w, h, ptr(org, offs[b]), ptr(pred, b * n), s, w, bd)
                O.xo_trans(ptr(c), lw, lh, bd)
                if not O.xo_rdoq_zero_test(ptr(c), lw, lh, qp, qs, intra, bd):
                    c[:], e_nnz = 0, 0
                elif rdoq:
                    e_nnz = OR.xo_rdoq(ptr(c), lw, lh, qp, lam, 1, bd, 0, C.byref(est))
                else:
                    e_nnz = O.xo_quant(ptr(c), lw, lh, qp, qs, intra, bd)
                assert nnz[b] == e_nnz and np.array_equal(coef[b], c), ("levels", lw, lh, qp, intra, b)
                O.xo_dquant(ptr(c), lw, lh, dqs, bd)
                O.xo_itrans(ptr(c), lw, lh, bd)
                e = np.zeros((h, s), np.int16)
                O.xo_recon(ptr(c), ptr(pred, b * n), 1, w, h, s, ptr(e), bd)
                y0, x0 = offs[b] // s, offs[b] % s
                assert np.array_equal(rec[y0:y0 + h, x0:x0 + w], e[:, :w]), ("rec", lw, lh, qp, intra, b)
                assert ssd[b, 1] == O.xo_ssd(w, h, ptr(org, offs[b]), ptr(rec, offs[b]), s, s, bd)
            if rdoq:
                assert (wrapped_outputs(fwd, levels, coef) > 0) == wraps_expected(lw, lh, qp, bd), (lw, lh, qp, intra)
            else:
                assert (_plain_wrap_count(fwd, coef, lw, lh, qp, intra) > 0) == plain_wraps_expected(lw, lh, qp, bd), (lw, lh, qp, intra)
