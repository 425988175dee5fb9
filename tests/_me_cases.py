"""Seeded cases for the integer-pel diamond search, shared by the reference-pinning test, the golden generator and
the GPU test."""
import ctypes as C

import numpy as np

from _libs import MeJob, MeParams, MeResult, oracle_me, ptr

PAD = 144
REFI_BITS_2_0 = 1  # xeve_tbl_refi_bits[2][0] (xeve_tbl.c:498-517)


def make_planes(r, textured, W=256, H=192):
    s = W + 2 * PAD
    if textured:  # smooth moving texture: the search actually walks, the far rings get used
        yy, xx = np.mgrid[0:H + 2 * PAD, 0:s]
        base = (512 + 300 * np.sin(xx / 23.0) * np.cos(yy / 17.0) + 150 * np.sin((xx + yy) / 41.0))
        org = np.clip(base + r.integers(-6, 7, size=base.shape), 0, 1023).astype(np.int16)
        shift = (int(r.integers(-30, 31)), int(r.integers(-30, 31)))
        ref = np.roll(org, shift, axis=(0, 1))
        ref = np.clip(ref + r.integers(-6, 7, size=base.shape), 0, 1023).astype(np.int16)
    else:
        org = r.integers(0, 1024, size=(H + 2 * PAD, s), dtype=np.int16)
        ref = r.integers(0, 1024, size=(H + 2 * PAD, s), dtype=np.int16)
    return dict(org=org, ref=ref, s=s, W=W, H=H)


def make_job(r, pl, S, bi):
    W, H = pl["W"], pl["H"]
    x, y = int(r.integers(0, (W - S) // 8 + 1)) * 8, int(r.integers(0, (H - S) // 8 + 1)) * 8
    min_clip, max_clip = (-127, -127), (W - 1, H - 1)  # -MAX_CU_SIZE + 1 .. pic - 1 (xeve_pinter.c:2124-2127): every block read stays inside the 144-sample padding
    mvp = (int(r.integers(-160, 161)), int(r.integers(-160, 161)))  # quarter pel
    msr = int(r.choice([32, 64, 128]))
    sr = 5 if bi == 1 else int(r.choice([msr // 4, msr // 2, msr]))
    cx = min(max(x + (mvp[0] >> 2), min_clip[0]), max_clip[0])
    cy = min(max(y + (mvp[1] >> 2), min_clip[1]), max_clip[1])
    rng = [min(max(cx - sr, min_clip[0]), max_clip[0]), min(max(cy - sr, min_clip[1]), max_clip[1]),
           min(max(cx + sr, min_clip[0]), max_clip[0]), min(max(cy + sr, min_clip[1]), max_clip[1])]
    org_bi = (2 * r.integers(0, 1024, size=S * S) - r.integers(0, 1024, size=S * S)).astype(np.int16)
    return dict(org=pl["org"], ref=pl["ref"], s=pl["s"], x=x, y=y, S=S, bi=bi, min_clip=min_clip, max_clip=max_clip, range=rng,
                gmvp=(mvp[0] + (x << 2), mvp[1] + (y << 2)), mvi=(mvp[0] + (x << 2), mvp[1] + (y << 2)), msr=msr, sr=sr,
                lambda_mv=int(r.integers(1 << 16, 1 << 23)), faststep=int(r.choice([2, 3])), mot_other=int(r.integers(2, 30)),
                org_bi=org_bi, beststep_in=int(r.integers(0, 3)))


def make_case(r, S, bi, textured):
    return make_job(r, make_planes(r, textured), S, bi)


def params_of(c):
    return MeParams(c["lambda_mv"], REFI_BITS_2_0, c["mot_other"], c["bi"], c["faststep"], c["msr"], c["sr"],
                    (C.c_int32 * 2)(*c["min_clip"]), (C.c_int32 * 2)(*c["max_clip"]), 0)


def job_of(c, org_off=0):
    return MeJob(c["x"], c["y"], org_off, (C.c_int16 * 4)(*c["range"]), (C.c_int16 * 2)(*c["gmvp"]), (C.c_int16 * 2)(*c["mvi"]), c["beststep_in"])


def run_oracle(c, bit_depth=10):
    O = oracle_me()
    lg = c["S"].bit_length() - 1
    p, j, res = params_of(c), job_of(c), MeResult()
    O.xo_me_ipel_diamond(ptr(c["org"], PAD * c["s"] + PAD), c["s"], ptr(c["org_bi"]), ptr(c["ref"], PAD * c["s"] + PAD), c["s"], C.byref(j), lg, lg,
                         bit_depth, C.byref(p), C.byref(res))
    return res


# ---- sub-pel pattern search (me_spel_pattern) ----------------------------------------------------------------------
def make_spel_job(r, pl, S, bi):
    from _libs import oracle

    W, H = pl["W"], pl["H"]
    x, y = int(r.integers(0, (W - S) // 8 + 1)) * 8, int(r.integers(0, (H - S) // 8 + 1)) * 8
    mvp = (int(r.integers(-160, 161)), int(r.integers(-160, 161)))
    mvi = (int(r.integers(-30, 31)) * 4, int(r.integers(-30, 31)) * 4)  # an integer-pel MV, quarter-pel units
    org_bi = (2 * r.integers(0, 1024, size=S * S) - r.integers(0, 1024, size=S * S)).astype(np.int16)
    return dict(org=pl["org"], ref=pl["ref"], s=pl["s"], x=x, y=y, S=S, bi=bi, gmvp=(mvp[0] + (x << 2), mvp[1] + (y << 2)), mvi=mvi,
                lambda_mv=int(r.integers(1 << 16, 1 << 23)), mot_other=int(r.integers(2, 30)), org_bi=org_bi,
                hpel_cnt=int(r.choice([2, 4, 8])), qpel_cnt=int(r.choice([0, 4, 8])))


def run_oracle_spel(c, bit_depth=10):
    from _libs import SpelJob, SpelParams, oracle_spel

    O = oracle_spel()
    lg = c["S"].bit_length() - 1
    p = SpelParams(c["lambda_mv"], REFI_BITS_2_0, c["mot_other"], c["bi"], c["hpel_cnt"], c["qpel_cnt"])
    j = SpelJob(c["x"], c["y"], 0, (C.c_int16 * 2)(*c["gmvp"]), (C.c_int16 * 2)(*c["mvi"]))
    res = MeResult()
    O.xo_me_spel_pattern(ptr(c["org"], PAD * c["s"] + PAD), c["s"], ptr(c["org_bi"]), ptr(c["ref"], PAD * c["s"] + PAD), c["s"], C.byref(j), lg, lg, bit_depth,
                         O.mc_l_coeff, C.byref(p), C.byref(res))
    return res


# ---- EPZS driver (pinter_me_epzs) ------------------------------------------------------------------------------------
def make_epzs_job(r, pl, S, bi):
    W, H = pl["W"], pl["H"]
    x, y = int(r.integers(0, (W - S) // 8 + 1)) * 8, int(r.integers(0, (H - S) // 8 + 1)) * 8
    msr = int(r.choice([32, 64]))
    return dict(org=pl["org"], ref=pl["ref"], s=pl["s"], x=x, y=y, S=S, bi=bi, min_clip=(-127, -127), max_clip=(W - 1, H - 1),
                mvp=(int(r.integers(-100, 101)), int(r.integers(-100, 101))), mv0=(int(r.integers(-25, 26)) * 4, int(r.integers(-25, 26)) * 4),
                msr=msr, sr=int(r.choice([msr // 4, msr // 2, msr])), lambda_mv=int(r.integers(1 << 16, 1 << 22)), mot_other=int(r.integers(2, 30)),
                org_bi=(2 * r.integers(0, 1024, size=S * S) - r.integers(0, 1024, size=S * S)).astype(np.int16),
                hpel_cnt=int(r.choice([2, 4, 8])), qpel_cnt=int(r.choice([0, 4, 8])))


def epzs_params_of(c):
    from _libs import EpzsParams, SpelParams

    # reserved: bit 0 = raster search on (me_complexity > 1), bits 8.. = refi (the raster step scales with it); refi_bits [2][0] == [2][1]
    me = MeParams(c["lambda_mv"], REFI_BITS_2_0, c["mot_other"], c["bi"], 3, c["msr"], c["sr"], (C.c_int32 * 2)(*c["min_clip"]),
                  (C.c_int32 * 2)(*c["max_clip"]), int(c.get("raster", 0)) | (int(c.get("refi", 0)) << 8))
    return EpzsParams(me, SpelParams(0, 0, 0, 0, c["hpel_cnt"], c["qpel_cnt"]))


def run_oracle_epzs(c, with_mot=False, bit_depth=10):
    """(cost, mv) of pinter_me_epzs; with_mot: also what it leaves in pi->mot_bits[lidx] (-1 = untouched)"""
    from _libs import oracle_epzs

    O = oracle_epzs()
    lg = c["S"].bit_length() - 1
    mvp, mv = np.array(c["mvp"], np.int16), np.array(c["mv0"], np.int16)
    p = epzs_params_of(c)
    mot = C.c_int(-1)
    O.xo_me_epzs_mot.restype = C.c_uint32
    O.xo_me_epzs_mot.argtypes = O.xo_me_epzs.argtypes + [C.POINTER(C.c_int)]
    cost = O.xo_me_epzs_mot(ptr(c["org"], PAD * c["s"] + PAD), c["s"], ptr(c["org_bi"]), ptr(c["ref"], PAD * c["s"] + PAD), c["s"], c["x"], c["y"], ptr(mvp),
                            ptr(mv), lg, lg, bit_depth, O.mc_l_coeff, C.byref(p), C.byref(mot))
    return (cost, int(mv[0]), int(mv[1]), mot.value) if with_mot else (cost, int(mv[0]), int(mv[1]))


# ---- degenerate content: candidates that tie, search windows that clip -------------------------------------------------------------------------------------------
# Small pictures (W = H = max(64, S)), same plane layout and clip limits as above.  Four families, each built for one property of the reference's search that
# the noise / texture generators above do not reach (the counters below measure it on the CPU, the tests assert the counts):
#   flat        reference plane constant, original noise: every SAD is the same, only the vector bits decide -- ties inside the dense round
#   periodicN   reference plane a random tile repeated (periodic4: 2 rows x 4 columns, ties inside the dense 5x5 / 11x11 round; periodic8 / 16 / 32: square, ties
#               in the rings), the original the reference displaced by half a period: the ring of L1 radius N/2 holds two exact matches at equal vector bits
#   outward     noise, the predictor 50 to 130 pel outside the picture: the clipped centre sits on a clip limit, the window is narrower than 2 * sr
#   static      reference == original, the whole plane flat or of period 8: a zero-SAD plateau (sub-pel stage, refinement loop of pinter_me_epzs)
TILES = {"periodic4": (2, 4), "periodic8": (8, 8), "periodic16": (16, 16), "periodic32": (32, 32)}
ME_FAMILIES = ("flat", "periodic4", "periodic8", "periodic16", "periodic32", "outward")


def make_degenerate_planes(r, family, S, bd=10, vertical=False, static_kind="flat"):
    W = H = max(64, S)
    s = W + 2 * PAD
    shape, top = (H + 2 * PAD, s), 1 << bd
    noise = lambda: r.integers(0, top, size=shape, dtype=np.int16)
    tiled = lambda t: np.tile(t, (shape[0] // t.shape[0] + 1, shape[1] // t.shape[1] + 1))[:shape[0], :shape[1]].copy()
    disp = (0, 0)
    if family == "flat":
        org, ref = noise(), np.full(shape, int(r.integers(0, top)), np.int16)
    elif family in TILES:
        th, tw = TILES[family]
        assert shape[0] % th == 0 and shape[1] % tw == 0  # the roll below wraps in phase
        ref = tiled(r.integers(0, top, size=(th, tw), dtype=np.int16))
        disp = (0, th // 2) if vertical else (tw // 2, 0)
        org = np.roll(ref, (-disp[1], -disp[0]), axis=(0, 1))  # org(u, v) = ref(u + dx, v + dy)
    elif family == "outward":  # (noise of 1/64 of the sample range about mid-grey: the vector bits weigh against it, and they pull towards the predictor -- outwards)
        org, ref = ((top >> 1) + (noise() >> 6) for _ in range(2))
    elif family == "static":
        ref = np.full(shape, int(r.integers(0, top)), np.int16) if static_kind == "flat" else tiled(r.integers(0, top, size=(8, 8), dtype=np.int16))
        org = ref.copy()
    else:
        raise ValueError(family)
    return dict(org=org, ref=ref, s=s, W=W, H=H, disp=disp, family=family)


def _clip(v, lo, hi):
    return min(max(v, lo), hi)


def _job_from(pl, S, bi, x, y, mvp, base, org_bi, beststep_in):
    """one job with the launch's shared parameters; the range derived exactly as make_job derives it"""
    mn, mx = base["min_clip"], base["max_clip"]
    sr = base["sr"]
    cx, cy = _clip(x + (mvp[0] >> 2), mn[0], mx[0]), _clip(y + (mvp[1] >> 2), mn[1], mx[1])
    rng = [_clip(cx - sr, mn[0], mx[0]), _clip(cy - sr, mn[1], mx[1]), _clip(cx + sr, mn[0], mx[0]), _clip(cy + sr, mn[1], mx[1])]
    g = (mvp[0] + (x << 2), mvp[1] + (y << 2))
    return dict(org=pl["org"], ref=pl["ref"], s=pl["s"], x=x, y=y, S=S, bi=bi, min_clip=mn, max_clip=mx, range=rng, gmvp=g, mvi=g, msr=base["msr"], sr=sr,
                lambda_mv=base["lambda_mv"], faststep=base["faststep"], mot_other=base["mot_other"], org_bi=org_bi, beststep_in=beststep_in)


def make_degenerate_jobs(r, family, S, bi, n, bd=10, vertical=False, static_kind="flat", pl=None):
    """n jobs of one launch (planes and launch-level parameters shared) -> (planes, cases); pl: planes of an earlier call of the same family and bit depth"""
    pl = make_degenerate_planes(r, family, S, bd, vertical, static_kind) if pl is None else pl
    W, H, top = pl["W"], pl["H"], 1 << bd
    base = make_job(r, pl, S, bi)
    if family in TILES:
        base.update(lambda_mv=1 << 16, faststep=3, msr=64, sr=5 if bi == 1 else 64)
    if family == "outward":
        base["lambda_mv"] = int(r.integers(1 << 20, 1 << 23))
    mn, mx = base["min_clip"], base["max_clip"]
    cases = []
    for k in range(n):
        x, y = int(r.integers(0, (W - S) // 8 + 1)) * 8, int(r.integers(0, (H - S) // 8 + 1)) * 8
        org_bi = (2 * r.integers(0, top, size=S * S) - r.integers(0, top, size=S * S)).astype(np.int16)
        if family in TILES:
            th, tw = TILES[family]
            # integer-pel predictor = start vector, a whole number of periods away: the original is the reference block at the centre displaced by half a period
            # (seven jobs of eight keep half a period from the clip limits, so that both matches of the ring lie inside the window)
            gx, gy = (0, 0) if k % 8 == 0 else (tw // 2, th // 2)
            kx = int(r.integers(-((x - mn[0] - gx) // tw), (mx[0] - gx - x) // tw + 1))
            ky = int(r.integers(-((y - mn[1] - gy) // th), (mx[1] - gy - y) // th + 1))
            mvp = (4 * kx * tw, 4 * ky * th)
            if family == "periodic4" and k % 2:  # (the dense round ties without that too: every other job with a quarter-pel predictor anywhere)
                mvp = (int(r.integers(-160, 161)), int(r.integers(-160, 161)))
            org_bi = np.ascontiguousarray(pl["org"][PAD + y:PAD + y + S, PAD + x:PAD + x + S]).reshape(-1).copy()
        elif family == "outward":
            # quarter-pel target per axis: 50 to 130 pel before the picture's first or beyond its last sample; every other target beyond the last sample sits exactly
            # 254 or 510 quarter pel past it -- the clip limit is then the last position before a step of the vector-bit table, one column cheaper than all others
            t = [(-4 * d - f if neg else 4 * (lim + d) + f) for d, f, neg, lim in zip(r.integers(50, 131, size=2).tolist(), r.integers(0, 4, size=2).tolist(),
                                                                                      r.integers(0, 2, size=2).tolist(), (W - 1, H - 1))]
            for a, lim in enumerate((W - 1, H - 1)):
                if t[a] > 0 and r.integers(0, 2):
                    t[a] = 4 * lim + int(r.choice([254, 510]))
            mvp = (t[0] - 4 * x, t[1] - 4 * y)
            org_bi = ((top >> 1) + 2 * (r.integers(0, top, size=S * S) >> 6) - (r.integers(0, top, size=S * S) >> 6)).astype(np.int16)  # (2 * original - the other prediction)
        else:
            mvp = (int(r.integers(-160, 161)), int(r.integers(-160, 161)))
            if family == "static":
                org_bi = np.ascontiguousarray(pl["org"][PAD + y:PAD + y + S, PAD + x:PAD + x + S]).reshape(-1).copy()
        cases.append(_job_from(pl, S, bi, x, y, mvp, base, org_bi, int(r.integers(0, 3))))
    return pl, cases


def spel_case_of(c, hpel_cnt=8, qpel_cnt=8):
    """the sub-pel pattern around the job's clipped integer centre, the predictor equal to it: (-2, 0) and (2, 0) cost the same bits, and so do the four quarter-pel axis points"""
    cx, cy = _clip(c["mvi"][0] >> 2, c["min_clip"][0], c["max_clip"][0]), _clip(c["mvi"][1] >> 2, c["min_clip"][1], c["max_clip"][1])
    return dict(org=c["org"], ref=c["ref"], s=c["s"], x=c["x"], y=c["y"], S=c["S"], bi=min(c["bi"], 1), gmvp=(cx << 2, cy << 2), mvi=((cx - c["x"]) << 2, (cy - c["y"]) << 2),
                lambda_mv=c["lambda_mv"], mot_other=c["mot_other"], org_bi=c["org_bi"], hpel_cnt=hpel_cnt, qpel_cnt=qpel_cnt)


def epzs_case_of(c, hpel_cnt=8, qpel_cnt=8, raster=0, refi=0):
    mvp = (c["gmvp"][0] - (c["x"] << 2), c["gmvp"][1] - (c["y"] << 2))
    return dict(org=c["org"], ref=c["ref"], s=c["s"], x=c["x"], y=c["y"], S=c["S"], bi=min(c["bi"], 1), min_clip=c["min_clip"], max_clip=c["max_clip"], mvp=mvp,
                mv0=((mvp[0] >> 2) << 2, (mvp[1] >> 2) << 2), msr=c["msr"], sr=c["sr"], lambda_mv=c["lambda_mv"], mot_other=c["mot_other"], org_bi=c["org_bi"],
                hpel_cnt=hpel_cnt, qpel_cnt=qpel_cnt, raster=raster, refi=refi)


# ---- the counters: the property each family was built for, from numpy SADs and xo_mv_bits (no search code) --------------------------------------------------------
def cand_cost(c, mx, my, bd=10):
    """MV_COST + SAD of one integer position, as me_ipel_diamond prices it"""
    S = c["S"]
    ref = c["ref"][PAD + my:PAD + my + S, PAD + mx:PAD + mx + S].astype(np.int64)
    org = c["org_bi"].reshape(S, S) if c["bi"] else c["org"][PAD + c["y"]:PAD + c["y"] + S, PAD + c["x"]:PAD + c["x"] + S]
    sad = int(np.abs(org.astype(np.int64) - ref).sum()) >> (bd - 8)
    bits = oracle_me().xo_mv_bits((mx << 2) - c["gmvp"][0], (my << 2) - c["gmvp"][1]) + REFI_BITS_2_0 + (c["mot_other"] if c["bi"] else 0)
    return (((c["lambda_mv"] * bits + (1 << 15)) & 0xFFFFFFFF) >> 16) + (sad >> 1 if c["bi"] else sad)


def centre_of(c):
    return _clip(c["mvi"][0] >> 2, c["min_clip"][0], c["max_clip"][0]), _clip(c["mvi"][1] >> 2, c["min_clip"][1], c["max_clip"][1])


def dense_grid(c):
    """corners of the first round's grid: 5x5 (bi == 1: 11x11) around the clipped centre, not extended on a side where the centre sits on the range (xeve_pinter.c:397-462)"""
    bx, by = centre_of(c)
    d, rg = (5 if c["bi"] == 1 else 2), c["range"]
    x0, y0 = (bx if bx <= rg[0] else bx - d), (by if by <= rg[1] else by - d)
    x1, y1 = (bx if bx >= rg[2] else bx + d), (by if by >= rg[3] else by + d)
    return x0, y0, x1, y1


def dense_round(c, bd=10):
    """[(mx, my, cost)] of the first round in evaluation order, cut to the range"""
    x0, y0, x1, y1 = dense_grid(c)
    S, rg = c["S"], c["range"]
    org = c["org_bi"].reshape(S, S) if c["bi"] else c["org"][PAD + c["y"]:PAD + c["y"] + S, PAD + c["x"]:PAD + c["x"] + S]
    win = np.lib.stride_tricks.sliding_window_view(c["ref"][PAD + y0:PAD + y1 + S, PAD + x0:PAD + x1 + S], (S, S)).astype(np.int32)
    sad = np.abs(win - org.astype(np.int32)).sum(axis=(2, 3)) >> (bd - 8)
    mvb, extra = oracle_me().xo_mv_bits, REFI_BITS_2_0 + (c["mot_other"] if c["bi"] else 0)
    out = []
    for my in range(y0, y1 + 1):
        for mx in range(x0, x1 + 1):
            if rg[0] <= mx <= rg[2] and rg[1] <= my <= rg[3]:
                bits = mvb((mx << 2) - c["gmvp"][0], (my << 2) - c["gmvp"][1]) + extra
                t = int(sad[my - y0, mx - x0])
                out.append((mx, my, (((c["lambda_mv"] * bits + (1 << 15)) & 0xFFFFFFFF) >> 16) + (t >> 1 if c["bi"] else t)))
    return out


def dense_points(c):
    x0, y0, x1, y1 = dense_grid(c)
    rg = c["range"]
    return max(0, min(x1, rg[2]) - max(x0, rg[0]) + 1) * max(0, min(y1, rg[3]) - max(y0, rg[1]) + 1)


def dense_tie(c, bd=10):
    costs = [t[2] for t in dense_round(c, bd)]
    return costs.count(min(costs)) >= 2


def winner_of(c, res):
    return c["x"] + (res.mv[0] >> 2), c["y"] + (res.mv[1] >> 2)


def ring_mirror_tie(c, res, bd=10):
    """the oracle's winner was found in a ring (beststep >= 4) and its point mirror about the rings' centre lies inside the re-centred range at the same cost"""
    if res.beststep < 4:
        return False
    dense = dense_round(c, bd)
    bx, by, _ = min(dense, key=lambda t: t[2])  # (min keeps the first of equals)
    sr, mn, mx = (5 if c["bi"] == 1 else c["sr"]), c["min_clip"], c["max_clip"]
    rg = [_clip(bx - sr, mn[0], mx[0]), _clip(by - sr, mn[1], mx[1]), _clip(bx + sr, mn[0], mx[0]), _clip(by + sr, mn[1], mx[1])]
    (ix, iy), (wx, wy) = centre_of(c), winner_of(c, res)
    qx, qy = 2 * ix - wx, 2 * iy - wy
    return (qx, qy) != (wx, wy) and rg[0] <= qx <= rg[2] and rg[1] <= qy <= rg[3] and cand_cost(c, qx, qy, bd) == res.cost


def on_clip_limit(c, res):
    wx, wy = winner_of(c, res)
    return wx in (c["min_clip"][0], c["max_clip"][0]) or wy in (c["min_clip"][1], c["max_clip"][1])


# ---- one launch per (family, S, bi, bit depth), its oracle results and its counts: computed once, shared by the CPU and the GPU tests -------------------------------
import functools  # noqa: E402

RING_STEP = {"periodic8": 4, "periodic16": 8, "periodic32": 16}
N_LAUNCH = 100


@functools.lru_cache(maxsize=None)
def degenerate_launch(family, S, bi, bd=10, static_kind="flat"):
    r = np.random.default_rng(5000 + 97 * (ME_FAMILIES + ("static",)).index(family) + S + 7 * bi + 1000 * bd + (static_kind != "flat"))
    pl, cases = make_degenerate_jobs(r, family, S, bi, N_LAUNCH, bd, vertical=(S.bit_length() + bi) % 2 == 1, static_kind=static_kind)
    res = [run_oracle(c, bd) for c in cases]
    return pl, cases, res


def family_counts(family, S, bi, bd=10):
    _, cases, res = degenerate_launch(family, S, bi, bd)
    n = dict(jobs=len(cases))
    if family in ("flat", "periodic4"):
        n["dense_tie"] = sum(dense_tie(c, bd) for c in cases)
    if family in RING_STEP:
        n["at_step"] = sum(e.beststep == RING_STEP[family] for e in res)
        n["mirror_tie"] = sum(ring_mirror_tie(c, e, bd) for c, e in zip(cases, res))
    if family == "outward":
        n["on_clip"] = sum(on_clip_limit(c, e) for c, e in zip(cases, res))
        n["cut_grid"] = sum(dense_points(c) < (121 if bi == 1 else 25) for c in cases)
    return n


def assert_family_condition(family, S, bi, bd=10):
    """what the family was built for does occur, at least at the share its test relies on (measured on the oracle alone: flat 34 to 61 of 100, periodic4 67 to 82,
    the ring families 100 at their step with 91 to 100 mirror ties, outward 49 to 64 winners on a clip limit and 70 to 90 cut grids)"""
    n = family_counts(family, S, bi, bd)
    print(family, S, bi, bd, n)
    if "dense_tie" in n:
        assert 4 * n["dense_tie"] >= n["jobs"], n
    if "at_step" in n:
        assert n["at_step"] == n["jobs"] and 5 * n["mirror_tie"] >= 4 * n["jobs"], n
    if "on_clip" in n:
        assert 4 * n["on_clip"] >= n["jobs"] and 2 * n["cut_grid"] >= n["jobs"], n
    return n


# ---- the rows of tests/golden/me_degenerate_v1.npz (make_me_degenerate_golden.py records the reference's results for them) ---------------------------------------------
# (key, family, bit depth, static kind): one plane pair each; per pair 2 jobs for every S and bi
GOLDEN_SETS = [("flat", "flat", 10, "flat"), ("periodic4", "periodic4", 10, "flat"), ("periodic8", "periodic8", 10, "flat"), ("periodic16", "periodic16", 10, "flat"),
               ("periodic32", "periodic32", 10, "flat"), ("outward", "outward", 10, "flat"), ("static_flat", "static", 10, "flat"), ("static_periodic", "static", 10, "periodic"),
               ("periodic8_bd8", "periodic8", 8, "flat"), ("periodic8_bd12", "periodic8", 12, "flat"), ("outward_bd8", "outward", 8, "flat"), ("outward_bd12", "outward", 12, "flat")]
EPZS_VARIANTS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 0, 1), (1, 1, 1)]  # (raster, refi, integer refinement instead of the sub-pel pattern)


def degenerate_golden_jobs(key):
    """(planes, bit depth, cases) of one set: seeded, so that the golden generator and the reference-pinning test walk the same rows"""
    k = [g[0] for g in GOLDEN_SETS].index(key)
    _, family, bd, kind = GOLDEN_SETS[k]
    r = np.random.default_rng(7100 + k)
    pl, cases = None, []
    for S in (8, 16, 32, 64):
        for bi in (0, 1, 2):
            pl, cs = make_degenerate_jobs(r, family, S, bi, 2, bd, vertical=(S.bit_length() + bi) % 2 == 1, static_kind=kind, pl=pl)
            cases += cs
    return pl, bd, cases


def epzs_variant_of(c, v):
    raster, refi, ipel = v
    return epzs_case_of(c, 0 if ipel else 8, 0 if ipel else 8, raster, refi)


# ---- the noise / texture batches of test_hip_me.py::test_me_batches_vs_oracle ------------------------------------------------------------------------------------------
def batch_cases(seed, S, bi, textured):
    r = np.random.default_rng(seed)
    pl = make_planes(r, textured)
    base = make_job(r, pl, S, bi)
    cases = []
    for _ in range(150):
        c = make_job(r, pl, S, bi)
        for k in ("lambda_mv", "mot_other", "faststep", "msr", "sr"):  # launch-level parameters are shared
            c[k] = base[k]
        # the job's own range must be derived with the shared search range
        sr = base["sr"]
        cx = min(max(c["x"] + ((c["gmvp"][0] - (c["x"] << 2)) >> 2), c["min_clip"][0]), c["max_clip"][0])
        cy = min(max(c["y"] + ((c["gmvp"][1] - (c["y"] << 2)) >> 2), c["min_clip"][1]), c["max_clip"][1])
        c["range"] = [min(max(cx - sr, c["min_clip"][0]), c["max_clip"][0]), min(max(cy - sr, c["min_clip"][1]), c["max_clip"][1]),
                      min(max(cx + sr, c["min_clip"][0]), c["max_clip"][0]), min(max(cy + sr, c["min_clip"][1]), c["max_clip"][1])]
        cases.append(c)
    return cases


def batch_launches(S, bi, textured):
    """one launch of 150 jobs per setting; a second one where the first never leaves the dense round (S 8, bi 2, texture: lambda_mv 8.3e6 on noise originals -- the
    vector bits decide everything)"""
    seeds = [1000 + S + bi * 7 + textured] + ([31023] if (S, bi, textured) == (8, 2, True) else [])
    return [batch_cases(seed, S, bi, textured) for seed in seeds]


# distinct beststep values the oracle ends at, per (S, bi, textured); bi == 1 has the dense round only (tests/test_me_degenerate.py counts them on the CPU)
BATCH_STEPS = {(8, 0, False): 3, (16, 0, False): 4, (32, 0, False): 6, (64, 0, False): 4, (8, 1, False): 1, (16, 1, False): 1, (32, 1, False): 1, (64, 1, False): 1,
               (8, 2, False): 3, (16, 2, False): 3, (32, 2, False): 5, (64, 2, False): 5, (8, 0, True): 5, (16, 0, True): 5, (32, 0, True): 6, (64, 0, True): 5,
               (8, 1, True): 1, (16, 1, True): 1, (32, 1, True): 1, (64, 1, True): 1, (8, 2, True): 5, (16, 2, True): 3, (32, 2, True): 4, (64, 2, True): 7}


# ---- the right edge of the widest accepted picture: quarter-pel FRAME coordinates beyond an s16 ----------------------------------------------------------------------
# pinter_me_epzs keeps gmvp = mvp + (x << 2) and mvi = start + (x << 2) in s16 (xeve_pinter.c:711-735, 790-791, 841-842).  x << 2 reaches 32 736 at x = 8184, so in
# the last CTU column of a picture wider than 8128 a predictor or start vector that points right wraps: the wrapped gmvp prices every candidate against a point 16 384
# samples to the left, and a wrapped mvi starts the diamond at min_clip -- its first round has no candidate inside the range, the range is re-centred there, and the
# whole search happens at the picture's LEFT end.  Deterministic C on the reference's side, mirrored by casts in the oracle, me.hip and walk_inter.h; this family
# executes them with values that wrap.
#   planes    8192 x 64 plus padding; the reference plane an integer texture (closed form, no generator state: the fixture stores a CRC, not the samples), the original
#             of size S the reference moved RE_SHIFT[S] samples plus a little noise, so the true motion points right
#   jobs      y = 0, x = 8192 - S for S = 64 / 32 / 16 / 8, five predictors per size: (x << 2) + mvp_x = 32 764, 32 767 (controls), 32 768, 32 800, 33 500
#   modes     bi 0, 1 (BI_NORMAL: starts from mv), 2 (starts from mvp)
#   ranges    xeve_pinter.c:2124-2126 for w = 8192, h = 64; RE_PRESETS: search ranges and sub-pel counts of presets fast, medium, slow (quarter pel) and placebo (raster)
# The twin of a job is the same search RE_TWIN samples further left on the same content (the planes rolled by RE_TWIN columns, x and max_clip RE_TWIN less): every sample, every
# clip distance and every vector is the same, only x << 2 is 4 * RE_TWIN less and nothing wraps -- what the wrapped job would give in int arithmetic.
RE_W, RE_H = 8192, 64
RE_SIZES = (64, 32, 16, 8)
RE_SHIFT = {64: 40, 32: 25, 16: 12, 8: 5}
RE_TARGETS = (32764, 32767, 32768, 32800, 33500)
RE_WRAPPED_PER_LAUNCH = 3  # of 5 jobs: the targets beyond 32 767
RE_PRESETS = {"fast": dict(msr=32, sr=16, hpel_cnt=2, qpel_cnt=0, raster=0), "medium": dict(msr=64, sr=32, hpel_cnt=4, qpel_cnt=0, raster=0),
              "slow": dict(msr=128, sr=64, hpel_cnt=4, qpel_cnt=4, raster=0), "placebo": dict(msr=384, sr=96, hpel_cnt=8, qpel_cnt=8, raster=1)}
RE_LAUNCHES = [(S, bi, preset) for S in RE_SIZES for bi in (0, 1, 2) for preset in RE_PRESETS]
RE_TWIN = 256  # (64 would do for the targets up to 32 800; 33 500 - 4 * 64 still wraps)


def s16(v):
    return ((int(v) + 32768) & 0xFFFF) - 32768


def _tri(v, p):
    return np.abs(v % (2 * p) - p)


@functools.lru_cache(maxsize=None)
def right_edge_ref_plane():
    yy, xx = np.mgrid[0:RE_H + 2 * PAD, 0:RE_W + 2 * PAD].astype(np.int64)
    v = 100 + 5 * _tri(xx + yy, 53) + 4 * _tri(2 * xx - yy, 37) + 3 * _tri(xx + 3 * yy, 11) + ((((xx * 73856093) ^ (yy * 19349663)) >> 5) & 7)
    return np.ascontiguousarray(v.astype(np.int16))


@functools.lru_cache(maxsize=None)
def right_edge_planes(S, twin=False):
    """the plane pair of size S; twin: both planes rolled RE_TWIN columns to the left, so that the block at x - RE_TWIN sees what the block at x saw"""
    ref = right_edge_ref_plane()
    yy, xx = np.mgrid[0:ref.shape[0], 0:ref.shape[1]].astype(np.int64)
    org = np.roll(ref, -RE_SHIFT[S], axis=1) + ((((xx * 83492791) ^ (yy * 2971215073)) >> 7) % 5 - 2).astype(np.int16)  # org(u) = ref(u + shift) + noise
    if twin:
        org, ref = np.roll(org, -RE_TWIN, axis=1), np.roll(ref, -RE_TWIN, axis=1)
    return dict(org=np.ascontiguousarray(org), ref=np.ascontiguousarray(ref), s=ref.shape[1], W=RE_W, H=RE_H)


def right_edge_jobs(S, bi, preset, twin=False):
    """the five jobs of one launch as diamond cases (gmvp and mvi as pinter_me_epzs hands them down: wrapped), with the raw mvp / mv0 and the sub-pel counts beside them"""
    pl, pr = right_edge_planes(S, twin), RE_PRESETS[preset]
    off = RE_TWIN if twin else 0
    x, y = RE_W - S - off, 0
    mn, mx = (-127, -127), (RE_W - 1 - off, RE_H - 1)
    k = RE_SIZES.index(S) * 12 + bi * 4 + list(RE_PRESETS).index(preset)
    lambda_mv, mot_other, sr = (1 << 17) + 9001 * k, 3 + k % 17, (5 if bi == 1 else pr["sr"])
    blk = pl["org"][PAD:PAD + S, PAD + x:PAD + x + S].astype(np.int32).reshape(-1)
    cases = []
    for t, target in enumerate(RE_TARGETS):
        mvp = (target - ((RE_W - S) << 2), 4 * (t - 2) + 1)
        mv0 = ((mvp[0] >> 2) << 2, (mvp[1] >> 2) << 2)
        start = mv0 if bi == 1 else mvp
        cx, cy = _clip(x + (start[0] >> 2), mn[0], mx[0]), _clip(y + (start[1] >> 2), mn[1], mx[1])
        rng = [_clip(cx - sr, mn[0], mx[0]), _clip(cy - sr, mn[1], mx[1]), _clip(cx + sr, mn[0], mx[0]), _clip(cy + sr, mn[1], mx[1])]
        org_bi = (blk + (np.arange(S * S) * 7 + 3 * t + k) % 5 - 2).astype(np.int16)  # 2 * original - the other list's prediction, where that prediction is good
        cases.append(dict(org=pl["org"], ref=pl["ref"], s=pl["s"], x=x, y=y, S=S, bi=bi, min_clip=mn, max_clip=mx, range=rng,
                          gmvp=(s16(mvp[0] + (x << 2)), s16(mvp[1] + (y << 2))), mvi=(s16(start[0] + (x << 2)), s16(start[1] + (y << 2))), msr=pr["msr"], sr=sr,
                          lambda_mv=lambda_mv, faststep=3, mot_other=mot_other, org_bi=org_bi, beststep_in=0, mvp=mvp, mv0=mv0, hpel_cnt=pr["hpel_cnt"],
                          qpel_cnt=pr["qpel_cnt"], raster=pr["raster"], frame_x=mvp[0] + (x << 2)))
    return cases


def right_edge_wrapped(c):
    """(a) of the family: the job's quarter-pel frame coordinate does not fit an s16"""
    return c["frame_x"] > 32767


def right_edge_spel_case(c, mvi=None):
    """the sub-pel pattern with the job's (wrapped) predictor around the integer vector of the true motion, or around mvi: the vector the job's diamond search ended
    on -- from a wrapped start that is a position at the picture's left end whose s16 vector has wrapped too, and cx = mvi + (x << 2) wraps back (xeve_pinter.c:584)"""
    return dict(org=c["org"], ref=c["ref"], s=c["s"], x=c["x"], y=c["y"], S=c["S"], bi=min(c["bi"], 1), gmvp=c["gmvp"], mvi=mvi or (4 * RE_SHIFT[c["S"]], 0), lambda_mv=c["lambda_mv"],
                mot_other=c["mot_other"], org_bi=c["org_bi"], hpel_cnt=c["hpel_cnt"], qpel_cnt=c["qpel_cnt"])


def right_edge_epzs_case(c, ipel=False):
    """the whole pinter_me_epzs of the job: raw mvp and start vector, the casts are the search's own; ipel: the integer refinement in place of the sub-pel pattern"""
    return dict(org=c["org"], ref=c["ref"], s=c["s"], x=c["x"], y=c["y"], S=c["S"], bi=min(c["bi"], 1), min_clip=c["min_clip"], max_clip=c["max_clip"], mvp=c["mvp"], mv0=c["mv0"],
                msr=c["msr"], sr=c["sr"], lambda_mv=c["lambda_mv"], mot_other=c["mot_other"], org_bi=c["org_bi"], hpel_cnt=0 if ipel else c["hpel_cnt"],
                qpel_cnt=0 if ipel else c["qpel_cnt"], raster=c["raster"], refi=0)


def right_edge_crc():
    import zlib

    return [zlib.crc32(right_edge_ref_plane().tobytes())] + [zlib.crc32(right_edge_planes(S)["org"].tobytes()) for S in RE_SIZES]


RE_JOBS, RE_WRAPPED = 240, 144  # 48 launches of 5 jobs; the 3 targets beyond 32 767 of each
RE_SPEL_WRAPS = 140             # wrapped jobs whose diamond ends on a vector v with v + (x << 2) outside an s16 (counted on the reference's recorded results)


def assert_right_edge_conditions(entries):
    """entries: [((S, bi, preset), case, dia, twin_dia, epzs, twin_epzs)] of whole launches, the results being the reference's (or what is held to them).
    (a) three jobs of five in every launch have (x << 2) + mvp_x > 32 767; (b) in every launch -- every size, mode and preset -- every one of them ends elsewhere or at
    another cost than its twin, where nothing wraps, in the diamond and in the whole search (with the casts removed job and twin are one computation); the two controls
    of each launch, 32 764 and 32 767, equal their twins, so the twin is a fair control"""
    per = {}
    for L, c, dia, tdia, ep, tep in entries:
        n = per.setdefault(L, dict(jobs=0, wrapped=0, differ=0, control_differs=0))
        n["jobs"] += 1
        if right_edge_wrapped(c):
            assert not -32768 <= c["frame_x"] <= 32767 and c["gmvp"][0] == c["frame_x"] - 65536
            n["wrapped"] += 1
            n["differ"] += dia != tdia and ep != tep
        else:
            assert c["gmvp"][0] == c["frame_x"]
            n["control_differs"] += dia != tdia or ep != tep
    for L, n in per.items():
        assert n == dict(jobs=5, wrapped=RE_WRAPPED_PER_LAUNCH, differ=RE_WRAPPED_PER_LAUNCH, control_differs=0), (L, n)
    wrapped = sum(n["wrapped"] for n in per.values())
    assert 3 * wrapped >= sum(n["jobs"] for n in per.values())
    return wrapped


def spel_wraps(c, dia):
    """the vector the diamond ended on, made a frame coordinate again (cx = mvi + (x << 2), xeve_pinter.c:584), does not fit an s16"""
    return not -32768 <= dia[1] + (c["x"] << 2) <= 32767
