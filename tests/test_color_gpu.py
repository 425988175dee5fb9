"""xeve_hip_rgb_to_yuv420 and xeve_hip_yuv420_to_rgb on the GPU (xeve_amd/csrc/color.hip): RGB tensors of every element type and view -> the frames the encoder takes, and
the 10-bit pictures it hands out -> RGB, both EQUAL to the numpy / Fraction restatement of the definition (tests/_color.py) -- at the smallest sizes where a path can go
wrong (2x2: every tap clamps; one block column / row; odd chroma rows; 258 wide: more than one workgroup along a row), one and three pictures, pictures further apart
than their size, rows padded by slicing, every layout the kernels tell apart, an expanded grey tensor, outputs inside sentinel-filled buffers."""
import ctypes as C
import itertools

import numpy as np
import pytest

import _color as K

pytestmark = [pytest.mark.gpu, pytest.mark.gpu_full]

SETTINGS = list(itertools.product(K.MATRICES, (False, True), K.SITINGS, (8, 10)))  # rotated through: every one is met many times over the cases
FILL = 0xA5
# (name, layout, the base tensor's shape for n pictures of w x h, the view of it that is handed over): the kernels' interleaved, planar and strided paths, rows and
# pictures further apart than their content
VIEWS = [
    ("hwc", "hwc", lambda n, h, w: (n, h, w, 3), lambda b: b),
    ("chw", "chw", lambda n, h, w: (n, 3, h, w), lambda b: b),
    ("hwc padded rows", "hwc", lambda n, h, w: (n, h, w + 5, 3), lambda b: b[:, :, 2:-3]),
    ("chw padded rows", "chw", lambda n, h, w: (n, 3, h + 1, w + 6), lambda b: b[:, :, :-1, 3:-3]),
    ("hwc of rgba", "hwc", lambda n, h, w: (n, h, w, 4), lambda b: b[..., :3]),
    ("chw every second column and picture", "chw", lambda n, h, w: (2 * n, 3, h, 2 * w), lambda b: b[::2, :, :, ::2]),
]


@pytest.fixture(scope="module")
def dev():
    import torch

    import xeve_amd

    xeve_amd.init(0)
    return torch.device("cuda:0")


def _np_dtype(dtype):
    return {"uint8": np.uint8, "float16": np.float16, "bfloat16": np.float32, "float32": np.float32}[dtype]


def _to_torch(a, dtype, dev):
    """a numpy block as a device tensor of the element type (bfloat16: the float32 values hold bfloat16 values exactly)"""
    import torch

    t = torch.from_numpy(a).to(dev)
    return t.to(torch.bfloat16) if dtype == "bfloat16" else t


def _hwc(v, layout):
    """a stacked view as (n, h, w, 3)"""
    if layout == "hwc":
        return v
    return v.transpose(0, 2, 3, 1) if isinstance(v, np.ndarray) else v.permute(0, 2, 3, 1)


def _color(matrix, full, siting, depth):
    from xeve_amd import lib

    return lib.Color(K.MATRICES.index(matrix), int(full), K.SITINGS.index(siting), depth)


def _forward(view, layout, n, col, w, h, out_ptr, pic_bytes):
    from xeve_amd import encode, lib

    v = view if n > 1 else view[0]
    desc, dw, dh, dn = encode._rgb_desc(v, layout, n > 1)
    assert (dw, dh, dn) == (w, h, n)
    return lib.load().xeve_hip_rgb_to_yuv420(C.c_void_p(v.data_ptr()), C.byref(desc), C.byref(col), w, h, n, C.c_void_p(out_ptr), pic_bytes, None)


def _inverse(yuv_ptr, pic_samples, col, w, h, n, view, layout):
    from xeve_amd import encode, lib

    v = view if n > 1 else view[0]
    desc, _, _, _ = encode._rgb_desc(v, layout, n > 1)
    return lib.load().xeve_hip_yuv420_to_rgb(C.c_void_p(yuv_ptr), pic_samples, C.byref(col), w, h, n, C.c_void_p(v.data_ptr()), C.byref(desc), None)


@pytest.mark.parametrize("dtype", K.DTYPES)
@pytest.mark.parametrize("w,h", K.SHAPES)
def test_rgb_to_yuv420_equals_the_restatement(w, h, dtype, dev):
    """every view x one and three pictures; the frames start an odd number of samples into a buffer filled with 0xA5 and lie 5 samples further apart than their size:
    the whole buffer is compared, so a sample outside a frame that was written shows; the input is only read"""
    import torch

    rng = np.random.default_rng(w * 1000 + h * 10 + K.DTYPES.index(dtype))
    turn = itertools.count(rng.integers(0, len(SETTINGS)))
    for (name, layout, shape, cut), n in itertools.product(VIEWS, (1, 3)):
        matrix, full, siting, depth = SETTINGS[next(turn) % len(SETTINGS)]
        pics = np.stack([K.picture(rng, w, h, dtype) for _ in range(n)])
        base = np.zeros(shape(n, h, w), _np_dtype(dtype))
        _hwc(cut(base), layout)[:] = pics
        t = _to_torch(base, dtype, dev)
        sb = 2 if depth > 8 else 1
        per, lead, gap = w * h * 3 // 2 * sb, 3 * sb, 5 * sb
        out = torch.full((lead + n * (per + gap) + 64,), FILL, dtype=torch.uint8, device=dev)
        want = np.full(out.numel(), FILL, np.uint8)
        for p in range(n):
            want[lead + p * (per + gap):lead + p * (per + gap) + per] = K.forward_frame(pics[p], matrix, full, siting, depth).view(np.uint8)
        torch.cuda.synchronize()
        assert _forward(cut(t), layout, n, _color(matrix, full, siting, depth), w, h, out.data_ptr() + lead, per + gap) == 0
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want), (name, n, matrix, full, siting, depth)
        after = t.float().cpu().numpy() if dtype == "bfloat16" else t.cpu().numpy()
        assert np.array_equal(after, base, equal_nan=dtype != "uint8"), name


@pytest.mark.parametrize("dtype", K.DTYPES)
@pytest.mark.parametrize("w,h", K.SHAPES)
def test_yuv420_to_rgb_equals_the_restatement(w, h, dtype, dev):
    """the same views as OUTPUTS, cut out of tensors filled with a value no conversion produces: the whole base tensor is compared, so what lies between the rows, beside
    the components and between the pictures must survive; the pictures start 3 samples into their buffer and lie 7 samples further apart than their size"""
    import torch

    rng = np.random.default_rng(w * 1000 + h * 10 + 5 + K.DTYPES.index(dtype))
    turn = itertools.count(rng.integers(0, len(SETTINGS)))
    sentinel = 7 if dtype == "uint8" else -3.0
    per, lead, gap = w * h * 3 // 2, 3, 7
    for (name, layout, shape, cut), n in itertools.product(VIEWS, (1, 3)):
        matrix, full, siting, _ = SETTINGS[next(turn) % len(SETTINGS)]
        yuv = rng.integers(0, 1024, size=(n, per)).astype(np.int16)
        buf = np.full(lead + n * (per + gap), -1, np.int16)
        for p in range(n):
            buf[lead + p * (per + gap):lead + p * (per + gap) + per] = yuv[p]
        d_yuv = torch.from_numpy(buf).to(dev)
        base = np.full(shape(n, h, w), sentinel, _np_dtype(dtype))
        t = _to_torch(base, dtype, dev)
        torch.cuda.synchronize()
        assert _inverse(d_yuv.data_ptr() + 2 * lead, per + gap, _color(matrix, full, siting, 10), w, h, n, cut(t), layout) == 0
        torch.cuda.synchronize()
        pics = np.stack([K.inverse_frame(yuv[p], w, h, dtype, matrix, full, siting) for p in range(n)])
        if dtype == "bfloat16":  # compared as bit patterns
            want = torch.from_numpy(base).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).copy()
            got = t.view(torch.int16).cpu().numpy().view(np.uint16)
        else:
            want, got = base.copy(), t.cpu().numpy()
        _hwc(cut(want), layout)[:] = pics
        assert np.array_equal(got, want), (name, n, matrix, full, siting)
        assert np.array_equal(d_yuv.cpu().numpy(), buf)


@pytest.mark.parametrize("dtype", ("uint8", "float32"))
def test_an_expanded_grey_tensor_is_read_through_its_zero_stride(dtype, dev):
    """(h, w, 1).expand(h, w, 3) and (1, h, w).expand(3, h, w): stride_c = 0, nothing is copied; chroma is exactly the grey point"""
    import torch

    from xeve_amd import encode

    w, h = 70, 50
    rng = np.random.default_rng(3)
    grey = K.picture(rng, w, h, dtype)[..., :1]
    t = torch.from_numpy(grey.copy()).to(dev)
    want = K.forward_frame(np.repeat(grey, 3, axis=2), "bt601", False, "left", 10)
    for layout, view in (("hwc", t.expand(h, w, 3)), ("chw", t.permute(2, 0, 1).expand(3, h, w))):
        assert 0 in view.stride()
        got = encode.rgb_to_yuv420(view, depth=10, layout=layout, matrix="bt601")
        assert got.dtype == torch.int16 and np.array_equal(got.cpu().numpy().view(np.uint16), want), layout
    assert (want[w * h:] == 512).all()


def test_the_python_face_of_the_leaves(dev):
    """rgb_to_yuv420 / yuv420_to_rgb on tensors: shapes, dtypes, the leading axis, a host tensor moved by torch, the colour keywords"""
    import torch

    from xeve_amd import encode

    w, h = 6, 10
    rng = np.random.default_rng(9)
    pics = np.stack([K.picture(rng, w, h, "uint8") for _ in range(3)])
    kw = encode.color(matrix="bt2020nc", full_range=True, siting="centre")
    got = encode.rgb_to_yuv420(torch.from_numpy(pics), depth=8, **kw)  # (a host tensor)
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (3, w * h * 3 // 2)
    for p in range(3):
        assert np.array_equal(got[p].cpu().numpy(), K.forward_frame(pics[p], "bt2020nc", True, "centre", 8))
    ten = encode.rgb_to_yuv420(torch.from_numpy(pics).to(dev).permute(0, 3, 1, 2), depth=10, layout="chw", **kw)  # (a permuted view: no copy is made)
    assert ten.shape == (3, w * h * 3 // 2) and ten.dtype == torch.int16
    back = encode.yuv420_to_rgb(ten, w, h, torch.float16, "chw", **kw)
    assert back.shape == (3, 3, h, w) and back.dtype == torch.float16
    for p in range(3):
        frame = K.forward_frame(pics[p], "bt2020nc", True, "centre", 10)
        assert np.array_equal(ten[p].cpu().numpy().view(np.uint16), frame)
        assert np.array_equal(back[p].permute(1, 2, 0).cpu().numpy(), K.inverse_frame(frame, w, h, "float16", "bt2020nc", True, "centre"))
    one = encode.yuv420_to_rgb(ten[0], w, h, **kw)
    assert one.shape == (h, w, 3) and one.dtype == torch.uint8
    with pytest.raises(ValueError):
        encode.color(matrix="bt470")
    with pytest.raises(ValueError):
        encode.rgb_to_yuv420(torch.zeros((4, 4, 2), dtype=torch.uint8, device=dev))


def test_flat_blocks_come_back_within_one_step_of_uint8(dev):
    """uint8 RGB whose 2x2 blocks are flat -> depth 10 -> uint8 RGB: at most 1 apart, for every matrix, range and siting.  2000 pictures of 4x4, one colour each (the
    corners of the cube among them): the inverse interpolates chroma ACROSS blocks, so only a picture whose blocks are flat and alike loses nothing to the subsampling
    -- what is left is the two roundings.  The largest difference seen is printed"""
    import torch

    from xeve_amd import encode

    rng = np.random.default_rng(11)
    colours = rng.integers(0, 256, size=(2000, 3), dtype=np.uint8)
    colours[:8] = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255]]
    rgb = np.broadcast_to(colours[:, None, None, :], (2000, 4, 4, 3)).copy()
    t = torch.from_numpy(rgb).to(dev)
    worst = 0
    for matrix, full, siting in itertools.product(K.MATRICES, (False, True), K.SITINGS):
        kw = dict(matrix=matrix, full_range=full, siting=siting)
        back = encode.yuv420_to_rgb(encode.rgb_to_yuv420(t, depth=10, **kw), 4, 4, **kw).cpu().numpy()
        d = int(np.abs(back.astype(int) - rgb.astype(int)).max())
        worst = max(worst, d)
        assert d <= 1, (matrix, full, siting, d)
    print("largest round-trip difference over all settings: %d" % worst)


def test_arguments_outside_the_contract_are_refused(dev):
    """XEVE_HIP_ERR_ARG before any launch: odd or oversized pictures, a depth of 9 (the inverse: any depth but 10), an unknown element type, matrix, range or siting, no
    pictures, host memory on either side, a null descriptor, colour or pointer, misaligned tensors, frames that overlap, negative strides; for the inverse also a zero
    stride in the output"""
    import torch

    from xeve_amd import lib

    L = lib.load()
    w, h = 70, 50
    rgb = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
    yuv = torch.full((2 * w * h * 3,), 21, dtype=torch.int16, device=dev)
    host = np.zeros(w * h * 3 * 4, np.uint8)
    base = dict(rgb=rgb.data_ptr(), dtype=3, sx=3, sy=3 * w, sc=1, sp=0, matrix=1, full=0, siting=0, depth=10, w=w, h=h, n=1, yuv=yuv.data_ptr(), pic=w * h * 3, desc=True, color=True)
    bad = (dict(w=69), dict(h=51), dict(w=0), dict(w=8194), dict(h=4322), dict(depth=9), dict(depth=12), dict(dtype=7), dict(dtype=-1), dict(matrix=3), dict(full=2), dict(siting=2),
           dict(n=0), dict(n=65536), dict(rgb=host.ctypes.data), dict(yuv=host.ctypes.data), dict(rgb=None), dict(yuv=None), dict(desc=False), dict(color=False),
           dict(rgb=rgb.data_ptr() + 2), dict(yuv=yuv.data_ptr() + 1), dict(pic=w * h * 3 - 2), dict(pic=w * h * 3 + 1), dict(sx=-3), dict(sy=-1), dict(sp=-1))

    def call(k, inverse):
        desc = lib.RgbDesc(k["dtype"], 0, k["sx"], k["sy"], k["sc"], k["sp"])
        col = lib.Color(k["matrix"], k["full"], k["siting"], k["depth"])
        d, c = (C.byref(desc) if k["desc"] else None), (C.byref(col) if k["color"] else None)
        if inverse:
            return L.xeve_hip_yuv420_to_rgb(k["yuv"], k["pic"] // 2, c, k["w"], k["h"], k["n"], k["rgb"], d, None)
        return L.xeve_hip_rgb_to_yuv420(k["rgb"], d, c, k["w"], k["h"], k["n"], k["yuv"], k["pic"], None)

    for kw in bad:
        assert call(dict(base, **kw), False) == -2 and "invalid argument" in lib.last_error(), kw
    for kw in bad + (dict(depth=8), dict(sc=0), dict(sx=0), dict(n=2, sp=0)):
        if kw in (dict(pic=w * h * 3 + 1), dict(yuv=yuv.data_ptr() + 1)):  # (in samples: the inverse's frames cannot lie half a sample apart; an odd address is covered below)
            continue
        assert call(dict(base, **kw), True) == -2 and "invalid argument" in lib.last_error(), kw
    assert L.xeve_hip_yuv420_to_rgb(yuv.data_ptr() + 1, w * h * 3 // 2, C.byref(lib.Color(1, 0, 0, 10)), w, h, 1, rgb.data_ptr(), C.byref(lib.RgbDesc(3, 0, 3, 3 * w, 1, 0)), None) == -2
    torch.cuda.synchronize()
    assert not rgb.any() and bool((yuv == 21).all())
    assert call(base, False) == 0 and call(base, True) == 0  # (and the base of both lists is a call that runs)
    torch.cuda.synchronize()
