"""The closed-GOP batch encoder (include/xeve_hip.h: xeve_hip_enc_*; xeve_amd/csrc/encode.hip + enc_host.h): G independent runs of F frames each -- one closed GOP
per run, coded as the reference application codes `--seek g*F --frames F` -- advance in lockstep on the device; every run's bitstream is byte-identical to the
reference's.  This module is the ctypes face of it plus the file plumbing (YUV in, .evc out).  No CPU path: it raises when the library or the GPU is missing."""
import ctypes as C

from . import lib as _lib

PRESETS = {"fast": 0, "medium": 1, "slow": 2, "placebo": 3}
SLICE_TYPES = "BPI"  # XEVE_ST_B / _P / _I


def psnr(sse, samples, bit_depth=10):
    """the application's PSNR of a plane from its sum of squared differences (find_psnr_16bit: 100 when the planes are equal)"""
    import math

    mse = sse / samples
    return 100.0 if mse == 0 else abs(10 * math.log10(255 * 255 * (1 << (bit_depth - 8)) ** 2 / mse))


def stats_line(p):
    """one picture as the application's table prints it: POC Tid Ftype QP PSNR-Y PSNR-U PSNR-V Bits"""
    return "%-7d%-5d(%s)     %-5d%-10.4f%-10.4f%-10.4f%-10d" % (p["poc"], p["tid"], p["type"], p["qp"], p["psnr"][0], p["psnr"][1], p["psnr"][2], p["bytes"] * 8)


def config(w, h, qp=32, keyint=0, bframes=15, closed_gop=False, preset="medium", threads=1, fps=(30, 1), ref=0, always_second_pass=False, input_depth=8, level_idc=40, sei_info=True,
           inter_slice_type=0, qp_cb_offset=0, qp_cr_offset=0, measure=False, keep_recon=False, hash=False, crop=False, ssim=False):
    """the options of the reference application (xeve_app: -w -h -q -I -b --closed-gop --preset -m -z --ref -d; --inter-slice-type 0 B / 1 P, --qp-cb-offset,
    --qp-cr-offset as the reference LIBRARY takes them) as the library's configuration record.  measure: per-picture SSE / PSNR (BatchEncoder.pictures);
    keep_recon: the reconstructed pictures stay on the device (BatchEncoder.recon; w * h * 3 bytes per picture of the batch) -- neither changes the bitstream.
    hash: the application's --hash -- a 56-byte picture-signature SEI with the MD5 of each decoded plane behind every picture (BatchEncoder.signatures), hash=1 in the
    option SEI; the digests are made on the device.  crop: w and h may be any even size (960x540, 1366x768) -- the picture is coded at the next multiples of 8 with zeros
    right of the input and below it and a cropping window in the SPS, as the reference codes it; frames are pushed and recon() is handed out at w x h, PSNR and the hash
    digests run over the coded planes as the application's do.  Without it a size that is no multiple of 8 is refused.  ssim: per-picture SSIM of the SHOWN w x h window
    (BatchEncoder.ssim; exact integer sums made on the device, stated in include/xeve_hip.h; 24 bytes per picture of the batch; w and h at least 16) -- independent of
    measure and keep_recon, and no byte of the bitstream changes"""
    c = _lib.EncConfig()
    c.w, c.h, c.fps_num, c.fps_den, c.qp, c.keyint, c.bframes, c.closed_gop = w, h, fps[0], fps[1], qp, keyint, bframes, int(bool(closed_gop))
    c.preset, c.threads, c.inter_slice_type, c.ref = PRESETS[preset] if isinstance(preset, str) else int(preset), threads, int(inter_slice_type), ref
    c.reserved[2], c.reserved[3] = int(qp_cb_offset), int(qp_cr_offset)
    c.reserved[0] = (1 if always_second_pass else 0) | (0 if sei_info else 2) | (4 if measure else 0) | (8 if keep_recon else 0) | (16 if hash else 0) | (32 if crop else 0) | (64 if ssim else 0) | ((int(level_idc) & 0xFF) << 8)  # (--info 0, --level-idc)
    c.reserved[1] = int(input_depth)
    return c


MATRICES = {"bt601": 0, "bt709": 1, "bt2020nc": 2}
SITINGS = {"left": 0, "centre": 1}
LAYOUTS = ("hwc", "chw")


def color(matrix="bt709", full_range=False, siting="left"):
    """the colour keywords of every RGB call below, checked, as a dict to pass on with ** : the matrix ("bt601", "bt709", "bt2020nc"), the range of the Y'CbCr side
    (limited 16 .. 235 / 240 scaled to the depth, or full) and where a chroma sample sits ("left": co-sited with the even luma columns, chroma_sample_loc_type 0, what
    decoders assume when nothing is signalled; "centre": in the middle of its 2x2 block).  THE BITSTREAM CARRIES NO COLOUR DESCRIPTION -- the reference's default streams
    carry none and this encoder writes no VUI: whoever consumes the stream (the container, the player's settings) has to be told these three things."""
    if matrix not in MATRICES or siting not in SITINGS:
        raise ValueError("matrix is one of %s, siting one of %s" % (sorted(MATRICES), sorted(SITINGS)))
    return {"matrix": matrix, "full_range": bool(full_range), "siting": siting}


def _color(depth, **kw):
    k = color(**kw)
    return _lib.Color(MATRICES[k["matrix"]], int(k["full_range"]), SITINGS[k["siting"]], int(depth))


def _rgb_desc(tensor, layout, stacked):
    """(xeve_hip_rgb_desc of the view as it is -- tensor.stride(), no copy --, w, h, pictures)"""
    import torch

    dtypes = {torch.uint8: 0, torch.float16: 1, torch.bfloat16: 2, torch.float32: 3}
    if layout not in LAYOUTS or tensor.dtype not in dtypes or tensor.dim() != (4 if stacked else 3):
        raise ValueError("an RGB tensor is uint8 / float16 / bfloat16 / float32 of shape %s%s" % ("(N, " if stacked else "(", "H, W, 3) for 'hwc', 3, H, W) for 'chw'"))
    shape, stride = list(tensor.shape), list(tensor.stride())
    n, sp = (shape.pop(0), stride.pop(0)) if stacked else (1, 0)
    (h, w, c), (sy, sx, sc) = (shape, stride) if layout == "hwc" else ((shape[1], shape[2], shape[0]), (stride[1], stride[2], stride[0]))
    if c != 3:
        raise ValueError("the component axis of an RGB tensor has length 3")
    return _lib.RgbDesc(dtypes[tensor.dtype], 0, sx, sy, sc, sp), w, h, n


def _on_gpu(tensor):
    import torch

    return tensor if tensor.is_cuda else tensor.to(torch.device("cuda", torch.cuda.current_device()))


def rgb_to_yuv420(tensor, depth=10, layout="hwc", **color_kw):
    """RGB -> the planar 4:2:0 frame BatchEncoder.push takes (xeve_hip_rgb_to_yuv420), on the tensor's GPU and torch's current stream.  tensor: (H, W, 3) / (3, H, W), or with
    a leading axis of pictures; any view (strides are passed on, nothing is made contiguous); a host tensor is moved first.  Returns a uint8 (depth 8) or int16 (depth 10)
    tensor of w * h * 3 / 2 samples per picture: Y, then U, then V.  color_kw: see color()"""
    import torch

    tensor = _on_gpu(tensor)
    stacked = tensor.dim() == 4
    desc, w, h, n = _rgb_desc(tensor, layout, stacked)
    col = _color(depth, **color_kw)
    per = w * h * 3 // 2
    out = torch.empty((n, per) if stacked else (per,), dtype=torch.int16 if depth > 8 else torch.uint8, device=tensor.device)
    with torch.cuda.device(tensor.device):
        _lib.check(_lib.load().xeve_hip_rgb_to_yuv420(C.c_void_p(tensor.data_ptr()), C.byref(desc), C.byref(col), w, h, n, C.c_void_p(out.data_ptr()), per * out.element_size(),
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def yuv420_to_rgb(yuv, w, h, dtype=None, layout="hwc", **color_kw):
    """the 10-bit planar 4:2:0 pictures BatchEncoder.recon_into fills -> RGB (xeve_hip_yuv420_to_rgb), on torch's current stream.  yuv: a contiguous int16 tensor of
    w * h * 3 / 2 samples, or (N, w * h * 3 / 2) for N pictures.  Returns (H, W, 3) / (3, H, W) of dtype (torch.uint8 by default), with the leading axis when yuv has one"""
    import torch

    yuv = _on_gpu(yuv)
    per = w * h * 3 // 2
    if yuv.dtype != torch.int16 or not yuv.is_contiguous() or yuv.dim() not in (1, 2) or yuv.shape[-1] != per:
        raise ValueError("yuv is a contiguous int16 tensor of w * h * 3 / 2 samples per picture")
    stacked = yuv.dim() == 2
    shape = (h, w, 3) if layout == "hwc" else (3, h, w)
    out = torch.empty(((yuv.shape[0],) if stacked else ()) + shape, dtype=dtype or torch.uint8, device=yuv.device)
    desc, _, _, n = _rgb_desc(out, layout, stacked)
    col = _color(10, **color_kw)
    with torch.cuda.device(yuv.device):
        _lib.check(_lib.load().xeve_hip_yuv420_to_rgb(C.c_void_p(yuv.data_ptr()), per, C.byref(col), w, h, n, C.c_void_p(out.data_ptr()), C.byref(desc),
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def color_matrix(depth=10, **color_kw):
    """the integer coefficients of a colour setting (xeve_hip_color_matrix; no device call): (fwd[9]: rows Y, Cb, Cr over R, G, B; (oY, oC); inv: iY, rCr, gCb, gCr, bCb)"""
    col = _color(depth, **color_kw)
    fwd, off, inv = (C.c_int64 * 9)(), (C.c_int64 * 2)(), (C.c_int64 * 5)()
    _lib.check(_lib.load().xeve_hip_color_matrix(C.byref(col), fwd, off, inv))
    return list(fwd), tuple(off), list(inv)


def _surface(y, uv, msb_aligned, stacked):
    """(xeve_hip_surface of the tensors as they are -- pitches and picture distances from tensor.stride(), no copy --, sw, sh, pictures, depth, the tensors kept alive).
    y: (H, W) samples, or (N, H, W) when stacked; uv: ONE tensor (H/2, W/2, 2) of interleaved U, V pairs (NV12 / P010), or a (u, v) pair of (H/2, W/2) planes.  uint8 holds
    8 bits; int16 / uint16 hold 10, in the low bits or with msb_aligned in the top bits"""
    import torch

    semi = hasattr(uv, "data_ptr")
    planes = [y, uv] if semi else [y] + list(uv)
    words = (torch.int16,) + ((torch.uint16,) if hasattr(torch, "uint16") else ())
    lead = 1 if stacked else 0
    if len(planes) != (2 if semi else 3) or any(p.dtype != y.dtype or p.device != y.device for p in planes) or y.dtype not in (torch.uint8,) + words:
        raise ValueError("a surface is y and uv (one interleaved tensor or a (u, v) pair), all uint8 or all int16 / uint16, on one device")
    if y.dim() != lead + 2 or any(p.dim() != lead + (3 if semi else 2) for p in planes[1:]):
        raise ValueError("y is (H, W), uv (H/2, W/2, 2) or a pair of (H/2, W/2)%s" % (", each behind a leading axis of pictures" if stacked else ""))
    es = y.element_size()
    depth = 8 if es == 1 else 10
    if msb_aligned and es == 1:
        raise ValueError("msb_aligned needs 16-bit words")
    sh, sw = int(y.shape[lead]), int(y.shape[lead + 1])
    n = int(y.shape[0]) if stacked else 1
    chroma = (sh // 2, sw // 2, 2) if semi else (sh // 2, sw // 2)
    for p in planes[1:]:
        if tuple(p.shape[lead:]) != chroma or (stacked and p.shape[0] != n):
            raise ValueError("the chroma of a %dx%d surface is %s" % (sw, sh, "x".join(map(str, chroma))))
    cs = planes[1].stride()
    if y.stride(-1) != 1 or cs[-1] != 1 or (semi and cs[-2] != 2) or any(p.stride() != cs for p in planes[2:]):
        raise ValueError("the samples of a row are neighbours in memory (an interleaved pair's as well), and u and v share their strides")
    s = _lib.Surface(1 if semi else 0, es, depth, (16 - depth) if msb_aligned else 0)
    for i, p in enumerate(planes):
        s.plane[i] = p.data_ptr()
    s.pitch_l, s.pitch_c = y.stride(lead) * es, cs[lead] * es
    s.pic_l, s.pic_c = (y.stride(0) * es, cs[0] * es) if stacked else (0, 0)
    return s, sw, sh, n, depth, planes


def surface_to_yuv420(y, uv, w, h, msb_aligned=False, siting="left"):
    """a decoder's surface -- NV12 / P010 (uv one (H/2, W/2, 2) tensor) or planar (uv a (u, v) pair), rows a pitch apart as tensor.stride() says, at the SOURCE's size -- ->
    the planar 4:2:0 frame BatchEncoder.push takes at w x h (xeve_hip_surface_to_yuv420): de-interleaved, shifted and resampled (stretched Catmull-Rom, all integer; stated
    in include/xeve_hip.h) in one kernel per plane, on the tensors' GPU and torch's current stream.  A leading axis of pictures on every tensor converts them at once.
    Returns a uint8 (depth 8) or int16 (depth 10) tensor of w * h * 3 / 2 samples per picture: Y, then U, then V.  A same-size call only de-interleaves, shifts and drops
    the pitch"""
    import torch

    if siting not in SITINGS:
        raise ValueError("siting is one of %s" % sorted(SITINGS))
    stacked = y.dim() == 3
    s, sw, sh, n, depth, keep = _surface(y, uv, msb_aligned, stacked)
    per = w * h * 3 // 2
    out = torch.empty((n, per) if stacked else (per,), dtype=torch.int16 if depth > 8 else torch.uint8, device=y.device)
    with torch.cuda.device(y.device):
        _lib.check(_lib.load().xeve_hip_surface_to_yuv420(C.byref(s), sw, sh, SITINGS[siting], int(w), int(h), depth, n, C.c_void_p(out.data_ptr()), per * out.element_size(),
                                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def scale_filter(src_n, dst_n, kind=0):
    """the scaler's table of one axis (xeve_hip_scale_filter; no device call): (first, coef, ntaps) -- per destination index its lowest tap and ntaps coefficients at 14
    fractional bits, every row summing to 16384.  kind 0: src_n -> dst_n samples of a plane; kind 1: the left-sited chroma columns of a picture src_n -> dst_n LUMA samples
    wide (dst_n / 2 rows)"""
    rows = max(1, int(dst_n) // 2 if kind == 1 else int(dst_n))
    first, coef, ntaps = (C.c_int32 * rows)(), (C.c_int16 * (rows * 33))(), C.c_int()
    _lib.check(_lib.load().xeve_hip_scale_filter(int(src_n), int(dst_n), int(kind), first, coef, rows * 33, C.byref(ntaps)))
    t = ntaps.value
    return list(first), [list(coef[i * t:(i + 1) * t]) for i in range(rows)], t


def ssim_windows(w, h):
    """the 8x8 windows of the planes Y, U, V of a w x h picture: (bx - 1)(by - 1) with 4x4 blocks cut from a plane's top left (include/xeve_hip.h)"""
    return [((pw >> 2) - 1) * ((ph >> 2) - 1) for pw, ph in ((w, h), (w // 2, h // 2), (w // 2, h // 2))]


def _ssim_operand(t, n, w, h):
    """pictures in the recon() layout as the leaf takes planes: in place where the rows are 16-byte (8-byte) aligned as they lie, else (a width that is no multiple of 8) copied into
    planes whose rows are: (tensors to keep alive, three addresses, (luma, chroma) strides, (luma, chroma) picture distances)"""
    import torch

    if t.dtype == torch.uint8:
        t = t.view(torch.int16)
    per = w * h * 3 // 2
    if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.int16 and t.numel() == n * per):
        raise ValueError("ssim_planes takes contiguous int16 (or uint8-viewed) device tensors of w * h * 3 / 2 samples per picture")
    nl, nc = w * h, w * h // 4
    if w % 8 == 0:
        return [t], [t.data_ptr(), t.data_ptr() + 2 * nl, t.data_ptr() + 2 * (nl + nc)], (w, w // 2), (per, per)
    t, sl = t.view(n, per), (w + 7) & ~7
    planes = [torch.zeros((n, h, sl), dtype=torch.int16, device=t.device), torch.zeros((n, h // 2, sl // 2), dtype=torch.int16, device=t.device),
              torch.zeros((n, h // 2, sl // 2), dtype=torch.int16, device=t.device)]
    planes[0][:, :, :w] = t[:, :nl].view(n, h, w)
    planes[1][:, :, :w // 2] = t[:, nl:nl + nc].view(n, h // 2, w // 2)
    planes[2][:, :, :w // 2] = t[:, nl + nc:].view(n, h // 2, w // 2)
    return planes, [p.data_ptr() for p in planes], (sl, sl // 2), (h * sl, h // 2 * (sl // 2))


def ssim_planes(rec, org, w, h):
    """the SSIM sums of pictures against their originals (xeve_hip_ssim_planes; include/xeve_hip.h states the arithmetic): rec and org are device tensors holding one
    picture, or with a leading axis several, in the layout BatchEncoder.recon() hands out -- planar Y, U, V of w x h at the codec's 10 bits, int16 (or the same bytes as
    uint8).  Returns an int64 device tensor [3] / [n, 3] of the exact sums Q, made on torch's current stream; ssim = Q / (ssim_windows(w, h)[plane] * 2 ** 30).  A width
    that is no multiple of 8 is first copied into planes with aligned rows"""
    import torch

    per = w * h * 3 // 2
    stacked = rec.dim() > 1
    n = rec.numel() * rec.element_size() // (2 * per)
    if n < 1 or org.device != rec.device:
        raise ValueError("rec and org hold the same number of w x h pictures on one device")
    keep_r, pr, sr, dr = _ssim_operand(rec, n, w, h)
    keep_o, po, so, do = _ssim_operand(org, n, w, h)
    sums = torch.empty((n, 3), dtype=torch.int64, device=rec.device)
    with torch.cuda.device(rec.device):
        _lib.check(_lib.load().xeve_hip_ssim_planes((C.c_void_p * 3)(*pr), sr[0], sr[1], dr[0], dr[1], (C.c_void_p * 3)(*po), so[0], so[1], do[0], do[1], int(w), int(h), n,
                                                    C.c_void_p(sums.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    del keep_r, keep_o  # (copies made on this stream and read on it: the allocator hands their memory out again in stream order)
    return sums if stacked else sums[0]


class BatchEncoder:
    """enc = BatchEncoder(cfg, ngops, frames); enc.push(g, f, frame_bytes | device tensor) ...; streams = enc.encode()"""

    def __init__(self, cfg, ngops, frames):
        L = _lib.load()
        self._L, self.cfg, self.ngops, self.frames = L, cfg, ngops, frames
        self.frame_bytes = cfg.w * cfg.h * 3 // 2 * (2 if cfg.reserved[1] > 8 else 1)
        self._h = L.xeve_hip_enc_create(C.byref(cfg), ngops, frames)
        if not self._h:
            raise _lib.XeveHipError(_lib.last_error())

    def close(self):
        if self._h:
            self._L.xeve_hip_enc_delete(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def push(self, gop, frame, data):
        """data: bytes-like of one planar 4:2:0 frame (host; one byte per sample, two little-endian with input_depth 10), or a uint8 torch tensor of those bytes on the GPU"""
        if hasattr(data, "data_ptr"):
            assert data.numel() == self.frame_bytes and data.is_contiguous()
            if data.is_cuda:  # the library copies on its own stream: whatever produced the tensor on torch's stream must be through
                import torch

                torch.cuda.current_stream(data.device).synchronize()
            _lib.check(self._L.xeve_hip_enc_push(self._h, gop, frame, C.c_void_p(data.data_ptr()), 1 if data.is_cuda else 0))
        else:
            b = bytes(data)
            assert len(b) == self.frame_bytes
            _lib.check(self._L.xeve_hip_enc_push(self._h, gop, frame, b, 0))

    def push_gop(self, gop, data):
        for f in range(self.frames):
            self.push(gop, f, data[f * self.frame_bytes:(f + 1) * self.frame_bytes])

    def push_rgb(self, gop, frame, tensor, layout="hwc", **color_kw):
        """one RGB picture of w x h -- (H, W, 3) for "hwc", (3, H, W) for "chw"; uint8, float16, bfloat16 or float32 (floats in [0, 1]); any view, nothing is copied to make
        it contiguous -- converted on the device straight into the frame's place (xeve_hip_enc_push_rgb) at the run's input depth.  A host tensor is moved to the GPU first.
        color_kw: color()'s keywords; the stream carries no colour description, so the consumer has to be told them"""
        import torch

        tensor = _on_gpu(tensor)
        desc, w, h, _ = _rgb_desc(tensor, layout, False)
        if (w, h) != (self.cfg.w, self.cfg.h):
            raise ValueError("the picture is %dx%d, the run's input %dx%d" % (w, h, self.cfg.w, self.cfg.h))
        col = _color(10 if self.cfg.reserved[1] > 8 else 8, **color_kw)
        torch.cuda.current_stream(tensor.device).synchronize()  # (the library converts on its own stream: whatever produced the tensor on torch's must be through)
        _lib.check(self._L.xeve_hip_enc_push_rgb(self._h, int(gop), int(frame), C.c_void_p(tensor.data_ptr()), C.byref(desc), C.byref(col)))

    def push_surface(self, gop, frame, y, uv, msb_aligned=False, siting="left"):
        """one decoded picture of ANY accepted size (even, 2 .. 8192 x 2 .. 4320, within 8 : 1 of the run's per axis) -- y (H, W) with uv (H/2, W/2, 2) for NV12 / P010 or a
        (u, v) pair; uint8 for a run of input depth 8, int16 / uint16 for depth 10 (msb_aligned: the sample in the top bits, as P010 has it); rows a pitch apart as
        tensor.stride() says -- scaled on the device straight into the frame's place at the run's input size (xeve_hip_enc_push_surface); see surface_to_yuv420"""
        import torch

        if siting not in SITINGS:
            raise ValueError("siting is one of %s" % sorted(SITINGS))
        s, sw, sh, _, depth, keep = _surface(y, uv, msb_aligned, False)
        if depth != (10 if self.cfg.reserved[1] > 8 else 8):
            raise ValueError("a run of input depth 10 takes int16 / uint16 surfaces, one of depth 8 uint8")
        torch.cuda.current_stream(y.device).synchronize()  # (the library converts on its own stream: whatever produced the tensors on torch's must be through)
        _lib.check(self._L.xeve_hip_enc_push_surface(self._h, int(gop), int(frame), C.byref(s), sw, sh, SITINGS[siting]))

    def push_video_rgb(self, gop, tensor, layout="hwc", **color_kw):
        """the run's pictures at once: the leading axis of the tensor is the frames"""
        if tensor.shape[0] != self.frames:
            raise ValueError("the leading axis holds %d pictures, a run %d" % (tensor.shape[0], self.frames))
        for f in range(self.frames):
            self.push_rgb(gop, f, tensor[f], layout, **color_kw)

    def recon_rgb(self, gop, frame, dtype=None, layout="hwc", out=None, **color_kw):
        """the reconstructed picture (config(keep_recon=True)) as RGB, converted on the device from the kept picture (xeve_hip_enc_recon_rgb): a new (H, W, 3) / (3, H, W)
        tensor of dtype (torch.uint8 by default) on the encoder's GPU, or `out` -- any view of that shape on that GPU; complete when the call returns"""
        import torch

        if out is None:
            out = torch.empty((self.cfg.h, self.cfg.w, 3) if layout == "hwc" else (3, self.cfg.h, self.cfg.w), dtype=dtype or torch.uint8, device=torch.device("cuda", torch.cuda.current_device()))
        desc, w, h, _ = _rgb_desc(out, layout, False)
        if (w, h) != (self.cfg.w, self.cfg.h) or not out.is_cuda:
            raise ValueError("out is a %dx%d picture on the encoder's GPU" % (self.cfg.w, self.cfg.h))
        col = _color(10, **color_kw)
        torch.cuda.current_stream(out.device).synchronize()  # (nothing queued on torch's stream may still use the tensor)
        _lib.check(self._L.xeve_hip_enc_recon_rgb(self._h, int(gop), int(frame), C.c_void_p(out.data_ptr()), C.byref(desc), C.byref(col)))
        return out

    def begin(self):
        _lib.check(self._L.xeve_hip_enc_begin(self._h))

    def advance(self, max_steps):
        """issues up to max_steps lockstep steps (one CTU of every row chain of every GOP each); returns the steps still to do"""
        left = C.c_int64()
        _lib.check(self._L.xeve_hip_enc_advance(self._h, int(max_steps), C.byref(left)))
        return left.value

    def sync(self):
        _lib.check(self._L.xeve_hip_enc_sync(self._h))

    def flush(self):
        """appends the access unit still outstanding (a picture's is appended when the next picture ends): bitstream() then holds every picture whose steps were issued"""
        _lib.check(self._L.xeve_hip_enc_flush(self._h))

    def bitstream(self, gop):
        """the bitstream of one GOP (bytes)"""
        p, n = C.c_void_p(), C.c_size_t()
        _lib.check(self._L.xeve_hip_enc_bitstream(self._h, gop, C.byref(p), C.byref(n)))
        return C.string_at(p.value, n.value) if n.value else b""

    def bitstream_sizes(self):
        out = []
        for g in range(self.ngops):
            p, n = C.c_void_p(), C.c_size_t()
            _lib.check(self._L.xeve_hip_enc_bitstream(self._h, g, C.byref(p), C.byref(n)))
            out.append(int(n.value))
        return out

    def bitstreams(self):
        return [self.bitstream(g) for g in range(self.ngops)]

    def encode(self):
        """codes every run; returns the list of bitstreams (bytes), one per GOP"""
        _lib.check(self._L.xeve_hip_enc_encode(self._h))
        out = []
        for g in range(self.ngops):
            p, n = C.c_void_p(), C.c_size_t()
            _lib.check(self._L.xeve_hip_enc_bitstream(self._h, g, C.byref(p), C.byref(n)))
            out.append(C.string_at(p.value, n.value) if n.value else b"")
        return out

    def picture(self, gop, frame):
        """the application's table row of one picture (config(measure=True)) -- xeve_hip_enc_picture_info; raises for a picture whose access unit is not in the bitstream yet"""
        p = _lib.EncPicture()
        _lib.check(self._L.xeve_hip_enc_picture_info(self._h, int(gop), int(frame), C.byref(p)))
        row = {"frame": p.frame, "poc": p.poc, "type": SLICE_TYPES[p.slice_type], "tid": p.tid, "qp": p.qp, "idr": bool(p.idr), "coding_pos": p.coding_pos, "bytes": int(p.bytes),
               "sse": [int(v) for v in p.sse], "psnr": [float(v) for v in p.psnr]}
        if self.cfg.reserved[0] & 16:  # (bytes stays the application's Bits / 8: the signature unit is not counted)
            row["md5"] = [d.hex() for d in self.signatures(gop, frame)]
        if self.cfg.reserved[0] & 64:
            row["ssim"] = self.ssim(gop, frame)["ssim"]
        return row

    def ssim(self, gop, frame=None):
        """the SSIM of one picture's shown w x h window (config(ssim=True)) -- xeve_hip_enc_picture_ssim: {"sums": the exact integer Q of planes Y, U, V, "windows": their
        window counts n, "ssim": Q / (n * 2 ** 30)}, or with frame=None a list of those for every frame in display order; raises for a picture whose access unit is not in
        the bitstream yet"""
        out = []
        for f in (range(self.frames) if frame is None else [int(frame)]):
            q, n, s = (C.c_int64 * 3)(), (C.c_int64 * 3)(), (C.c_double * 3)()
            _lib.check(self._L.xeve_hip_enc_picture_ssim(self._h, int(gop), f, q, n, s))
            out.append({"sums": [int(v) for v in q], "windows": [int(v) for v in n], "ssim": [float(v) for v in s]})
        return out if frame is None else out[0]

    def signatures(self, gop, frame=None):
        """the MD5 of the decoded Y, U and V plane (config(hash=True)) -- what the picture's signature SEI carries and hashlib.md5 gives for the planes of recon(): three
        16-byte digests of one frame, or with frame=None a list of those for every frame in display order; raises for a picture whose access unit is not in the bitstream yet"""
        out = []
        for f in (range(self.frames) if frame is None else [int(frame)]):
            buf = (C.c_uint8 * 48)()
            _lib.check(self._L.xeve_hip_enc_signature(self._h, int(gop), f, buf))
            out.append([bytes(buf[16 * c:16 * c + 16]) for c in range(3)])
        return out if frame is None else out[0]

    def pictures(self, gop):
        """every picture of one GOP in display order (a list of dicts: frame, poc, type 'I' / 'P' / 'B', tid, qp, idr, coding_pos, bytes, sse[3], psnr[3]; with
        config(hash=True) also md5: the three planes' digests as hex)"""
        return [self.picture(gop, f) for f in range(self.frames)]

    def recon(self, gop, frame=None):
        """the reconstructed picture (config(keep_recon=True)) as the application's -r writes it: planar Y, U, V, cropped, 16-bit little-endian samples at the codec's 10 bits
        (w * h * 3 bytes); frame=None: the whole run in display order -- that run's -r file"""
        n = self.cfg.w * self.cfg.h * 3
        frames = range(self.frames) if frame is None else [int(frame)]
        buf = C.create_string_buffer(n * len(frames))
        for i, f in enumerate(frames):
            _lib.check(self._L.xeve_hip_enc_recon(self._h, int(gop), f, C.byref(buf, i * n), 0))
        return buf.raw

    def recon_into(self, gop, frame, tensor):
        """the same picture, device to device, into a contiguous uint8 / int16 torch tensor of w * h * 3 bytes on the encoder's GPU (complete when the call returns)"""
        import torch

        assert tensor.is_cuda and tensor.is_contiguous() and tensor.dtype in (torch.uint8, torch.int16)
        assert tensor.numel() * tensor.element_size() == self.cfg.w * self.cfg.h * 3  # (the library refuses memory of another GPU than the encoder's)
        torch.cuda.current_stream(tensor.device).synchronize()  # (the library copies on its own stream: nothing queued on torch's may still use the tensor)
        _lib.check(self._L.xeve_hip_enc_recon(self._h, int(gop), int(frame), C.c_void_p(tensor.data_ptr()), 1))
        return tensor

    def stats(self):
        steps, a, b = C.c_int64(), C.c_double(), C.c_double()
        _lib.check(self._L.xeve_hip_enc_stats(self._h, C.byref(steps), C.byref(a), C.byref(b)))
        return {"ctu_steps": steps.value, "step_seconds": a.value, "picture_end_seconds": b.value}


class walk_select:
    """with walk_select(0 | 1 | -1, chains_per_team=0, side=-1): ... -- pins the composed walk (0) / the fused kernel (1) / the choice by width (-1) for the encoders created
    inside, optionally how many chains a team of the fused kernel carries, and whether the composed walk uses its side stream (1 / 0; -1 leaves it as it is)
    (xeve_hip_walk_select / _team / _side: process-wide; create AND close the encoder inside)"""

    def __init__(self, mode, chains_per_team=0, side=-1):
        self.mode, self.team, self.side = int(mode), int(chains_per_team), int(side)

    def __enter__(self):
        L = _lib.load()
        self.before, self.team_before, self.side_before = L.xeve_hip_walk_select(self.mode), L.xeve_hip_walk_team(self.team), L.xeve_hip_walk_side(self.side)
        return self

    def __exit__(self, *exc):
        L = _lib.load()
        L.xeve_hip_walk_select(self.before), L.xeve_hip_walk_team(self.team_before), L.xeve_hip_walk_side(self.side_before)
        return False


def signature_sei(tid, digests):
    """the 56-byte picture-signature SEI NAL unit of --hash for a temporal id and three 16-byte digests (Y, U, V) -- xeve_hip_signature_sei; no device call"""
    d = b"".join(bytes(x) for x in digests)
    assert len(d) == 48
    out = (C.c_uint8 * _lib.SIGNATURE_SEI_BYTES)()
    n = _lib.load().xeve_hip_signature_sei(int(tid), d, out, len(out))
    if n != _lib.SIGNATURE_SEI_BYTES:
        raise _lib.XeveHipError("libxeve_hip rc=%d: %s" % (n, _lib.last_error()))
    return bytes(out)


def split_nal_units(bitstream):
    """[(nal unit type, temporal id, payload behind the two header bytes)] of a bitstream as the encoder writes it: every unit behind a 4-byte big-endian length
    (xeve_eco_nal_unit_len).  Raises unless the units consume the bitstream exactly.  Types: 0 non-IDR slice, 1 IDR slice, 24 SPS, 25 PPS, 28 SEI."""
    units, at, n = [], 0, len(bitstream)
    while at < n:
        if at + 4 > n:
            raise ValueError("a NAL unit's length field is cut short at byte %d" % at)
        size = int.from_bytes(bitstream[at:at + 4], "big")
        if size < 2 or at + 4 + size > n:
            raise ValueError("the NAL unit at byte %d says %d bytes; %d are left" % (at, size, n - at - 4))
        head = int.from_bytes(bitstream[at + 4:at + 6], "big")  # forbidden_zero_bit, nal_unit_type_plus1 (6), nuh_temporal_id (3), reserved (5), extension (1)
        units.append((((head >> 9) & 0x3F) - 1, (head >> 6) & 7, bytes(bitstream[at + 6:at + 4 + size])))
        at += 4 + size
    return units


def read_signatures(bitstream):
    """[(temporal id, [md5 of Y, of U, of V])] per picture, in coding order, from the picture-signature SEI units of a bitstream coded with --hash (payload type 0x10, the
    size byte 0x10, three 16-byte digests); a bitstream without them gives an empty list"""
    return [(tid, [p[2 + 16 * c:18 + 16 * c] for c in range(3)]) for nut, tid, p in split_nal_units(bitstream) if nut == 28 and len(p) == 50 and p[:2] == b"\x10\x10"]


def footprint(cfg, ngops, frames):
    """(device bytes a batch of ngops x frames takes, the most GOPs one batch can hold at this picture size) -- xeve_hip_enc_footprint; no device call"""
    L = _lib.load()
    b, m = C.c_uint64(), C.c_int32()
    _lib.check(L.xeve_hip_enc_footprint(C.byref(cfg), int(ngops), int(frames), C.byref(b), C.byref(m)))
    return int(b.value), int(m.value)


def slice_capacity(cfg, frames):
    """the bytes one picture's slice data may take on the device, per GOP (sized by the run's lowest slice QP) -- xeve_hip_enc_slice_capacity; no device call"""
    L = _lib.load()
    b = C.c_uint64()
    _lib.check(L.xeve_hip_enc_slice_capacity(C.byref(cfg), int(frames), C.byref(b)))
    return int(b.value)


def plan_batches(cfg, ngops, frames, free_bytes, max_batches=3, reserve_bytes=8 << 30, batch_gops=None):
    """How `ngops` GOPs are cut into batches that run side by side on one GPU (a host thread and a stream each): as few batches as the per-batch limit (32-bit offsets into
    the stacked originals) and the free HBM allow, at most max_batches AT A TIME -- what is left over waits for the next round.  Returns a list of rounds, each a list of
    (first GOP, GOPs).  A step's time hardly depends on the chains it carries and the device runs the batches' launch chains side by side, so frames/s grows with the
    GOPs in flight (profiles/r03t_*): a round is filled as far as the memory goes.  batch_gops: a lower cap on a batch than the library's (tests)."""
    one, most = footprint(cfg, 1, frames)
    if batch_gops:
        most = min(most, int(batch_gops))
    two, _ = footprint(cfg, 2, frames)
    per_gop, fixed = max(1, two - one), max(0, 2 * one - two)
    rounds, at = [], 0
    while at < ngops:
        room, batches = free_bytes - reserve_bytes, []
        while at < ngops and len(batches) < max_batches:
            g = int(min(most, ngops - at, (room - fixed) // per_gop))
            if g < 1:
                break
            batches.append((at, g))
            at += g
            room -= fixed + g * per_gop
        if not batches:
            raise _lib.XeveHipError("not enough device memory for a single GOP of this size")
        rounds.append(batches)
    return rounds


def encode_gops(cfg, ngops, frames, feed, free_bytes=None, max_batches=3, batch_gops=None, collect=None):
    """codes `ngops` closed GOPs of `frames` pictures each on the current GPU and returns their bitstreams in order.  feed(encoder, first_gop, count) pushes the frames of
    GOPs [first_gop, first_gop + count) into `encoder` as its GOPs 0 .. count - 1.  The GOPs are cut into batches by plan_batches; the batches of a round are encoded
    side by side, one host thread each (the library call releases the GIL).  collect(first_gop, encoder) is called after each batch's encode, before the batch is
    closed, in the order of the GOPs: the place to read pictures() / recon() of a configuration with measure / keep_recon."""
    import concurrent.futures as cf

    if free_bytes is None:
        import torch

        free_bytes = torch.cuda.mem_get_info()[0]
    out = [None] * ngops
    for batches in plan_batches(cfg, ngops, frames, free_bytes, max_batches, batch_gops=batch_gops):
        encs = [BatchEncoder(cfg, n, frames) for _, n in batches]
        try:
            for e, (first, n) in zip(encs, batches):
                feed(e, first, n)
            with cf.ThreadPoolExecutor(len(encs)) as ex:
                results = list(ex.map(lambda e: e.encode(), encs))
            for (first, n), streams in zip(batches, results):
                out[first:first + n] = streams
            if collect is not None:
                for e, (first, _) in zip(encs, batches):
                    collect(first, e)
        finally:
            for e in encs:
                e.close()
    return out


def encode_video_rgb(video, cfg, frames, layout="hwc", max_batches=3, **color_kw):
    """an RGB video tensor -- (T, H, W, 3) for "hwc", (T, 3, H, W) for "chw", T a multiple of `frames` -- as T / frames closed GOPs over encode_gops; returns the joined
    bitstream (bytes): what the reference writes for the converted sequence with --closed-gop -I frames.  color_kw: color()'s keywords (the stream does not carry them)"""
    t = int(video.shape[0])
    if t < frames or t % frames:
        raise ValueError("the video's %d pictures are no multiple of %d" % (t, frames))

    def feed(enc, first, n):
        for g in range(n):
            enc.push_video_rgb(g, video[(first + g) * frames:(first + g + 1) * frames], layout, **color_kw)

    return b"".join(encode_gops(cfg, t // frames, frames, feed, max_batches=max_batches))


def encode_file(yuv_path, out_path, cfg, gops, frames, max_batches=3, recon_path=None, stats_path=None, hash=False, ssim=False):
    """the whole sequence: GOP g = frames [g * frames, (g + 1) * frames) of the file; the concatenated bitstreams are what the reference writes for the same sequence
    with --closed-gop -I frames.  Sequences beyond one batch are cut into batches that run side by side (encode_gops).  recon_path: the reconstructed
    sequence, GOP after GOP in display order -- the reference's -r file of the same run; stats_path: one line per picture as the application's table prints it (POC Tid
    Ftype QP PSNR-Y PSNR-U PSNR-V Bits), every GOP in coding order.  Either switches the configuration's measure / keep_recon on for this call.  hash: the
    application's --hash for this call (a configuration made with config(hash=True) has it already); the table's Bits stay what they are without it.  ssim: every
    picture's SSIM is measured in this call (config(ssim=True)) and each row of the table ends in three more columns, SSIM-Y SSIM-U SSIM-V ("%-10.6f"); without it the rows
    are byte for byte what they are."""
    if recon_path or stats_path or hash or ssim:
        c = _lib.EncConfig.from_buffer_copy(cfg)
        c.reserved[0] |= (8 if recon_path else 0) | (4 if stats_path else 0) | (16 if hash else 0) | (64 if ssim else 0)
        cfg = c
    fb = cfg.w * cfg.h * 3 // 2 * (2 if cfg.reserved[1] > 8 else 1)
    recon_file, stats_file = open(recon_path, "wb") if recon_path else None, open(stats_path, "w") if stats_path else None

    def collect(first, enc):  # (encode_gops calls it in the order of the GOPs)
        for g in range(enc.ngops):
            if recon_file:
                recon_file.write(enc.recon(g))
            if stats_file:
                for p in sorted(enc.pictures(g), key=lambda p: p["coding_pos"]):
                    stats_file.write(stats_line(p) + ("%-10.6f%-10.6f%-10.6f" % tuple(p["ssim"]) if ssim else "") + "\n")

    def feed(enc, first, n):
        with open(yuv_path, "rb") as f:
            f.seek(first * frames * fb)
            for g in range(n):
                for k in range(frames):
                    enc.push(g, k, f.read(fb))

    try:
        streams = encode_gops(cfg, gops, frames, feed, max_batches=max_batches, collect=collect if recon_file or stats_file else None)
    finally:
        for f in (recon_file, stats_file):
            if f:
                f.close()
    with open(out_path, "wb") as f:
        for s in streams:
            f.write(s)
    return streams
