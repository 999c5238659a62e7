"""Layer-level gfx950 kernels (include/fac_ops.h) on torch device tensors.

The §8f model families (ResVitKan, S3D) are sequences of ordinary layers:
their Python mirrors fold BatchNorm and pack weights once here, then call one
kernel per layer on the current torch stream (capturable into a hipGraph).
Activations are 16-bit channels-last tensors shaped ``[N, D, H, W, C]``
(``D = 1`` for 2-D nets), ``C`` a multiple of 8.  There is no CPU fallback:
every call goes through ``libfac_cvit.so`` and raises if it cannot.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import torch

from . import _lib

TORCH16 = {"bf16": torch.bfloat16, "fp16": torch.float16}

RELU, RESID, RELU2, OUT_F32, MAXPOOL3S2, MAXPOOL3S1, PREPOOL3S2 = 1, 2, 4, 8, 16, 32, 64   # FAC_CONV_* flags


class ConvDesc(ctypes.Structure):
    _fields_ = [("dtype", ctypes.c_int), ("inp", ctypes.c_void_p),
                ("n", ctypes.c_int), ("d", ctypes.c_int), ("h", ctypes.c_int), ("w", ctypes.c_int),
                ("cin", ctypes.c_int), ("weight", ctypes.c_void_p), ("bias", ctypes.c_void_p),
                ("cout", ctypes.c_int), ("k_pad", ctypes.c_int),
                ("kd", ctypes.c_int), ("kh", ctypes.c_int), ("kw", ctypes.c_int),
                ("sd", ctypes.c_int), ("sh", ctypes.c_int), ("sw", ctypes.c_int),
                ("pd", ctypes.c_int), ("ph", ctypes.c_int), ("pw", ctypes.c_int),
                ("od", ctypes.c_int), ("oh", ctypes.c_int), ("ow", ctypes.c_int),
                ("out", ctypes.c_void_p), ("ldo", ctypes.c_int), ("c_off", ctypes.c_int),
                ("residual", ctypes.c_void_p), ("ldr", ctypes.c_int), ("r_off", ctypes.c_int),
                ("flags", ctypes.c_int)]


class PoolDesc(ctypes.Structure):
    _fields_ = [("dtype", ctypes.c_int), ("inp", ctypes.c_void_p),
                ("n", ctypes.c_int), ("d", ctypes.c_int), ("h", ctypes.c_int), ("w", ctypes.c_int),
                ("c", ctypes.c_int),
                ("kd", ctypes.c_int), ("kh", ctypes.c_int), ("kw", ctypes.c_int),
                ("sd", ctypes.c_int), ("sh", ctypes.c_int), ("sw", ctypes.c_int),
                ("pd", ctypes.c_int), ("ph", ctypes.c_int), ("pw", ctypes.c_int),
                ("od", ctypes.c_int), ("oh", ctypes.c_int), ("ow", ctypes.c_int),
                ("mode", ctypes.c_int), ("out", ctypes.c_void_p), ("ldo", ctypes.c_int), ("c_off", ctypes.c_int)]


_ZERO256: dict = {}


def _zero256(device: torch.device) -> torch.Tensor:
    """256 zero bytes of device memory: the source of conv.hip's zero-padding loads."""
    key = (device.type, device.index)
    if key not in _ZERO256:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the zero page must be allocated before graph capture (construct the layers first)")
        _ZERO256[key] = torch.zeros(128, dtype=torch.int16, device=device)
    return _ZERO256[key]


def _stream(t: torch.Tensor):
    return torch.cuda.current_stream(t.device).cuda_stream


def _triple(v):
    if isinstance(v, int):
        return (v, v, v)
    v = tuple(v)
    return (1,) * (3 - len(v)) + v if len(v) < 3 else v


def _pads(v):
    if isinstance(v, int):
        return (v, v, v)
    v = tuple(v)
    return (0,) * (3 - len(v)) + v if len(v) < 3 else v


def fold_bn(weight: torch.Tensor, bias, gamma, beta, mean, var, eps: float):
    """Eval-mode BatchNorm folded into the preceding conv, in fp32 on the host:
    s = gamma / sqrt(var + eps), W' = W s, b' = (b - mean) s + beta."""
    w = weight.detach().to("cpu", torch.float32)
    co = w.shape[0]
    b = bias.detach().to("cpu", torch.float32) if bias is not None else torch.zeros(co)
    if gamma is None:
        return w, b
    s = gamma.detach().float().cpu() / torch.sqrt(var.detach().float().cpu() + eps)
    w = w * s.view(-1, *([1] * (w.dim() - 1)))
    b = (b - mean.detach().float().cpu()) * s + beta.detach().float().cpu()
    return w, b


@dataclass
class ConvGeom:
    kd: int
    kh: int
    kw: int
    sd: int
    sh: int
    sw: int
    pd: int
    ph: int
    pw: int


class ConvLayer:
    """A conv (+ folded BN) packed for fac_conv_nd: weights 16-bit
    [cout_pad][k_pad] with k = ((tz*kh + ty)*kw + tx)*cin_p + c."""

    def __init__(self, weight: torch.Tensor, bias: torch.Tensor, stride=1, padding=0, *, dtype: str, device,
                 cin_pad: int | None = None):
        w = weight.detach().to("cpu", torch.float32)
        if w.dim() == 4:                             # Conv2d: [co, ci, kh, kw] -> depth 1, no depth stride/pad
            w = w.unsqueeze(2)
            st = (1,) + ((stride, stride) if isinstance(stride, int) else tuple(stride))
            pd = (0,) + ((padding, padding) if isinstance(padding, int) else tuple(padding))
        else:
            st, pd = _triple(stride), _pads(padding)
        co, ci, kd, kh, kw = w.shape
        self.cout, self.cin = co, ci
        self.cin_p = cin_pad or (ci + 7) // 8 * 8
        self.g = ConvGeom(kd, kh, kw, *st, *pd)
        lib = _lib.load()
        cp, kp = ctypes.c_int(), ctypes.c_int()
        _lib.check(lib.fac_conv_weight_layout(co, self.cin_p, kd, kh, kw, ctypes.byref(cp), ctypes.byref(kp)), None,
                   "fac_conv_weight_layout")
        self.cout_pad, self.k_pad = cp.value, kp.value
        wp = torch.zeros(co, kd, kh, kw, self.cin_p)
        wp[..., :ci] = w.permute(0, 2, 3, 4, 1)
        packed = torch.zeros(self.cout_pad, self.k_pad)
        packed[:co, :kd * kh * kw * self.cin_p] = wp.reshape(co, -1)
        self.dtype = dtype
        self.w = packed.to(TORCH16[dtype]).to(device)
        b = torch.zeros(self.cout_pad)
        b[:co] = bias.detach().to("cpu", torch.float32)
        self.b = b.to(device)
        # 3x3 / stride 1 / padding 1 spatial convs with 32-channel chunks (the
        # ResNet-50 and S3D (1,3,3) layers) run on the CViT conv-stack kernel
        # (conv.hip: halo staged once per 32-channel chunk for all 9 taps)
        # wherever it has a tile for the resolution and width: packed per
        # input size on first use (fac_conv3x3_pack), else fac_conv_nd.
        self._w33 = None
        g = self.g
        if (kd, kh, kw) == (1, 3, 3) and (g.sd, g.sh, g.sw) == (1, 1, 1) and (g.pd, g.ph, g.pw) == (0, 1, 1) \
                and ci % 32 == 0:
            self._w33 = w[:, :, 0].reshape(co, ci, 9).contiguous()
            self._pk33 = {}
            self._device = device
            _zero256(torch.device(device))  # allocated (and zeroed) before any graph capture
            # conv.hip weights are packed on first use per input size (a
            # synchronous host->device copy: run one eager forward before
            # graph capture, which every caller here does), so a layer holds
            # only the packings of the sizes it sees

    def _packed33(self, h: int):
        """fac_conv3x3 weights for h x h inputs, or None if conv.hip has no tile for it."""
        if h not in self._pk33:
            if torch.cuda.is_current_stream_capturing():
                # packing copies host -> device synchronously: illegal inside a capture
                raise RuntimeError(f"conv weights for {h}x{h} inputs are packed on first use: run one eager "
                                   "forward (or the model's reserve()) at this input size before graph capture")
            lib = _lib.load()
            n = lib.fac_conv3x3_packed_elems(h, self.cin, self.cout)
            pk = None
            if n:
                out = torch.empty(n, dtype=torch.int16)
                _lib.check(lib.fac_conv3x3_pack(_lib.DTYPES[self.dtype], h, self.cin, self.cout, self._w33.data_ptr(),
                                                out.data_ptr()), None, "fac_conv3x3_pack")
                pk = out.view(TORCH16[self.dtype]).to(self._device)
            self._pk33[h] = pk
        return self._pk33[h]

    # maps the S3D drop-in fuses branch3's pool on: the kernel also takes 3 x 3,
    # where the chain of 13 dependent 64-channel chunks per unit measured
    # slower than the pool + conv launches (94 vs ~59 us at 1536 clips)
    MAXPOOL3S1_MAPS = (14, 7)

    def maxpool3s1_ok(self, x: torch.Tensor, out: torch.Tensor | None = None, c_off: int = 0) -> bool:
        """Whether fac_conv_nd takes FAC_CONV_MAXPOOL3S1 for this layer on x
        (ops.hip maxpool3_pw)."""
        g = self.g
        _, _, h, w, _ = x.shape
        return ((g.kd, g.kh, g.kw, g.sd, g.sh, g.sw, g.pd, g.ph, g.pw) == (1, 1, 1, 1, 1, 1, 0, 0, 0)
                and h == w and h in self.MAXPOOL3S1_MAPS and self.cout % 32 == 0 and c_off % 8 == 0
                and (out is None or out.shape[4] % 8 == 0) and _lib.exports("fac_conv_nd"))

    def prepool3s2_ok(self, x: torch.Tensor) -> bool:
        """Whether fac_conv_nd takes FAC_CONV_PREPOOL3S2 for this layer on x:
        MaxPool3d((1,3,3), (1,2,2), (0,1,1)) of x, then this 1x1x1 64 -> 64
        conv (S3D's base.1 + base.2 at 112^2 clips, ops.hip maxpool2s_pw)."""
        g = self.g
        return ((g.kd, g.kh, g.kw, g.sd, g.sh, g.sw, g.pd, g.ph, g.pw) == (1, 1, 1, 1, 1, 1, 0, 0, 0)
                and self.cin == 64 and self.cin_p == 64 and self.cout == 64 and x.shape[3] == 56
                and x.shape[4] == 64)

    def out_dims(self, d, h, w):
        g = self.g
        return ((d + 2 * g.pd - g.kd) // g.sd + 1, (h + 2 * g.ph - g.kh) // g.sh + 1,
                (w + 2 * g.pw - g.kw) // g.sw + 1)

    def __call__(self, x: torch.Tensor, *, relu: bool = True, out: torch.Tensor | None = None, c_off: int = 0,
                 residual: torch.Tensor | None = None, relu2: bool = False, out_f32: bool = False,
                 maxpool3s2: bool = False, maxpool3s1: bool = False, prepool3s2: bool = False) -> torch.Tensor:
        """maxpool3s2: MaxPool2d(3, 2, 1) over H, W fused into the launch
        (FAC_CONV_MAXPOOL3S2: the space-to-depth first conv with relu only;
        the output is the pooled [N, D, Ho/2, Wo/2, C]).  maxpool3s1:
        MaxPool3d(3, 1, 1) over the INPUT first (FAC_CONV_MAXPOOL3S1: a 1x1x1
        conv on a 14 / 7 / 3 square map, cout % 32 == 0; maxpool3s1_ok).
        prepool3s2: MaxPool3d((1,3,3), (1,2,2), (0,1,1)) over the INPUT
        first, the output at the pooled positions (FAC_CONV_PREPOOL3S2:
        prepool3s2_ok)."""
        n, d, h, w, _ = x.shape
        dsc = _desc(self, x, None, (RELU if relu else 0) | (RELU2 if relu2 else 0) | (OUT_F32 if out_f32 else 0) |
                    (MAXPOOL3S2 if maxpool3s2 else 0) | (MAXPOOL3S1 if maxpool3s1 else 0) |
                    (PREPOOL3S2 if prepool3s2 else 0))
        od, oh, ow = dsc.od, dsc.oh, dsc.ow
        if prepool3s2:
            if not self.prepool3s2_ok(x) or residual is not None or relu2 or out_f32 or maxpool3s2 or maxpool3s1:
                raise ValueError("prepool3s2 needs a 1x1x1 64 -> 64 conv on a 56-wide map, no residual / relu2 / "
                                 "fp32 output / other pool")
            oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        if maxpool3s2:
            if not relu or residual is not None or relu2 or out_f32 or c_off or oh % 2 or ow % 2:
                raise ValueError("maxpool3s2 needs relu, no residual / relu2 / fp32 output, even output dims")
            oh, ow = oh // 2, ow // 2
        if out is None:
            out = torch.empty(n, od, oh, ow, self.cout, device=x.device,
                              dtype=torch.float32 if out_f32 else x.dtype)
        if tuple(out.shape[:4]) != (n, od, oh, ow) or not out.is_contiguous():
            raise ValueError(f"conv output must be contiguous [{n},{od},{oh},{ow},C], got {tuple(out.shape)}")
        if maxpool3s1 and (not self.maxpool3s1_ok(x, out, c_off) or residual is not None or relu2 or out_f32):
            raise ValueError("maxpool3s1 needs a 1x1x1 conv over a 14 / 7 / 3 square map, cout % 32 == 0, "
                             "no residual / relu2 / fp32 output, ldo and c_off % 8 == 0")
        if (self._w33 is not None and h == w and residual is None and not relu2 and not out_f32 and c_off == 0
                and not maxpool3s2 and not maxpool3s1 and not prepool3s2 and out.shape[4] == self.cout and self.cin_p == self.cin):
            pk = self._packed33(h)
            if pk is not None:
                lib = _lib.load()
                _lib.check(lib.fac_conv3x3(_lib.DTYPES[self.dtype], x.data_ptr(), pk.data_ptr(), self.b.data_ptr(),
                                           out.data_ptr(), n * d, h, self.cin, self.cout, 0, 1 if relu else 0,
                                           _zero256(x.device).data_ptr(), _stream(x)), None, "fac_conv3x3")
                return out
        # what differs from the plain descriptor: the output found above (the
        # conv's own positions, before the fused pool, for maxpool3s2), the residual
        dsc.od, dsc.oh, dsc.ow = (od, 2 * oh, 2 * ow) if maxpool3s2 else (od, oh, ow)
        dsc.out, dsc.ldo, dsc.c_off = out.data_ptr(), out.shape[4], c_off
        if residual is not None:
            if tuple(residual.shape[:4]) != (n, od, oh, ow) or residual.dtype != x.dtype:
                raise ValueError("residual must match the output positions and dtype")
            dsc.residual, dsc.ldr, dsc.r_off = residual.data_ptr(), residual.shape[4], 0
            dsc.flags |= RESID
        _lib.check(_lib.load().fac_conv_nd(ctypes.byref(dsc), _stream(x)), None, "fac_conv_nd")
        return out


def _desc(layer: ConvLayer, x, out: torch.Tensor | None, flags: int, *, c_off: int = 0) -> "ConvDesc":
    """The one place that fills a fac_conv_desc: `layer` over `x`, into
    channels [c_off, c_off + cout) of `out` (None: no output of its own, or
    set by the caller).  `x` is the input tensor, checked here, or the
    (n, d, h, w) of an input the kernel makes itself (from a clip, or from
    the conv before it in a fused pair)."""
    if isinstance(x, torch.Tensor):
        n, d, h, w, c = x.shape
        if c != layer.cin_p or x.dtype != TORCH16[layer.dtype] or not x.is_contiguous():
            raise ValueError(f"conv input must be contiguous {layer.dtype} [N,D,H,W,{layer.cin_p}], got "
                             f"{x.dtype} {tuple(x.shape)}")
    else:
        n, d, h, w = x
    g = layer.g
    dsc = ConvDesc()
    dsc.dtype = _lib.DTYPES[layer.dtype]
    if isinstance(x, torch.Tensor):
        dsc.inp = x.data_ptr()
    dsc.n, dsc.d, dsc.h, dsc.w, dsc.cin = n, d, h, w, layer.cin_p
    dsc.weight, dsc.bias = layer.w.data_ptr(), layer.b.data_ptr()
    dsc.cout, dsc.k_pad = layer.cout, layer.k_pad
    dsc.kd, dsc.kh, dsc.kw, dsc.sd, dsc.sh, dsc.sw = g.kd, g.kh, g.kw, g.sd, g.sh, g.sw
    dsc.pd, dsc.ph, dsc.pw = g.pd, g.ph, g.pw
    dsc.od, dsc.oh, dsc.ow = layer.out_dims(d, h, w)
    if out is not None:
        dsc.out, dsc.ldo, dsc.c_off = out.data_ptr(), out.shape[4], c_off
    dsc.flags = flags
    return dsc


def conv_dual(layer: ConvLayer, h: torch.Tensor, ds: ConvLayer, x: torch.Tensor,
              out: torch.Tensor | None = None) -> torch.Tensor:
    """relu(relu(layer(h)) + ds(x)) in one fac_conv_nd_dual launch: a ResNet
    bottleneck's conv3 + bn3 + ReLU with its downsample branch (conv + bn,
    ResVitKan.py:146-152) added before the final ReLU, without the
    downsample output going through memory.  Same result as
    ``layer(h, residual=ds(x, relu=False), relu2=True)`` up to fp32 rounding
    (the downsample's sum is not rounded to 16 bits first)."""
    n, d, hh, w, _ = h.shape
    od, oh, ow = layer.out_dims(d, hh, w)
    if tuple(ds.out_dims(*x.shape[1:4])) != (od, oh, ow) or x.shape[0] != n or ds.cout != layer.cout:
        raise ValueError("conv_dual: the two convs must produce the same output positions and channels")
    if out is None:
        out = torch.empty(n, od, oh, ow, layer.cout, device=h.device, dtype=h.dtype)
    d1 = _desc(layer, h, out, RELU | RELU2)
    d2 = _desc(ds, x, None, 0)
    _lib.check(_lib.load().fac_conv_nd_dual(ctypes.byref(d1), ctypes.byref(d2), _stream(h)), None,
               "fac_conv_nd_dual")
    return out


def bottleneck_pw2(c3: ConvLayer, h: torch.Tensor, res: torch.Tensor, c1: ConvLayer):
    """(x, h1) = (relu(relu(c3(h)) + res), c1(x)) in one fac_bottleneck_pw2
    launch: a ResNet-50 layer1 bottleneck's conv3 (+ bn3, identity residual)
    and the next block's conv1 (+ bn1 + ReLU), the 256-channel block output
    written once and not read back (ResVitKan.py:146-152).  Same values as
    ``c3(h, residual=res, relu2=True)`` then ``c1(x)`` up to fp32 summation
    order."""
    n, d, hh, w, _ = h.shape
    x = torch.empty(n, d, hh, w, c3.cout, device=h.device, dtype=h.dtype)
    h1 = torch.empty(n, d, hh, w, c1.cout, device=h.device, dtype=h.dtype)
    if tuple(res.shape) != tuple(x.shape) or res.dtype != h.dtype or not res.is_contiguous():
        raise ValueError("bottleneck_pw2: residual must be the block input [N,D,H,W,256]")
    d3 = _desc(c3, h, x, RELU | RESID | RELU2)
    d3.residual, d3.ldr, d3.r_off = res.data_ptr(), res.shape[4], 0
    d1 = _desc(c1, x, h1, RELU)
    _lib.check(_lib.load().fac_bottleneck_pw2(ctypes.byref(d3), ctypes.byref(d1), _stream(h)), None,
               "fac_bottleneck_pw2")
    return x, h1


def conv_split(layer: ConvLayer, x: torch.Tensor, splits, out0: torch.Tensor, c_off0: int, out1: torch.Tensor,
               out2: torch.Tensor, relu: bool = True) -> None:
    """One fac_conv_nd_split launch of `layer` (a conv over concatenated
    output channels): columns [0, s1) -> out0[..., c_off0:], [s1, s2) -> out1,
    [s2, cout) -> out2 (each [N,D,H,W,C] contiguous)."""
    s1, s2 = splits
    dsc = _desc(layer, x, out0, RELU if relu else 0, c_off=c_off0)
    for t, width in ((out1, s2 - s1), (out2, layer.cout - s2)):
        if tuple(t.shape[:4]) != (dsc.n, dsc.od, dsc.oh, dsc.ow) or t.shape[4] < width or not t.is_contiguous():
            raise ValueError("conv_split outputs must be contiguous [N,D,H,W,C] tensors wide enough")
    _lib.check(_lib.load().fac_conv_nd_split(ctypes.byref(dsc), out1.data_ptr(), out1.shape[4], s1, out2.data_ptr(),
                                             out2.shape[4], s2, _stream(x)), None, "fac_conv_nd_split")


def _pool_desc(x: torch.Tensor, kernel, stride, padding, mode: str, out: torch.Tensor | None, c_off: int):
    """The one place that fills a fac_pool_desc: (desc, out), `out` allocated when None."""
    n, d, h, w, c = x.shape
    (kd, kh, kw), (sd, sh, sw), (pd, ph, pw) = _triple(kernel), _triple(stride), _pads(padding)
    od, oh, ow = (d + 2 * pd - kd) // sd + 1, (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1
    if out is None:
        out = torch.empty(n, od, oh, ow, c, device=x.device, dtype=x.dtype)
    dsc = PoolDesc()
    dsc.dtype = 0 if x.dtype == torch.bfloat16 else 1
    dsc.inp = x.data_ptr()
    dsc.n, dsc.d, dsc.h, dsc.w, dsc.c = n, d, h, w, c
    dsc.kd, dsc.kh, dsc.kw, dsc.sd, dsc.sh, dsc.sw, dsc.pd, dsc.ph, dsc.pw = kd, kh, kw, sd, sh, sw, pd, ph, pw
    dsc.od, dsc.oh, dsc.ow = od, oh, ow
    dsc.mode = {"max": 0, "avg": 1}[mode]
    dsc.out, dsc.ldo, dsc.c_off = out.data_ptr(), out.shape[4], c_off
    return dsc, out


def pool(x: torch.Tensor, kernel, stride, padding=0, mode: str = "max", out: torch.Tensor | None = None,
         c_off: int = 0) -> torch.Tensor:
    dsc, out = _pool_desc(x, kernel, stride, padding, mode, out, c_off)
    _lib.check(_lib.load().fac_pool_nd(ctypes.byref(dsc), _stream(x)), None, "fac_pool_nd")
    return out


def pool_route(x: torch.Tensor, kernel, stride, padding=0, mode: str = "max", out: torch.Tensor | None = None,
               c_off: int = 0) -> str:
    """The kernel family ``pool`` would launch for these arguments (fac_pool_nd_route: "pool_nd",
    "pool_max_win", "maxpool3_s1", ...); launches nothing, raises where ``pool`` would be refused."""
    dsc, _ = _pool_desc(x, kernel, stride, padding, mode, out, c_off)
    st = ctypes.c_int(0)
    name = _lib.load().fac_pool_nd_route(ctypes.byref(dsc), ctypes.byref(st))
    if not name:
        _lib.check(st.value, None, "fac_pool_nd_route")
    return name.decode()


def max_pool_sep(x: torch.Tensor, kernel, stride, padding=0) -> torch.Tensor:
    """Max pooling.  MaxPool3d(3, 1, 1) and strided windows are one
    fac_pool_nd call (a sliding-window kernel / a direct pass: for S3D's
    (1,3,3)/(1,2,2), (3,3,3)/2, (2,2,2)/2 and ResNet's 3x3/2 one direct pass
    over the 4-8x smaller output beat the separable passes, same-box S3D
    29.4k -> 30.35k clips/s); other stride-1 windows are one fac_pool_nd pass
    per axis (W, then H, then D; axes with kernel 1, stride 1 and no padding
    are skipped).  A max over a box window (padding ignored, i.e. -inf) is
    the max over its rows of the max over its columns, so every form is
    bit-identical to one 3-D pass."""
    k, s, p = _triple(kernel), _triple(stride), _pads(padding)
    if (k == (3, 3, 3) and s == (1, 1, 1) and p == (1, 1, 1)) or s != (1, 1, 1):
        return pool(x, kernel, stride, padding, "max")
    y = x
    for ax in (2, 1, 0):
        if k[ax] == 1 and s[ax] == 1 and p[ax] == 0:
            continue
        kk, ss, pp = [1, 1, 1], [1, 1, 1], [0, 0, 0]
        kk[ax], ss[ax], pp[ax] = k[ax], s[ax], p[ax]
        y = pool(y, tuple(kk), tuple(ss), tuple(pp), "max")
    return y if y is not x else pool(x, kernel, stride, padding, "max")


def _pack_out(out: torch.Tensor | None, shape, device, dtype: str) -> torch.Tensor:
    """The packers' output: a new tensor, or the caller's if it is exactly what a new one would be."""
    if out is None:
        return torch.empty(*shape, device=device, dtype=TORCH16[dtype])
    if tuple(out.shape) != tuple(shape) or out.dtype != TORCH16[dtype] or out.device != device or \
            not out.is_contiguous() or out.data_ptr() % 16:
        raise ValueError(f"out must be a contiguous 16-byte aligned {dtype} tensor {tuple(shape)} on {device}")
    return out


def pack_input(src: torch.Tensor, *, dtype: str, u8: bool, div: float = 1.0, mean=None, std=None,
               spatial: tuple[int, ...], c_pad: int = 8, out: torch.Tensor | None = None) -> torch.Tensor:
    """3-channel images -> 16-bit [N, D, H, W, c_pad] (fac_pack_input), zeros
    beyond channel 3; c_pad a multiple of 8.  u8: src uint8 [N, *spatial, 3];
    else fp32 planar [N, 3, *spatial].  out: a contiguous tensor of that shape
    and type to write instead of a new one."""
    n = src.shape[0]
    s = 1
    for v in spatial:
        s *= v
    d, h, w = (1,) * (3 - len(spatial)) + tuple(spatial)
    out = _pack_out(out, (n, d, h, w, c_pad), src.device, dtype)
    m = (ctypes.c_float * 3)(*(mean if mean is not None else (0.0, 0.0, 0.0)))
    sd = (ctypes.c_float * 3)(*(std if std is not None else (1.0, 1.0, 1.0)))
    src = src.contiguous()
    _lib.check(_lib.load().fac_pack_input(_lib.DTYPES[dtype], src.data_ptr(), 0 if u8 else 1, n, s, float(div),
                                          ctypes.cast(m, ctypes.c_void_p), ctypes.cast(sd, ctypes.c_void_p),
                                          out.data_ptr(), c_pad, _stream(src)), None, "fac_pack_input")
    return out


def pack_input_s2d(src: torch.Tensor, *, dtype: str, u8: bool, div: float = 1.0, mean=None, std=None,
                   pad_before: int = 2, pad_after: int = 1, out: torch.Tensor | None = None) -> torch.Tensor:
    """3-channel images -> 16-bit space-to-depth cells [N, T, h/2+pb+pa, w/2+pb+pa, 16]
    (fac_pack_input_s2d).  u8: src uint8 [N, h, w, 3] (T = 1); else fp32
    [N, 3, h, w] (T = 1) or a clip batch [N, 3, T, h, w].  out: as in pack_input."""
    n = src.shape[0]
    frames = src.shape[2] if (not u8 and src.dim() == 5) else 1
    h, w = (src.shape[1], src.shape[2]) if u8 else (src.shape[-2], src.shape[-1])
    ho, wo = h // 2 + pad_before + pad_after, w // 2 + pad_before + pad_after
    out = _pack_out(out, (n, frames, ho, wo, 16), src.device, dtype)
    m = (ctypes.c_float * 3)(*(mean if mean is not None else (0.0, 0.0, 0.0)))
    sd = (ctypes.c_float * 3)(*(std if std is not None else (1.0, 1.0, 1.0)))
    src = src.contiguous()
    _lib.check(_lib.load().fac_pack_input_s2d(_lib.DTYPES[dtype], src.data_ptr(), 0 if u8 else 1, n, frames, h, w,
                                              pad_before, pad_after, float(div), ctypes.cast(m, ctypes.c_void_p),
                                              ctypes.cast(sd, ctypes.c_void_p), out.data_ptr(), _stream(src)),
               None, "fac_pack_input_s2d")
    return out


def conv_s2d4_clip(layer: ConvLayer, clip: torch.Tensor, *, pad_before: int = 2, pad_after: int = 1,
                   relu: bool = True) -> torch.Tensor:
    """``layer(pack_input_s2d(clip, u8=False, pad_before, pad_after))`` in one
    launch (fac_conv_s2d4_clip): S3D's base.0 spatial (1,7,7)/(1,2,2) conv
    (model.py:18) with the space-to-depth packing folded into the conv's halo
    staging, so the 16-bit cell image never goes through HBM.  ``clip`` is the
    fp32 batch [N, 3, T, h, w], or uint8 (fac_conv_s2d4_clip_u8: decoded
    frames, a quarter of the bytes, the output of the same clip cast to fp32);
    ``layer`` the s2d-weight 4x4 conv.  Bit-identical to the two launches."""
    if clip.dtype not in (torch.float32, torch.uint8) or clip.dim() != 5 or clip.shape[1] != 3 or \
            not clip.is_contiguous():
        raise ValueError(f"expected a contiguous fp32 / uint8 clip [N,3,T,H,W], got {clip.dtype} {tuple(clip.shape)}")
    n, _, t, h, w = clip.shape
    hc, wc = h // 2 + pad_before + pad_after, w // 2 + pad_before + pad_after
    out = torch.empty(n, *layer.out_dims(t, hc, wc), layer.cout, device=clip.device, dtype=TORCH16[layer.dtype])
    dsc = _desc(layer, (n, t, hc, wc), out, RELU if relu else 0)   # the cells the kernel makes of the clip
    fn = "fac_conv_s2d4_clip_u8" if clip.dtype == torch.uint8 else "fac_conv_s2d4_clip"
    _lib.check(getattr(_lib.load(), fn)(ctypes.byref(dsc), clip.data_ptr(), h, w, pad_before, _stream(clip)), None, fn)
    return out


def sep_mid_ok(spatial: ConvLayer, temporal: ConvLayer, x: torch.Tensor) -> bool:
    """Whether fac_sep_mid takes this SepConv3d on x: Mixed_3c's branch2
    (1,3,3) 32 -> 96 (output rows zero-padded to 128) then (3,1,1) 128 -> 96
    over [N, 8, 14, 14, 32]."""
    gs, gt = spatial.g, temporal.g
    return (x.dim() == 5 and tuple(x.shape[1:]) == (8, 14, 14, 32) and spatial.cin_p == 32 and spatial.cout == 128
            and (gs.kd, gs.kh, gs.kw, gs.sd, gs.sh, gs.sw, gs.pd, gs.ph, gs.pw) == (1, 3, 3, 1, 1, 1, 0, 1, 1)
            and temporal.cin_p == 128 and temporal.cout == 96
            and (gt.kd, gt.kh, gt.kw, gt.sd, gt.sh, gt.sw, gt.pd, gt.ph, gt.pw) == (3, 1, 1, 1, 1, 1, 1, 0, 0)
            and _lib.exports("fac_sep_mid"))


def sep_tiny_ok(spatial: ConvLayer, temporal: ConvLayer, x: torch.Tensor) -> bool:
    """Whether fac_sep_tiny takes this SepConv3d on x: Mixed_3b's branch2
    (1,3,3) 16 -> 32 then (3,1,1) 32 -> 32 over [N, 8, 14, 14, 16]."""
    gs, gt = spatial.g, temporal.g
    return (x.dim() == 5 and tuple(x.shape[1:]) == (8, 14, 14, 16) and spatial.cin_p == 16 and spatial.cout == 32
            and (gs.kd, gs.kh, gs.kw, gs.sd, gs.sh, gs.sw, gs.pd, gs.ph, gs.pw) == (1, 3, 3, 1, 1, 1, 0, 1, 1)
            and temporal.cin_p == 32 and temporal.cout == 32
            and (gt.kd, gt.kh, gt.kw, gt.sd, gt.sh, gt.sw, gt.pd, gt.ph, gt.pw) == (3, 1, 1, 1, 1, 1, 1, 0, 0)
            and _lib.exports("fac_sep_tiny"))


def sep_tiny(spatial: ConvLayer, temporal: ConvLayer, x: torch.Tensor, out: torch.Tensor, c_off: int = 0) -> torch.Tensor:
    """``temporal(spatial(x))`` with both ReLUs in one launch, written into
    channels [c_off, c_off + cout) of `out` [N, 8, 14, 14, C]: fac_sep_tiny
    (Mixed_3b's branch2 SepConv, the 32-channel map kept in LDS) or, for
    Mixed_3c's 32 -> 96 -> 96 one, fac_sep_mid (2-row bands, the 96-channel
    map in LDS)."""
    mid = sep_mid_ok(spatial, temporal, x)
    if not (mid or sep_tiny_ok(spatial, temporal, x)) or x.dtype != TORCH16[spatial.dtype] or not x.is_contiguous():
        raise ValueError(f"sep_tiny needs Mixed_3b's / 3c's branch2 SepConv over [N,8,14,14,16|32], got "
                         f"{tuple(x.shape)}")
    if tuple(out.shape[:4]) != tuple(x.shape[:4]) or not out.is_contiguous():
        raise ValueError("out must be contiguous [N,8,14,14,C]")
    sd = _desc(spatial, x, None, RELU)
    td = _desc(temporal, (x.shape[0], 8, 14, 14), out, RELU, c_off=c_off)   # over the spatial half's map in LDS
    fn = "fac_sep_mid" if mid else "fac_sep_tiny"
    _lib.check(getattr(_lib.load(), fn)(ctypes.byref(sd), ctypes.byref(td), _stream(x)), None, fn)
    return out


def s3d_base0_u8(spatial: ConvLayer, temporal: ConvLayer, clip: torch.Tensor, *, pad_before: int = 2,
                 pad_after: int = 1) -> torch.Tensor:
    """S3D's base.0 in one launch (fac_s3d_base0_u8): ``temporal(
    conv_s2d4_clip(spatial, clip))`` for a uint8 clip batch [N, 3, 16, 112,
    112], both halves + ReLU, without the 16-frame half-resolution map going
    through HBM; bit-identical to the two launches.  -> [N, 8, 56, 56, 64]."""
    if clip.dtype != torch.uint8 or clip.dim() != 5 or clip.shape[1] != 3 or not clip.is_contiguous():
        raise ValueError(f"expected a contiguous uint8 clip [N,3,16,H,W], got {clip.dtype} {tuple(clip.shape)}")
    n, _, t, h, w = clip.shape
    hc, wc = h // 2 + pad_before + pad_after, w // 2 + pad_before + pad_after
    sd = _desc(spatial, (n, t, hc, wc), None, RELU)   # the clip's cells in, its map (dense, kept in LDS) out
    sd.ldo = spatial.cout
    mid = (n, sd.od, sd.oh, sd.ow)
    out = torch.empty(n, *temporal.out_dims(*mid[1:]), temporal.cout, device=clip.device,
                      dtype=TORCH16[temporal.dtype])
    td = _desc(temporal, mid, out, RELU)
    _lib.check(_lib.load().fac_s3d_base0_u8(ctypes.byref(sd), ctypes.byref(td), clip.data_ptr(), h, w, pad_before,
                                            _stream(clip)), None, "fac_s3d_base0_u8")
    return out


def s2d_weight(w: torch.Tensor) -> torch.Tensor:
    """[co, 3, 7, 7] stride-2 pad-3 kernel -> [co, 16, 4, 4] stride-1 kernel over
    fac_pack_input_s2d cells: w'[o][(dy*2+dx)*4 + c][ty][tx] = w[o][c][2ty+dy-1][2tx+dx-1].
    A (1, 7, 7) Conv3d kernel maps to (1, 4, 4) the same way."""
    if w.dim() == 5:
        if w.shape[2] != 1:
            raise ValueError("space-to-depth packing is for spatial-only (1, k, k) kernels")
        return s2d_weight(w[:, :, 0]).unsqueeze(2)
    co, ci, kh, kw = w.shape
    if ci != 3 or kh != 7 or kw != 7:
        raise ValueError("space-to-depth packing is for the 3-channel 7x7/2 first conv")
    out = torch.zeros(co, 16, 4, 4, dtype=w.dtype)
    for ty in range(4):
        for dy in range(2):
            ky = 2 * ty + dy - 1
            if not 0 <= ky < 7:
                continue
            for tx in range(4):
                for dx in range(2):
                    kx = 2 * tx + dx - 1
                    if 0 <= kx < 7:
                        out[:, (dy * 2 + dx) * 4:(dy * 2 + dx) * 4 + 3, ty, tx] = w[:, :, ky, kx]
    return out


class KANLinearLayer:
    """KANLinear (CViT-main/ResVitKan/kan.py:18-206) packed for fac_kan_linear:
    wcat[i][0][o] = base_weight[o][i], wcat[i][1+k][o] = spline_weight[o][i][k] * spline_scaler[o][i]."""

    N_KNOTS = 12

    def __init__(self, grid, base_weight, spline_weight, spline_scaler, device):
        g = grid.detach().to("cpu", torch.float32)
        bw = base_weight.detach().to("cpu", torch.float32)
        sw = spline_weight.detach().to("cpu", torch.float32)
        ss = spline_scaler.detach().to("cpu", torch.float32)
        self.out_f, self.in_f = bw.shape
        if g.shape != (self.in_f, self.N_KNOTS) or sw.shape != (self.out_f, self.in_f, self.N_KNOTS - 4):
            raise ValueError("KANLinear with grid_size 5 and spline_order 3 expected")
        scaled = sw * ss.unsqueeze(-1)                    # scaled_spline_weight (kan.py:176-183)
        # k-major [in][1 + nb][out] (fac_kan_linear)
        self.wcat = torch.cat([bw.unsqueeze(-1), scaled], dim=2).permute(1, 2, 0).contiguous().to(device)
        self.grid = g.contiguous().to(device)
        self._scratch = None

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        rows = x.shape[0]
        lib = _lib.load()
        nbytes = lib.fac_kan_scratch_bytes(rows, self.in_f, self.out_f)
        if self._scratch is None or self._scratch.numel() * 4 < nbytes or self._scratch.device != x.device:
            self._scratch = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device)
        y = torch.empty(rows, self.out_f, dtype=torch.float32, device=x.device)
        x = x.contiguous()
        _lib.check(lib.fac_kan_linear(x.data_ptr(), rows, self.in_f, self.out_f, self.grid.data_ptr(), self.N_KNOTS,
                                      self.wcat.data_ptr(), y.data_ptr(), self._scratch.data_ptr(), _stream(x)),
                   None, "fac_kan_linear")
        return y


class ContextAdd:
    """GCNet context block (ContextBlock3d, 'avg' pooling, 'channel_add') for
    fac_context_add: global mean over (T, H, W), Conv1x1x1(c -> p) +
    LayerNorm([p,1,1,1]) + ReLU6 + Conv1x1x1(p -> c), broadcast add.  Holds the
    six fp32 tensors on the device (w3 transposed to [p][c], fac_ops.h)."""

    ROUTES = {"auto": 0, "clip": 1, "split": 2}

    def __init__(self, w0, b0, ln_w, ln_b, w3, b3, *, eps: float = 1e-5, dtype: str, device):
        f = lambda t: t.detach().to("cpu", torch.float32)  # noqa: E731
        w0, w3 = f(w0), f(w3)
        self.p, self.c = int(w0.shape[0]), int(w0.shape[1])
        w0, w3 = w0.reshape(self.p, self.c), w3.reshape(self.c, self.p)
        if f(b0).numel() != self.p or f(ln_w).numel() != self.p or f(ln_b).numel() != self.p or f(b3).numel() != self.c:
            raise ValueError("ContextAdd: weight shapes do not describe Conv(c->p) + LayerNorm(p) + Conv(p->c)")
        self.dtype_name, self.eps = dtype, float(eps)
        self.w0 = w0.contiguous().to(device)
        self.b0 = f(b0).reshape(self.p).contiguous().to(device)
        self.ln_w = f(ln_w).reshape(self.p).contiguous().to(device)
        self.ln_b = f(ln_b).reshape(self.p).contiguous().to(device)
        self.w3t = w3.t().contiguous().to(device)
        self.b3 = f(b3).reshape(self.c).contiguous().to(device)

    def __call__(self, x: torch.Tensor, out: torch.Tensor | None = None, inplace: bool = False, route: int = 0,
                 return_term: bool = False):
        if x.dtype != TORCH16[self.dtype_name] or x.dim() < 3 or x.shape[-1] != self.c or not x.is_contiguous():
            raise ValueError(f"ContextAdd: expected a contiguous {self.dtype_name} [N, ..., {self.c}] tensor, "
                             f"got {x.dtype} {tuple(x.shape)}")
        if inplace:
            if out is not None and out.data_ptr() != x.data_ptr():
                raise ValueError("ContextAdd: inplace and out are exclusive")
            out = x
        elif out is None:
            out = torch.empty_like(x)
        if out.shape != x.shape or out.dtype != x.dtype or not out.is_contiguous() or out.device != x.device:
            raise ValueError("ContextAdd: out must match x in shape, dtype, device and be contiguous")
        if (x.data_ptr() | out.data_ptr()) % 16:
            raise ValueError("ContextAdd: x and out must be 16-byte aligned (the kernels load and store 16-byte vectors)")
        n, s = int(x.shape[0]), int(x.numel() // (x.shape[0] * self.c))
        lib = _lib.load()
        # scratch only where the split route runs (route 0 picks from (s, c): fac_context_route), and from
        # torch, like term: the caching allocator serves them under graph capture
        scratch = None
        if (int(route) or lib.fac_context_route(s, self.c)) == 2:
            scratch = torch.empty(max(lib.fac_context_scratch_bytes(n, s, self.c) // 4, 1), dtype=torch.float32,
                                  device=x.device)
        term = torch.empty(n, self.c, dtype=torch.float32, device=x.device) if return_term else None
        _lib.check(lib.fac_context_add(_lib.DTYPES[self.dtype_name], x.data_ptr(), n, s, self.c, self.p,
                                       self.w0.data_ptr(), self.b0.data_ptr(), self.ln_w.data_ptr(),
                                       self.ln_b.data_ptr(), self.eps, self.w3t.data_ptr(), self.b3.data_ptr(),
                                       out.data_ptr(), term.data_ptr() if return_term else None,
                                       scratch.data_ptr() if scratch is not None else None,
                                       int(route), _stream(x)), None, "fac_context_add")
        return (out, term) if return_term else out


# ---------------------------------------------------------------- msca.hip
class DWSepDesc(ctypes.Structure):
    _fields_ = [("dtype", ctypes.c_int), ("inp", ctypes.c_void_p), ("ldi", ctypes.c_int), ("i_off", ctypes.c_int),
                ("n", ctypes.c_int), ("t", ctypes.c_int), ("h", ctypes.c_int), ("w", ctypes.c_int), ("c", ctypes.c_int),
                ("kt", ctypes.c_int), ("k", ctypes.c_int), ("ws", ctypes.c_void_p), ("wt", ctypes.c_void_p),
                ("scale", ctypes.c_void_p), ("shift", ctypes.c_void_p), ("act", ctypes.c_int),
                ("scale2", ctypes.c_void_p), ("shift2", ctypes.c_void_p), ("out", ctypes.c_void_p),
                ("ldo", ctypes.c_int), ("o_off", ctypes.c_int), ("out_f32", ctypes.c_int)]


DWSEP_ACTS = {"none": 0, "affine2": 1, "gelu": 2}
EW_OPS = {"affine": 0, "gelu": 1, "mul": 2, "add": 3, "add_gelu": 4, "clamp6": 5, "add3": 6}


def bn_affine(gamma, beta, mean, var, eps: float):
    """Eval-mode BatchNorm as (scale, shift) fp32 on the host: scale = gamma / sqrt(var + eps)."""
    f = lambda t: t.detach().to("cpu", torch.float32)  # noqa: E731
    s = f(gamma) / torch.sqrt(f(var) + eps)
    return s, f(beta) - f(mean) * s


def _cl_slice(t: torch.Tensor, off: int, c: int, what: str, dtype=None):
    """Checks that channels [off, off + c) of the contiguous channels-last
    tensor t [..., ld] are a slice the msca.hip kernels take."""
    if t.dim() < 2 or not t.is_contiguous() or not t.is_cuda:
        raise ValueError(f"{what}: expected a contiguous channels-last GPU tensor, got {tuple(t.shape)}")
    if dtype is not None and t.dtype != dtype:
        raise ValueError(f"{what}: expected {dtype}, got {t.dtype}")
    ld = int(t.shape[-1])
    if c < 8 or c % 8 or ld % 8 or off % 8 or off < 0 or off + c > ld:
        raise ValueError(f"{what}: channels [{off}, {off + c}) of {ld} must be multiples of 8 inside the row")
    if t.data_ptr() % 16:
        raise ValueError(f"{what}: must be 16-byte aligned (the kernels load and store 16-byte vectors)")
    return ld


class DWSepLayer:
    """DWSepConv3d(c, (kt,k,k)) + its BatchNorm (given as scale / shift, see
    bn_affine) + ReLU6 for fac_dwsep3d, then `act`: 'none', 'affine2' (a second
    BatchNorm: scale2 / shift2) or 'gelu'.  w_s: conv_s.weight [c,1,1,k,k],
    w_t: conv_t.weight [c,1,kt,1,1]; k in {3,5,7}, kt in {1,3} (kt = 1 is a
    per-channel scale, folded into the spatial weights here)."""

    def __init__(self, w_s, w_t, scale, shift, *, act: str = "none", scale2=None, shift2=None, dtype: str, device):
        f = lambda t: t.detach().to("cpu", torch.float32)  # noqa: E731
        w_s, w_t = f(w_s), f(w_t)
        c = int(w_s.shape[0])
        if w_s.dim() != 5 or tuple(w_s.shape[1:3]) != (1, 1) or w_s.shape[3] != w_s.shape[4]:
            raise ValueError(f"DWSepLayer: conv_s.weight must be [c,1,1,k,k], got {tuple(w_s.shape)}")
        k, kt = int(w_s.shape[3]), int(w_t.shape[2]) if w_t.dim() == 5 else -1
        if tuple(w_t.shape) != (c, 1, kt, 1, 1):
            raise ValueError(f"DWSepLayer: conv_t.weight must be [{c},1,kt,1,1], got {tuple(w_t.shape)}")
        if k not in (3, 5, 7) or kt not in (1, 3):
            raise ValueError(f"DWSepLayer: k must be 3, 5 or 7 and kt 1 or 3, got k={k} kt={kt}")
        if c % 8:
            raise ValueError(f"DWSepLayer: channels must be a multiple of 8, got {c}")
        if act not in DWSEP_ACTS:
            raise ValueError(f"DWSepLayer: act must be one of {list(DWSEP_ACTS)}")
        if (act == "affine2") != (scale2 is not None and shift2 is not None):
            raise ValueError("DWSepLayer: scale2 and shift2 go with act='affine2', and only with it")
        if dtype not in _lib.DTYPES:
            raise ValueError(f"dtype must be one of {list(_lib.DTYPES)}")
        for v in (scale, shift, scale2, shift2):
            if v is not None and f(v).numel() != c:
                raise ValueError(f"DWSepLayer: per-channel tables must have {c} values")
        ws = w_s.reshape(c, k * k)
        if kt == 1:
            ws = ws * w_t.reshape(c, 1)
        self.c, self.k, self.kt, self.act, self.dtype = c, k, kt, act, dtype
        self.ws = ws.t().contiguous().to(device)                       # tap-major [k*k][c]
        self.wt = w_t.reshape(c, kt).t().contiguous().to(device) if kt == 3 else None
        self.scale, self.shift = f(scale).reshape(c).contiguous().to(device), f(shift).reshape(c).contiguous().to(device)
        self.scale2 = f(scale2).reshape(c).contiguous().to(device) if act == "affine2" else None
        self.shift2 = f(shift2).reshape(c).contiguous().to(device) if act == "affine2" else None

    def __call__(self, x: torch.Tensor, *, c_in_off: int = 0, out: torch.Tensor | None = None, c_off: int = 0,
                 out_f32: bool = False) -> torch.Tensor:
        if x.dim() != 5:
            raise ValueError(f"DWSepLayer: expected [N,T,H,W,C], got {tuple(x.shape)}")
        ldi = _cl_slice(x, c_in_off, self.c, "DWSepLayer input", TORCH16[self.dtype])
        n, t, h, w, _ = x.shape
        if out is None:
            out = torch.empty(n, t, h, w, self.c, device=x.device, dtype=torch.float32 if out_f32 else x.dtype)
        if tuple(out.shape[:4]) != (n, t, h, w):
            raise ValueError(f"DWSepLayer: out must be [{n},{t},{h},{w},C], got {tuple(out.shape)}")
        ldo = _cl_slice(out, c_off, self.c, "DWSepLayer output", torch.float32 if out_f32 else x.dtype)
        d = DWSepDesc()
        d.dtype = _lib.DTYPES[self.dtype]
        d.inp, d.ldi, d.i_off = x.data_ptr(), ldi, c_in_off
        d.n, d.t, d.h, d.w, d.c, d.kt, d.k = n, t, h, w, self.c, self.kt, self.k
        d.ws, d.wt = self.ws.data_ptr(), self.wt.data_ptr() if self.wt is not None else None
        d.scale, d.shift, d.act = self.scale.data_ptr(), self.shift.data_ptr(), DWSEP_ACTS[self.act]
        if self.act == "affine2":
            d.scale2, d.shift2 = self.scale2.data_ptr(), self.shift2.data_ptr()
        d.out, d.ldo, d.o_off, d.out_f32 = out.data_ptr(), ldo, c_off, int(out_f32)
        _lib.check(_lib.load().fac_dwsep3d(ctypes.byref(d), _stream(x)), None, "fac_dwsep3d")
        return out


def ew(op: str, a: torch.Tensor, b: torch.Tensor | None = None, c3: torch.Tensor | None = None, *, c: int | None = None,
       a_off: int = 0, b_off: int = 0, c3_off: int = 0, out: torch.Tensor | None = None, o_off: int = 0,
       scale: torch.Tensor | None = None, shift: torch.Tensor | None = None) -> torch.Tensor:
    """One fac_ew launch over channels-last 16-bit tensors: `op` of EW_OPS on
    channels [a_off, a_off + c) of a (and of b, c3 at their offsets), written
    to channels [o_off, o_off + c) of out (a new [..., c] tensor by default;
    out may be a).  'affine' takes fp32 device tables scale, shift [c]."""
    if op not in EW_OPS:
        raise ValueError(f"ew: op must be one of {list(EW_OPS)}")
    if a.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"ew: expected a 16-bit tensor, got {a.dtype}")
    c = int(a.shape[-1]) - a_off if c is None else c
    lda = _cl_slice(a, a_off, c, "ew a")
    rows = a.numel() // lda
    if out is None:
        out = torch.empty(*a.shape[:-1], c, device=a.device, dtype=a.dtype)
    ldo = _cl_slice(out, o_off, c, "ew out", a.dtype)
    if out.numel() // ldo != rows:
        raise ValueError("ew: out must have a's positions")
    ptr, ld, off = [None, None], [0, 0], (b_off, c3_off)
    need = {"mul": 1, "add": 1, "add_gelu": 1, "add3": 2}.get(op, 0)
    for i, t in enumerate((b, c3)):
        if (t is not None) != (i < need):
            raise ValueError(f"ew: '{op}' takes {need} operand(s) besides a")
        if t is not None:
            ld[i] = _cl_slice(t, off[i], c, "ew operand", a.dtype)
            if t.numel() // ld[i] != rows:
                raise ValueError("ew: every operand must have a's positions")
            ptr[i] = t.data_ptr()
    if op == "affine":
        for t in (scale, shift):
            if t is None or t.dtype != torch.float32 or t.numel() != c or not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"ew: 'affine' needs fp32 device tables scale, shift of {c} values")
    _lib.check(_lib.load().fac_ew(0 if a.dtype == torch.bfloat16 else 1, EW_OPS[op], a.data_ptr(), lda, a_off,
                                  ptr[0], ld[0], b_off, ptr[1], ld[1], c3_off,
                                  scale.data_ptr() if op == "affine" else None,
                                  shift.data_ptr() if op == "affine" else None, out.data_ptr(), ldo, o_off, rows, c,
                                  _stream(a)), None, "fac_ew")
    return out


def clamp6_(x: torch.Tensor, c_off: int = 0, c: int | None = None) -> torch.Tensor:
    """min(max(x, 0), 6) in place on channels [c_off, c_off + c) of x.  After a
    conv's own ReLU and 16-bit rounding this gives the bits of one ReLU6
    epilogue: 6 is a 16-bit value and the rounding is monotonic."""
    return ew("clamp6", x, a_off=c_off, c=c, out=x, o_off=c_off)


def msca_sum(a: torch.Tensor, dw5: DWSepLayer, dw7: DWSepLayer) -> torch.Tensor:
    """The MSCA sum (msca_3d.py:55-63): (a + DWSep5(a)) + DWSep7(a).  Two
    fac_dwsep3d launches and one fac_ew 'add3': each term is rounded to 16 bits
    where it is stored, then the sum once."""
    if dw5.k != 5 or dw7.k != 7 or dw5.c != dw7.c or dw5.act != "none" or dw7.act != "none":
        raise ValueError("msca_sum: expected the 5- and 7-window DWSepLayers of one width, act 'none'")
    return ew("add3", a, dw5(a), dw7(a))


def bn_max_pool(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, kt: int, *, c_in_off: int = 0,
                c: int | None = None, out: torch.Tensor | None = None, c_off: int = 0) -> torch.Tensor:
    """MaxPool3d((kt,3,3), 1, (kt//2,1,1)) of x * scale + shift on channels
    [c_in_off, c_in_off + c) of x [N,T,H,W,C] (fac_bn_maxpool3d): the iFormer
    block's BatchNorm + pool branch read straight from the block input."""
    if x.dim() != 5 or x.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"bn_max_pool: expected a 16-bit [N,T,H,W,C] tensor, got {x.dtype} {tuple(x.shape)}")
    if kt not in (1, 3):
        raise ValueError(f"bn_max_pool: kt must be 1 or 3, got {kt}")
    c = int(x.shape[-1]) - c_in_off if c is None else c
    ldi = _cl_slice(x, c_in_off, c, "bn_max_pool input")
    n, t, h, w, _ = x.shape
    if out is None:
        out = torch.empty(n, t, h, w, c, device=x.device, dtype=x.dtype)
    if tuple(out.shape[:4]) != (n, t, h, w):
        raise ValueError(f"bn_max_pool: out must be [{n},{t},{h},{w},C], got {tuple(out.shape)}")
    ldo = _cl_slice(out, c_off, c, "bn_max_pool output", x.dtype)
    for tb in (scale, shift):
        if tb.dtype != torch.float32 or tb.numel() != c or not tb.is_cuda or not tb.is_contiguous():
            raise ValueError(f"bn_max_pool: scale and shift must be fp32 device tables of {c} values")
    _lib.check(_lib.load().fac_bn_maxpool3d(0 if x.dtype == torch.bfloat16 else 1, x.data_ptr(), ldi, c_in_off, n, t,
                                            h, w, c, kt, scale.data_ptr(), shift.data_ptr(), out.data_ptr(), ldo,
                                            c_off, _stream(x)), None, "fac_bn_maxpool3d")
    return out


class Conv3x3Res:
    """A ResNet BasicBlock's second conv packed for fac_conv3x3_res (resnet.hip):
    Conv2d(3x3, stride 1, padding 1, c -> c) + folded BN, + residual, ReLU, on
    one of a ResNet-34's maps, (h, c) in SHAPES.  weight: the folded fp32
    [c, c, 3, 3]; bias fp32 [c]."""

    SHAPES = ((56, 64), (28, 128), (14, 256), (7, 512))

    def __init__(self, weight: torch.Tensor, bias: torch.Tensor, h: int, *, dtype: str, device):
        w = weight.detach().to("cpu", torch.float32).contiguous()
        c = int(w.shape[0])
        if tuple(w.shape) != (c, c, 3, 3):
            raise ValueError(f"Conv3x3Res: weight must be [c,c,3,3], got {tuple(w.shape)}")
        lib = _lib.load()
        n = lib.fac_conv3x3_res_packed_elems(h, c)
        if not n:
            raise ValueError(f"Conv3x3Res: no fac_conv3x3_res kernel for a {h}x{h}x{c} map (has {self.SHAPES})")
        pk = torch.empty(n, dtype=torch.int16)
        _lib.check(lib.fac_conv3x3_res_pack(_lib.DTYPES[dtype], h, c, w.data_ptr(), pk.data_ptr()), None,
                   "fac_conv3x3_res_pack")
        self.h, self.c, self.dtype = h, c, dtype
        self.w = pk.view(TORCH16[dtype]).to(device)
        self.b = bias.detach().to("cpu", torch.float32).contiguous().to(device)

    def __call__(self, x: torch.Tensor, residual: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        want = (self.h, self.h, self.c)
        for t, what in ((x, "input"), (residual, "residual")):
            if tuple(t.shape[-3:]) != want or t.dtype != TORCH16[self.dtype] or not t.is_contiguous() or \
                    t.shape != x.shape or not t.is_cuda:
                raise ValueError(f"Conv3x3Res: {what} must be a contiguous {self.dtype} GPU tensor [N,...,{self.h},"
                                 f"{self.h},{self.c}], got {t.dtype} {tuple(t.shape)}")
        if out is None:
            out = torch.empty_like(x)
        if out.shape != x.shape or out.dtype != x.dtype or not out.is_contiguous() or out.device != x.device:
            raise ValueError("Conv3x3Res: out must match the input in shape, dtype, device and be contiguous")
        n = x.numel() // (self.h * self.h * self.c)
        _lib.check(_lib.load().fac_conv3x3_res(_lib.DTYPES[self.dtype], x.data_ptr(), self.w.data_ptr(),
                                               self.b.data_ptr(), residual.data_ptr(), out.data_ptr(), n, self.h,
                                               self.c, _stream(x)), None, "fac_conv3x3_res")
        return out


def avgpool_f32(x: torch.Tensor) -> torch.Tensor:
    """Mean over every position of a 16-bit channels-last map [N, ..., C] ->
    fp32 [N, C] (fac_avgpool_f32): fp32 sums in a fixed order, the result never
    rounded to 16 bits."""
    if x.dtype not in (torch.float16, torch.bfloat16) or x.dim() < 2 or not x.is_contiguous() or not x.is_cuda:
        raise ValueError(f"avgpool_f32: expected a contiguous 16-bit GPU tensor [N,...,C], got {x.dtype} "
                         f"{tuple(x.shape)}")
    n, c = int(x.shape[0]), int(x.shape[-1])
    s = x.numel() // max(n * c, 1)
    y = torch.empty(n, c, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().fac_avgpool_f32(0 if x.dtype == torch.bfloat16 else 1, x.data_ptr(), n, s, c, y.data_ptr(),
                                           _stream(x)), None, "fac_avgpool_f32")
    return y


def sigmoid(x: torch.Tensor) -> torch.Tensor:
    y = torch.empty_like(x)
    _lib.check(_lib.load().fac_sigmoid(x.data_ptr(), y.data_ptr(), x.numel(), _stream(x)), None, "fac_sigmoid")
    return y
