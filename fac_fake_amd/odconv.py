"""Drop-ins for ``CViT-main/model/other/cvit_GGCA_ADD_ODConv.py`` and
``cvit_GGCA_ODConv.py`` on gfx950 HIP kernels, and their ODConv2d block as one
``fac_odconv`` call.

``cvit_GGCA_ADD_ODConv`` is the (4, 1) plain CViT stem with four of its 3x3
convs replaced by ``ODConv2d(C, C, 3) -> BatchNorm2d -> ReLU`` (64x112x112,
128x56x56, 256x28x28 twice, the last followed by the max-pool), ``x +
GGCA(512, 7, 7)(x)`` on the stem output and a top-level ``odconv`` that is in
the ``state_dict`` and never called.  ``cvit_GGCA_ODConv`` is the plain stem with
a bare ``ODConv2d(256, 256, 3)`` (no BatchNorm, no ReLU: a signed map) on the
256x14x14 output of ``features1`` and ``x = GGCA(512, 7, 7)(x)``.  Both keep the
CViT's channel / pool plan, patch, 2-token tail and ``pos_embedding`` rule, so
each is ``variants.VariantCViT`` on its ``weights.ODCONV_VARIANTS`` entry.  This
module holds the block's host fold, packing and launch (the ``odconv`` step) and
the factory by name.

The block (odconv.hip has the formula): per crop, the channel means go through
a 16-wide bottleneck (1x1, BatchNorm, ReLU) to four heads, a sigmoid over the
input channels, one over the output channels, one over the nine taps and a
softmax over four candidate kernels; the conv's weight is the attention-weighted
sum of the four kernels, so it differs per crop.  The attention's BatchNorm and
the BatchNorm that follows the block are folded on the host in fp32
(``odconv_fold``).

Grad-CAM is not implemented for the classes.
"""
from __future__ import annotations

import torch

from . import _lib
from .variants import BN_EPS, VariantCViT, variant_class
from .weights import ODCONV_NAMES, ODCONV_VARIANTS

PACK_ORDER = ("weight", "fc", "bn_scale", "bn_shift", "channel_fc", "channel_b", "filter_fc", "filter_b", "spatial_fc",
              "spatial_b", "kernel_fc", "kernel_b", "scale", "shift")
KERNEL_NUM = 4
ATT_WIDTH = 16


def odconv_fold(sd, prefix: str, bn_prefix: str | None = None):
    """One ODConv2d block (state_dict prefix) and the BatchNorm after it as
    fac_odconv_pack's operands, fp32 on the host: dict(weight [4, c, c, 3, 3], fc
    [16, c], bn_scale, bn_shift [16] (the attention's BatchNorm), channel_fc [c,
    16], channel_b [c], filter_fc [c, 16], filter_b [c], spatial_fc [9, 16],
    spatial_b [9], kernel_fc [4, 16], kernel_b [4], scale, shift [c]).  bn_prefix
    None: scale 1, shift 0.  ValueError on a wrong shape or kernel_num != 4."""
    f = lambda k: sd[k].detach().to("cpu", torch.float32)  # noqa: E731
    p, a = prefix + ".", prefix + ".attention."
    w = f(p + "weight")
    if w.dim() != 5 or w.shape[0] != KERNEL_NUM:
        raise ValueError(f"ODConv {prefix}: expected a weight [4, c, c, 3, 3] (kernel_num 4), got {list(w.shape)}")
    c = w.shape[1]
    for q, n in ((a + "bn.", ATT_WIDTH),) + (((bn_prefix + ".", c),) if bn_prefix is not None else ()):
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            if tuple(sd[q + leaf].shape) != (n,):
                raise ValueError(f"ODConv {prefix} {q}{leaf}: expected [{n}], got {list(sd[q + leaf].shape)}")
    s = f(a + "bn.weight") / torch.sqrt(f(a + "bn.running_var") + BN_EPS)
    ops = dict(weight=w.contiguous(), fc=f(a + "fc.weight").flatten(1).contiguous(), bn_scale=s.contiguous(),
               bn_shift=(f(a + "bn.bias") - f(a + "bn.running_mean") * s).contiguous())
    for head in ("channel", "filter", "spatial", "kernel"):
        ops[head + "_fc"] = f(a + head + "_fc.weight").flatten(1).contiguous()
        ops[head + "_b"] = f(a + head + "_fc.bias").contiguous()
    if bn_prefix is None:
        ops["scale"], ops["shift"] = torch.ones(c), torch.zeros(c)
    else:
        q = bn_prefix + "."
        s = f(q + "weight") / torch.sqrt(f(q + "running_var") + BN_EPS)
        ops["scale"], ops["shift"] = s.contiguous(), (f(q + "bias") - f(q + "running_mean") * s).contiguous()
    h = ATT_WIDTH
    want = dict(weight=(KERNEL_NUM, c, c, 3, 3), fc=(h, c), bn_scale=(h,), bn_shift=(h,), channel_fc=(c, h), channel_b=(c,),
                filter_fc=(c, h), filter_b=(c,), spatial_fc=(9, h), spatial_b=(9,), kernel_fc=(KERNEL_NUM, h),
                kernel_b=(KERNEL_NUM,), scale=(c,), shift=(c,))
    for k, shape in want.items():
        if tuple(ops[k].shape) != shape:
            raise ValueError(f"ODConv {prefix} {k}: expected {list(shape)}, got {list(ops[k].shape)}")
    return ops


def odconv_pack(ops: dict, dtype: str, device) -> torch.Tensor:
    """fac_odconv_pack of odconv_fold's operands -> the device blob odconv16 takes."""
    lib = _lib.load()
    c = ops["weight"].shape[1]
    n = lib.fac_odconv_packed_bytes(c)
    if n == 0:
        raise ValueError(f"ODConv with {c} channels is not a fac_odconv shape")
    host = [ops[k].detach().to("cpu", torch.float32).contiguous() for k in PACK_ORDER]
    out = torch.empty(n, dtype=torch.uint8)
    _lib.check(lib.fac_odconv_pack(_lib.DTYPES[dtype], c, *[t.data_ptr() for t in host], out.data_ptr()), None,
               "fac_odconv_pack")
    return out.to(device)


def odconv16(x: torch.Tensor, packed: torch.Tensor, dtype: str, relu: bool = True, pool: bool = False,
             att_out: torch.Tensor | None = None, scratch: torch.Tensor | None = None) -> torch.Tensor:
    """act(ODConv(x) * scale + shift), act ReLU or (relu False) the identity, 2x2
    max-pooled with `pool`, on a [B,h,w,c] 16-bit NHWC device tensor (one
    fac_odconv call).  att_out: a contiguous fp32 [B, 2c + 13] device tensor that
    receives ca | fa | sa | ka.  scratch: at least fac_odconv_scratch_bytes(B, h,
    w, c) bytes on x's device; allocated per call when None."""
    B, h, w, c = x.shape
    lib = _lib.load()
    need = lib.fac_odconv_scratch_bytes(B, h, w, c)
    if need == 0 or (pool and (h % 2 or w % 2)):
        raise ValueError(f"[{B},{h},{w},{c}] (pool {bool(pool)}) is not a fac_odconv shape")
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=x.device)
    elif scratch.numel() * scratch.element_size() < need:
        raise ValueError(f"fac_odconv needs {need} scratch bytes, got {scratch.numel() * scratch.element_size()}")
    if att_out is not None and (att_out.dtype != torch.float32 or tuple(att_out.shape) != (B, 2 * c + 13) or
                                not att_out.is_contiguous() or att_out.device != x.device):
        raise ValueError(f"att_out must be a contiguous fp32 [{B},{2 * c + 13}] tensor on {x.device}")
    out = torch.empty((B, h // 2, w // 2, c) if pool else (B, h, w, c), dtype=x.dtype, device=x.device)
    _lib.check(lib.fac_odconv(_lib.DTYPES[dtype], x.data_ptr(), B, h, w, c, packed.data_ptr(), int(bool(relu)),
                              int(bool(pool)), out.data_ptr(), att_out.data_ptr() if att_out is not None else None,
                              scratch.data_ptr(), torch.cuda.current_stream(x.device).cuda_stream), None, "fac_odconv")
    return out


ODConvCViT = VariantCViT       # the classes have no body of their own


def odconv_class(name: str) -> type:
    """The drop-in class of reference file ``model/other/<name>.py`` (its ``CViT``)."""
    if name not in ODCONV_VARIANTS:
        raise KeyError(f"unknown ODConv CViT {name!r}; known: {', '.join(ODCONV_NAMES)}")
    return variant_class(name)


def CViT(name: str = "cvit_GGCA_ADD_ODConv", *args, **kwargs) -> VariantCViT:
    """``odconv_class(name)(*args, **kwargs)``: the reference's constructor arguments plus ``dtype``."""
    return odconv_class(name)(*args, **kwargs)


__all__ = ["ATT_WIDTH", "CViT", "KERNEL_NUM", "ODCONV_NAMES", "ODCONV_VARIANTS", "ODConvCViT", "PACK_ORDER", "odconv16",
           "odconv_class", "odconv_fold", "odconv_pack"]
