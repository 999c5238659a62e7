"""Drop-in for ``CViT-main/model/other/cvit_GGCA_ADD_ScConv.py`` on gfx950 HIP
kernels, and its ScConv block as one ``fac_scconv`` call.

The class is the (4, 1) plain CViT stem with four of its 3x3 convs replaced by
``ScConv(C) -> BatchNorm2d -> ReLU`` (64x112x112, 128x56x56, 256x28x28 twice,
the last followed by the max-pool) and ``x + GGCA(512, 7, 7)(x)`` on the stem
output; it keeps the CViT's channel / pool plan, patch, 2-token tail and
``pos_embedding`` rule, so it is ``variants.VariantCViT`` on its
``weights.SCCONV_VARIANTS`` entry.  This module holds the block's host fold,
packing and launch (the ``scconv`` step) and the factory by name.

The block (scconv.hip has the derivation): GroupNorm(4, C) statistics per crop,
a hard gate that moves channels between the two halves, two 1x1 squeezes, a
grouped 3x3 + 1x1 on one half and a 1x1 + identity on the other, both rescaled
by a softmax over the 2C per-crop channel means, which are linear in the
squeezed map and so known before either is formed.  The BatchNorm that follows
is folded on the host in fp32 into the kernel's scale and shift
(``scconv_fold``), before the one rounding of the conv weights to 16 bits
(``fac_scconv_pack``).

Grad-CAM is not implemented for the class.
"""
from __future__ import annotations

import torch

from . import _lib
from .variants import BN_EPS, VariantCViT, variant_class
from .weights import SCCONV_NAMES, SCCONV_VARIANTS

PACK_ORDER = ("gamma", "beta", "kc", "squeeze1", "squeeze2", "gwc_w", "gwc_b", "pwc1", "pwc2", "scale", "shift")


def scconv_fold(sd, prefix: str, bn_prefix: str | None = None):
    """One ScConv block (state_dict prefix) and the BatchNorm after it as
    fac_scconv_pack's operands, fp32 on the host: dict(gamma, beta [c], kc [c] =
    gamma / sum(gamma), squeeze1, squeeze2 [c/4, c/2], gwc_w [c, c/8, 3, 3],
    gwc_b [c], pwc1 [c, c/4], pwc2 [3c/4, c/4], scale, shift [c]).  bn_prefix
    None: scale 1, shift 0.  ValueError where sum(gamma) is 0 or not finite:
    the block divides by it."""
    f = lambda k: sd[k].detach().to("cpu", torch.float32)  # noqa: E731
    p = prefix + "."
    g = f(p + "SRU.gn.weight")
    c = g.shape[0]
    tot = g.sum()
    if not bool(torch.isfinite(tot)) or float(tot) == 0.0:
        raise ValueError(f"ScConv {prefix}: sum(gn.weight) is {float(tot)}; the block divides by it")
    ops = dict(gamma=g.contiguous(), beta=f(p + "SRU.gn.bias").contiguous(), kc=(g / tot).contiguous(),
               squeeze1=f(p + "CRU.squeeze1.weight").reshape(c // 4, -1).contiguous(),
               squeeze2=f(p + "CRU.squeeze2.weight").reshape(c // 4, -1).contiguous(),
               gwc_w=f(p + "CRU.GWC.weight").contiguous(), gwc_b=f(p + "CRU.GWC.bias").contiguous(),
               pwc1=f(p + "CRU.PWC1.weight").reshape(c, -1).contiguous(),
               pwc2=f(p + "CRU.PWC2.weight").reshape(3 * c // 4, -1).contiguous())
    if bn_prefix is None:
        ops["scale"], ops["shift"] = torch.ones(c), torch.zeros(c)
    else:
        q = bn_prefix + "."
        s = f(q + "weight") / torch.sqrt(f(q + "running_var") + BN_EPS)
        ops["scale"], ops["shift"] = s.contiguous(), (f(q + "bias") - f(q + "running_mean") * s).contiguous()
    want = dict(gamma=(c,), beta=(c,), kc=(c,), squeeze1=(c // 4, c // 2), squeeze2=(c // 4, c // 2),
                gwc_w=(c, c // 8, 3, 3), gwc_b=(c,), pwc1=(c, c // 4), pwc2=(3 * c // 4, c // 4), scale=(c,), shift=(c,))
    for k, shape in want.items():
        if tuple(ops[k].shape) != shape:
            raise ValueError(f"ScConv {prefix} {k}: expected {list(shape)}, got {list(ops[k].shape)}")
    return ops


def scconv_pack(ops: dict, dtype: str, device) -> torch.Tensor:
    """fac_scconv_pack of scconv_fold's operands -> the device blob scconv16 takes."""
    lib = _lib.load()
    c = ops["gamma"].shape[0]
    n = lib.fac_scconv_packed_bytes(c)
    if n == 0:
        raise ValueError(f"ScConv with {c} channels is not a fac_scconv shape")
    host = [ops[k].detach().to("cpu", torch.float32).contiguous() for k in PACK_ORDER]
    out = torch.empty(n, dtype=torch.uint8)
    _lib.check(lib.fac_scconv_pack(_lib.DTYPES[dtype], c, *[t.data_ptr() for t in host], out.data_ptr()), None,
               "fac_scconv_pack")
    return out.to(device)


def scconv16(x: torch.Tensor, packed: torch.Tensor, dtype: str, pool: bool = False,
             stats_out: torch.Tensor | None = None, scratch: torch.Tensor | None = None) -> torch.Tensor:
    """ReLU(ScConv(x) * scale + shift), 2x2 max-pooled with `pool`, on a
    [B,h,w,c] 16-bit NHWC device tensor (one fac_scconv call, six launches).
    stats_out: a contiguous fp32 [B,4,2] device tensor that receives (mu_g,
    rstd_g).  scratch: at least fac_scconv_scratch_bytes(B, h, w, c) bytes on
    x's device; allocated per call when None."""
    B, h, w, c = x.shape
    lib = _lib.load()
    need = lib.fac_scconv_scratch_bytes(B, h, w, c)
    if need == 0 or (pool and (h % 2 or w % 2)):
        raise ValueError(f"[{B},{h},{w},{c}] (pool {bool(pool)}) is not a fac_scconv shape")
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=x.device)
    elif scratch.numel() * scratch.element_size() < need:
        raise ValueError(f"fac_scconv needs {need} scratch bytes, got {scratch.numel() * scratch.element_size()}")
    if stats_out is not None and (stats_out.dtype != torch.float32 or tuple(stats_out.shape) != (B, 4, 2) or
                                  not stats_out.is_contiguous() or stats_out.device != x.device):
        raise ValueError(f"stats_out must be a contiguous fp32 [{B},4,2] tensor on {x.device}")
    out = torch.empty((B, h // 2, w // 2, c) if pool else (B, h, w, c), dtype=x.dtype, device=x.device)
    _lib.check(lib.fac_scconv(_lib.DTYPES[dtype], x.data_ptr(), B, h, w, c, packed.data_ptr(), int(bool(pool)),
                              out.data_ptr(), stats_out.data_ptr() if stats_out is not None else None,
                              scratch.data_ptr(), torch.cuda.current_stream(x.device).cuda_stream), None, "fac_scconv")
    return out


ScConvCViT = VariantCViT       # the class has no body of its own


def scconv_class(name: str) -> type:
    """The drop-in class of reference file ``model/other/<name>.py`` (its ``CViT``)."""
    if name not in SCCONV_VARIANTS:
        raise KeyError(f"unknown ScConv CViT {name!r}; known: {', '.join(SCCONV_NAMES)}")
    return variant_class(name)


def CViT(name: str = "cvit_GGCA_ADD_ScConv", *args, **kwargs) -> VariantCViT:
    """``scconv_class(name)(*args, **kwargs)``: the reference's constructor arguments plus ``dtype``."""
    return scconv_class(name)(*args, **kwargs)


__all__ = ["CViT", "PACK_ORDER", "SCCONV_NAMES", "SCCONV_VARIANTS", "ScConvCViT", "scconv16", "scconv_class",
           "scconv_fold", "scconv_pack"]
