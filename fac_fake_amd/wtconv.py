"""Drop-in for ``CViT-main/model/other/cvit_GGCA_ADD_WTConv.py`` on gfx950 HIP
kernels, and its WTConv2d block as one ``fac_wtconv`` call.

The base CViT's one ``features`` Sequential with nine of its seventeen 3x3
convs replaced by ``WTConv2d(C) -> BatchNorm2d -> ReLU`` (:226-317 with
kernel_size 5, wt_levels 1, db1; two each on 32x224x224, 64x112x112 and
128x56x56, three on 256x28x28, the last of every block followed by the
max-pool), ``x + GGCA(512, 7, 7)(x)`` on the stem output and the base CViT's
tail.  The class is ``variants.VariantCViT`` on its ``weights.WTCONV_VARIANTS``
entry; its first block holds WTConv layers, so the stem starts with the
``pack32`` step instead of the fused ``fac_stem224``.  This module holds the
``wt`` step's host fold, packing and launch.

The block (wtconv.hip has the formula): the map goes through the 2x2 Haar
analysis filters to four half-resolution subbands, each through its own
depthwise 5x5 and scale, back through the synthesis filters, and is added to a
scaled depthwise 5x5 (with bias) of the map itself.  Both scales, the bias and
the BatchNorm that follows are folded on the host in fp32 (``wt_fold``); the
2x2 filters are taken from the ``state_dict``, where the reference keeps them
as frozen parameters.  One launch, no scratch.

Grad-CAM is not implemented for the class.
"""
from __future__ import annotations

import torch

from . import _lib
from .variants import BN_EPS, variant_class
from .weights import WTCONV_NAMES

NAME = WTCONV_NAMES[0]
PACK_ORDER = ("dwt", "wtaps", "iwt", "btaps", "scale", "shift")


def wt_fold(sd, p: str, q: str | None = None):
    """One WTConv2d (state_dict prefix p) and the BatchNorm after it (prefix q;
    None: scale 1, shift 0) as fac_wtconv's operands in their natural order,
    fp32 on the host: dict(dwt [c, 4, 2, 2] = wt_filter, wtaps [c, 4, 25] =
    wavelet_convs.0.weight * wavelet_scale.0.weight, iwt [c, 4, 2, 2] =
    iwt_filter, btaps [c, 25] = base_conv.weight * base_scale.weight, scale =
    gamma / sqrt(var + eps), shift = beta - mean * scale + base_scale * bias *
    scale).  ValueError on a wrong shape or more than one wavelet level."""
    f = lambda k: sd[k].detach().to("cpu", torch.float32)  # noqa: E731
    if any(k.startswith(p + ".wavelet_convs.") and not k.startswith(p + ".wavelet_convs.0.") for k in sd):
        raise ValueError(f"WTConv {p}: more than one wavelet level; only wt_levels=1 is implemented")
    base = f(p + ".base_conv.weight")
    c = base.shape[0]
    want = {"wt_filter": (4 * c, 1, 2, 2), "iwt_filter": (4 * c, 1, 2, 2), "base_conv.weight": (c, 1, 5, 5),
            "base_conv.bias": (c,), "base_scale.weight": (1, c, 1, 1), "wavelet_convs.0.weight": (4 * c, 1, 5, 5),
            "wavelet_scale.0.weight": (1, 4 * c, 1, 1)}
    for leaf, shape in want.items():
        if tuple(sd[f"{p}.{leaf}"].shape) != shape:
            raise ValueError(f"WTConv {p}.{leaf}: expected {list(shape)}, got {list(sd[f'{p}.{leaf}'].shape)}")
    bscale = f(p + ".base_scale.weight").reshape(c)
    ops = dict(dwt=f(p + ".wt_filter").reshape(c, 4, 2, 2).contiguous(),
               wtaps=(f(p + ".wavelet_convs.0.weight").reshape(4 * c, 25) *
                      f(p + ".wavelet_scale.0.weight").reshape(4 * c, 1)).reshape(c, 4, 25).contiguous(),
               iwt=f(p + ".iwt_filter").reshape(c, 4, 2, 2).contiguous(),
               btaps=(base.reshape(c, 25) * bscale.view(c, 1)).contiguous())
    if q is None:
        scale, shift = torch.ones(c), torch.zeros(c)
    else:
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            if tuple(sd[f"{q}.{leaf}"].shape) != (c,):
                raise ValueError(f"WTConv {p} {q}.{leaf}: expected [{c}], got {list(sd[f'{q}.{leaf}'].shape)}")
        scale = f(q + ".weight") / torch.sqrt(f(q + ".running_var") + BN_EPS)
        shift = f(q + ".bias") - f(q + ".running_mean") * scale
    ops["scale"] = scale.contiguous()
    ops["shift"] = (shift + bscale * f(p + ".base_conv.bias") * scale).contiguous()
    return ops


def wt_pack(ops: dict, device) -> tuple:
    """wt_fold's operands in fac_wtconv's memory order on `device`, in PACK_ORDER:
    the channel split as 4 * quad + e with e innermost (dwt, iwt [c/4, 4, 4, 4],
    wtaps [c/4, 4, 25, 4], btaps [c/4, 25, 4]); scale and shift as they are."""
    c = ops["scale"].shape[0]
    if c % 4:
        raise ValueError(f"WTConv with {c} channels is not a fac_wtconv shape")
    g = lambda t, *mid: t.detach().to("cpu", torch.float32).reshape(c // 4, 4, *mid)  # noqa: E731
    packed = dict(dwt=g(ops["dwt"], 4, 4).permute(0, 2, 3, 1), wtaps=g(ops["wtaps"], 4, 25).permute(0, 2, 3, 1),
                  iwt=g(ops["iwt"], 4, 4).permute(0, 2, 3, 1), btaps=g(ops["btaps"], 25).permute(0, 2, 1),
                  scale=ops["scale"].detach().float(), shift=ops["shift"].detach().float())
    return tuple(packed[k].contiguous().to(device) for k in PACK_ORDER)


def wtconv16(x: torch.Tensor, ops, dtype: str, pool: bool = False) -> torch.Tensor:
    """maxpool?(relu(scale * WTConv(x) + shift)) on a [B,h,w,c] 16-bit NHWC device
    tensor (one fac_wtconv call).  ops: wt_pack's tuple on x's device, or
    wt_fold's dict (packed per call)."""
    B, h, w, c = x.shape
    if isinstance(ops, dict):
        ops = wt_pack(ops, x.device)
    if c % 32 or not 32 <= c <= 256 or h % 2 or w % 2 or not 2 <= h <= 224 or not 2 <= w <= 224:
        raise ValueError(f"[{B},{h},{w},{c}] is not a fac_wtconv shape")
    out = torch.empty((B, h // 2, w // 2, c) if pool else (B, h, w, c), dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().fac_wtconv(_lib.DTYPES[dtype], x.data_ptr(), out.data_ptr(), B, h, w, c,
                                      *[t.data_ptr() for t in ops], int(bool(pool)),
                                      torch.cuda.current_stream(x.device).cuda_stream), None, "fac_wtconv")
    return out


CViT = variant_class(NAME)

__all__ = ["CViT", "NAME", "PACK_ORDER", "WTCONV_NAMES", "wt_fold", "wt_pack", "wtconv16"]
