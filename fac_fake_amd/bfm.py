"""Drop-in for ``CViT-main/model/other/cvit_GGCA4_BFM5.py`` on gfx950 HIP kernels,
and its BFM block as one fused kernel.

``cvit_GGCA4_BFM5`` is ``cvit_GGCA4`` (``x = GGCA(256,14,14)(x)`` between
``features1`` and ``features2``) plus ``x = BFM(512)(x, x)`` on the stem's
512x7x7 output; it keeps the CViT's channel / pool plan, patch, 2-token tail and
``pos_embedding`` rule, so it is ``variants.VariantCViT`` on its
``weights.BFM_VARIANTS`` entry.  This module holds the block's host fold,
packing and launch (the ``bfm`` step) and the factory by name.

The block.  ``BFM(t1, t2)`` runs both inputs through one
``MultiScaleFeatureExtractor`` (``MSFE(x) = ReLU(conv3x3(x)) + ReLU(conv5x5(x))
+ ReLU(conv7x7(x))``, three full C -> C convs) and fuses them with TFAM,
``(cs[0] + ss[0] + 1) a + (cs[1] + ss[1] + 1) b`` where ``cs`` and ``ss`` are
softmaxes over the stacking dimension of size 2.  Every reference call site is
``self.bfm(x, x)``: then ``a is b``, each softmax pair sums to 1, and the block
is ``4 MSFE(x)`` whatever the TFAM weights are.  Only that is built:
``bfm16`` is ``scale * sum_k ReLU(conv_k(x) + b_k)`` with ``scale = 4`` in one
``fac_bfm`` launch (bfm.hip).  The eight ``bfm.tfam.*`` tensors stay in the
``state_dict`` (loaded, kept, returned) and are never uploaded; a
``BFM(t1, t2)`` with two different inputs is not built because no reference
model has one.

``bfm16_composed`` is the same block from launches that existed before: three
``ops.ConvLayer`` (fac_conv_nd, ReLU in the epilogue), ``ops.ew("add3")`` and
the scale.  It rounds to 16 bits four times where ``bfm16`` rounds once; it is
the A/B baseline of tools/bench_bfm.py and the tests' second GPU witness.

The model's ``bfm`` step takes ``MODEL_ROUTE`` (``bfm_prepare``): the composed
route, which measured faster than ``fac_bfm`` at 256 crops (see there).

Grad-CAM is not implemented for the class.
"""
from __future__ import annotations

import torch

from . import _lib
from .ops import TORCH16
from .variants import VariantCViT, variant_class
from .weights import BFM_CONVS, BFM_NAMES, BFM_VARIANTS

BFM_SCALE = 4.0          # TFAM on two identical inputs (module docstring)


def bfm_fold(sd, prefix: str = "bfm"):
    """The BFM block (state_dict prefix) as fac_bfm_pack's operands, fp32 on the
    host: dict(w3 [c,c,3,3], w5 [c,c,5,5], w7 [c,c,7,7], bias3 [3,c] = the three
    convs' biases in that order).  The tfam.* tensors do not enter."""
    f = lambda k: sd[f"{prefix}.multi_scale_extractor.{k}"].detach().to("cpu", torch.float32).contiguous()  # noqa: E731
    ops = {f"w{k}": f(f"{name}.weight") for name, k in BFM_CONVS}
    ops["bias3"] = torch.stack([f(f"{name}.bias") for name, _k in BFM_CONVS]).contiguous()
    c = ops["bias3"].shape[1]
    for _name, k in BFM_CONVS:
        if tuple(ops[f"w{k}"].shape) != (c, c, k, k):
            raise ValueError(f"BFM conv {k}x{k}: expected [{c},{c},{k},{k}], got {tuple(ops[f'w{k}'].shape)}")
    return ops


def bfm_pack(ops: dict, dtype: str, device):
    """fac_bfm_pack of bfm_fold's operands -> (wpk, bias3) on the device, what bfm16 takes."""
    lib = _lib.load()
    c = ops["bias3"].shape[1]
    n = lib.fac_bfm_packed_elems(c)
    if n == 0:
        raise ValueError(f"BFM with {c} channels is not a fac_bfm shape")
    host = [ops[k].detach().to("cpu", torch.float32).contiguous() for k in ("w3", "w5", "w7")]
    out = torch.empty(n, dtype=torch.int16)
    _lib.check(lib.fac_bfm_pack(_lib.DTYPES[dtype], c, *[t.data_ptr() for t in host], out.data_ptr()), None,
               "fac_bfm_pack")
    return out.view(TORCH16[dtype]).to(device), ops["bias3"].detach().to(device=device, dtype=torch.float32).contiguous()


def bfm16(x: torch.Tensor, wpk: torch.Tensor, bias3: torch.Tensor, dtype: str, scale: float = BFM_SCALE):
    """BFM(x, x) on a [B,h,w,c] 16-bit NHWC device tensor (one fac_bfm call)."""
    B, h, w, c = x.shape
    out = torch.empty_like(x)
    _lib.check(_lib.load().fac_bfm(_lib.DTYPES[dtype], x.data_ptr(), B, h, w, c, wpk.data_ptr(), bias3.data_ptr(),
                                   float(scale), out.data_ptr(), torch.cuda.current_stream(x.device).cuda_stream),
               None, "fac_bfm")
    return out


class FusedBFM:
    """The block as one fac_bfm launch on operands packed once."""

    def __init__(self, ops: dict, dtype: str, device, scale: float = BFM_SCALE):
        self.wpk, self.bias3 = bfm_pack(ops, dtype, device)
        self.dtype, self.scale = dtype, float(scale)

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        return bfm16(x, self.wpk, self.bias3, self.dtype, self.scale)


class ComposedBFM:
    """The block from fac_conv_nd and fac_ew launches: three ops.ConvLayer with
    ReLU, ew("add3"), ew("affine") for the scale (skipped at scale 1)."""

    def __init__(self, ops: dict, dtype: str, device, scale: float = BFM_SCALE):
        from .ops import ConvLayer
        self.convs = [ConvLayer(ops[f"w{k}"], b, 1, k // 2, dtype=dtype, device=device)
                      for (_name, k), b in zip(BFM_CONVS, ops["bias3"])]
        c = ops["bias3"].shape[1]
        self.scale = None if scale == 1 else torch.full((c,), float(scale), dtype=torch.float32, device=device)
        self.shift = torch.zeros(c, dtype=torch.float32, device=device)

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        from .ops import ew
        B, h, w, c = x.shape
        x5 = x.view(B, 1, h, w, c)
        a, b, d = (conv(x5, relu=True) for conv in self.convs)
        y = ew("add3", a, b, d)
        if self.scale is not None:
            y = ew("affine", y, scale=self.scale, shift=self.shift, out=y)
        return y.view(B, h, w, c)


def bfm16_composed(x: torch.Tensor, ops: dict, dtype: str, scale: float = BFM_SCALE) -> torch.Tensor:
    """bfm16's result from the launches that existed before it (ComposedBFM,
    built per call: keep a ComposedBFM to time it)."""
    return ComposedBFM(ops, dtype, x.device, scale)(x)


# The route the model's bfm step takes.  The fused kernel is used only if it
# measured faster than the composed route at B = 256 in both dtypes; it did not
# (tools/bench_bfm.py, profiles/bfm_bench.txt, DESIGN 3.21: 1.70 ms against
# 1.04 ms on [256,7,7,512]; it is the faster one at B = 29, 0.70 against 1.02 ms,
# but a crop's bits must not depend on its batch, so the route does not either).
MODEL_ROUTE = "composed"
_ROUTES = {"fused": FusedBFM, "composed": ComposedBFM}


def bfm_prepare(ops: dict, dtype: str, device, scale: float = BFM_SCALE):
    """The model's bfm step: a callable x [B,h,w,c] -> BFM(x, x) on MODEL_ROUTE."""
    return _ROUTES[MODEL_ROUTE](ops, dtype, device, scale)


BfmCViT = VariantCViT        # the class has no body of its own


def bfm_class(name: str) -> type:
    """The drop-in class of reference file ``model/other/<name>.py`` (its ``CViT``)."""
    if name not in BFM_VARIANTS:
        raise KeyError(f"unknown BFM CViT {name!r}; known: {', '.join(BFM_NAMES)}")
    return variant_class(name)


def CViT(name: str, *args, **kwargs) -> VariantCViT:
    """``bfm_class(name)(*args, **kwargs)``: the reference's constructor arguments plus ``dtype``."""
    return bfm_class(name)(*args, **kwargs)


__all__ = ["BFM_NAMES", "BFM_SCALE", "BFM_VARIANTS", "BfmCViT", "CViT", "ComposedBFM", "FusedBFM", "MODEL_ROUTE", "bfm16",
           "bfm16_composed", "bfm_class", "bfm_fold", "bfm_pack", "bfm_prepare"]
