"""Drop-in for ``CViT-main/model/cvit_GGCA_ADD_DConv.py`` on gfx950 HIP kernels.

The base CViT with nine of its seventeen 3x3 convs replaced by
``InceptionDWConv2d`` (:157-177: 5/8 of the channels pass, 1/8 each go through
a depthwise 3x3, 1x11 and 11x1 conv), ``x + GGCA(x)`` on the 512x7x7 map and
the base CViT's tail (``nn.LayerNorm`` in both PreNorms).  The class is
``variants.VariantCViT`` on the ``weights.CVIT_FAMILY`` entry of that name; its
first block holds two InceptionDWConv2d layers, so the stem starts with the
``pack32`` step instead of the fused ``fac_stem224``.  This module holds the
host-side fold of the ``idw`` step: every ``InceptionDWConv2d -> BatchNorm2d ->
ReLU (-> MaxPool2d)`` is one ``fac_idwconv`` launch (idwconv.hip), the conv
biases and the BatchNorm folded into a per-channel fp32 scale and shift, the
taps left as they are.

Grad-CAM is not implemented for this class.
"""
from __future__ import annotations

import torch

from .variants import BN_EPS, variant_class
from .weights import DCONV_NAME as NAME


def idw_fold(sd, p: str, q: str):
    """One InceptionDWConv2d (state_dict prefix p) and its BatchNorm (prefix q)
    as fac_idwconv's operands, fp32 on the host: the taps [gc,9], [gc,11],
    [gc,11] as stored, scale = gamma / sqrt(var + eps) and shift = beta - mean *
    scale, plus bias * scale on the 3 gc conv channels."""
    f = lambda k: sd[k].detach().to("cpu", torch.float32)  # noqa: E731
    w_hw, w_w, w_h = f(p + ".dwconv_hw.weight"), f(p + ".dwconv_w.weight"), f(p + ".dwconv_h.weight")
    gc = w_hw.shape[0]
    scale = f(q + ".weight") / torch.sqrt(f(q + ".running_var") + BN_EPS)
    shift = f(q + ".bias") - f(q + ".running_mean") * scale
    bias = torch.cat([f(p + ".dwconv_hw.bias"), f(p + ".dwconv_w.bias"), f(p + ".dwconv_h.bias")])
    shift[-3 * gc:] += bias * scale[-3 * gc:]
    return w_hw.reshape(gc, 9).contiguous(), w_w.reshape(gc, 11).contiguous(), w_h.reshape(gc, 11).contiguous(), \
        scale.contiguous(), shift.contiguous()


CViT = variant_class(NAME)

__all__ = ["CViT", "NAME", "idw_fold"]
