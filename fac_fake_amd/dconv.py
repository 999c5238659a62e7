"""Drop-in for ``CViT-main/model/cvit_GGCA_ADD_DConv.py`` on gfx950 HIP kernels.

The base CViT with nine of its seventeen 3x3 convs replaced by
``InceptionDWConv2d`` (:157-177: 5/8 of the channels pass, 1/8 each go through
a depthwise 3x3, 1x11 and 11x1 conv), ``x + GGCA(x)`` on the 512x7x7 map and
the base CViT's tail (``nn.LayerNorm`` in both PreNorms).  The contract is
``variants.VariantCViT``'s, whose weight handling, tail and forward it
inherits; the stem is its own:

* conv 3->32 at 224x224: ``fac_pack_input`` to 32 channels (zeros beyond 3, so
  the conv's zero padding lands in normalised space) and one ``fac_conv3x3``
  launch with the folded weight zero beyond input channel 3.  The block's two
  InceptionDWConv2d layers follow it, so the fused ``fac_stem224`` does not apply;
* every ``InceptionDWConv2d -> BatchNorm2d -> ReLU (-> MaxPool2d)``: one
  ``fac_idwconv`` launch (idwconv.hip), the conv biases and the BatchNorm folded
  into a per-channel fp32 scale and shift, the taps left as they are;
* the seven other convs: ``fac_conv3x3`` with the BatchNorm folded.

Grad-CAM is not implemented for this class.
"""
from __future__ import annotations

import torch

from . import _lib
from .ops import TORCH16, fold_bn, pack_input
from .repbn8 import BN_EPS
from .variants import VariantCViT
from .weights import DCONV_LAYERS, dconv_param_specs

NAME = "cvit_GGCA_ADD_DConv"
MEAN = (0.485, 0.456, 0.406)     # cvit_prediction.py:41
STD = (0.229, 0.224, 0.225)      # cvit_prediction.py:42


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


class CViT(VariantCViT):
    """cvit_GGCA_ADD_DConv.CViT on gfx950 (inference)."""

    variant = NAME

    def _table(self):
        return dict(layers=DCONV_LAYERS, ggca=("stem", (512, 7, 7), "add"), ff_norm="layernorm", deconv=False)

    def _param_specs(self, **kw):
        return dconv_param_specs(**kw)

    def folded_layers(self):
        """Per layer ("conv", weight, bias, pool) with the BatchNorm folded, or
        ("idw", w_hw, w_w, w_h, scale, shift, pool) (idw_fold), fp32 on the host."""
        sd = self.state_dict()
        out = []
        for idx, kind, _ci, _co, bn, pl in DCONV_LAYERS:
            p, q = f"features.{idx}", f"features.{bn}"
            if kind == "conv":
                w, b = fold_bn(sd[p + ".weight"], sd[p + ".bias"], sd[q + ".weight"], sd[q + ".bias"],
                               sd[q + ".running_mean"], sd[q + ".running_var"], BN_EPS)
                out.append(("conv", w, b, pl))
            else:
                out.append(("idw", *idw_fold(sd, p, q), pl))
        return out

    def _prepare_stem(self, sd, device):
        layers, H = [], 224
        for i, (kind, *ops, pl) in enumerate(self.folded_layers()):
            if kind == "conv":
                w, b = ops
                if i == 0:      # 3 -> 32 on the 32-channel packed input
                    w = torch.cat([w, torch.zeros(w.shape[0], 32 - w.shape[1], 3, 3)], 1)
                co, ci = w.shape[:2]
                layers.append(("conv", self._packed_conv(w, H, device), b.to(device), H, ci, co, pl))
            else:
                layers.append(("idw", *[t.to(device) for t in ops], H, ops[3].shape[0], pl))
            if pl:
                H //= 2
        self._layers = layers

    def _ggca_after(self):
        return len(DCONV_LAYERS)

    def stem_features(self, src: torch.Tensor, u8: bool, upto=None) -> torch.Tensor:
        """The conv stem and x + GGCA(x) -> [B,7,7,512] 16-bit NHWC.  src: uint8
        NHWC crops (u8) or normalised fp32 NCHW images.  upto: an int stops
        after that many layers (1..17) and returns that map."""
        lib = _lib.load()
        dt = self.dtype_name
        dti = _lib.DTYPES[dt]
        B, dev = src.shape[0], src.device
        st = torch.cuda.current_stream(dev).cuda_stream
        if u8:
            x = pack_input(src, dtype=dt, u8=True, div=255.0, mean=MEAN, std=STD, spatial=(224, 224), c_pad=32)
        else:
            x = pack_input(src, dtype=dt, u8=False, spatial=(224, 224), c_pad=32)
        x = x.view(B, 224, 224, 32)
        for i, (kind, *ops) in enumerate(self._layers):
            if kind == "conv":
                wpk, b, H, ci, co, pl = ops
                Ho = H // 2 if pl else H
                y = torch.empty(B, Ho, Ho, co, dtype=TORCH16[dt], device=dev)
                _lib.check(lib.fac_conv3x3(dti, x.data_ptr(), wpk.data_ptr(), b.data_ptr(), y.data_ptr(), B, H, ci, co,
                                           int(pl), 1, self._zero.data_ptr(), st), None, "fac_conv3x3")
            else:
                w_hw, w_w, w_h, scale, shift, H, c, pl = ops
                Ho = H // 2 if pl else H
                y = torch.empty(B, Ho, Ho, c, dtype=TORCH16[dt], device=dev)
                _lib.check(lib.fac_idwconv(dti, x.data_ptr(), y.data_ptr(), B, H, H, c, w_hw.data_ptr(),
                                           w_w.data_ptr(), w_h.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                           int(pl), st), None, "fac_idwconv")
            x = y
            if upto == i + 1:
                return x
        return self.ggca_combine16(x)


__all__ = ["CViT", "NAME", "idw_fold"]
