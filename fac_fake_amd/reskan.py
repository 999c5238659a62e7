"""Drop-in ``ResKan`` (ResNet-34 + KAN) on gfx950 HIP kernels.

Mirrors ``CViT-main/ResKan/kan_resnet.py`` (:132-260): ``ResNet`` /
``resnet34(set_device, num_classes, include_top, include_top_kan)`` in the
trainer's configuration (``num_classes=2, include_top=False,
include_top_kan=True``, ResKan_train.py:68-70), the same 224-key
``state_dict`` (names, shapes, order) and ``forward(img)`` on a normalised fp32
NCHW ``[B,3,224,224]`` batch returning fp32 logits ``[B,2]`` (eval mode).
There is no ``pos_embedding``: any ``B >= 1`` is valid.

Arithmetic (no CPU fallback, every layer is a HIP kernel of libfac_cvit.so):

* conv1 7x7/2 + bn1 + ReLU + MaxPool2d(3, 2, 1): one launch, the 4x4 conv over
  space-to-depth cells with the fused pool (``ConvLayer(..., maxpool3s2=True)``).
* BasicBlock (kan_resnet.py:38-65): ``conv1`` + bn1 + ReLU is ``fac_conv3x3``
  (stride 1 at 56^2 / 28^2 / 14^2) or ``fac_conv_nd`` (the 3x3/2 convs and
  layer4's 7^2 ones); the 1x1/2 downsample + BN is ``fac_conv_nd``; ``conv2`` +
  bn2, + identity, ReLU - in that order - is one ``fac_conv3x3_res`` launch
  (resnet.hip), the identity added in fp32 before the one 16-bit rounding.
  BatchNorm (eps 1e-5) is folded on the host in fp32.  Activations are 16-bit
  NHWC.
* AdaptiveAvgPool2d((1, 1)): ``fac_avgpool_f32``, 16-bit in, fp32 out; its
  output goes straight into ``KAN([512, 64, 2])`` (two ``fac_kan_linear``
  launches in fp32), so the KAN's input is never rounded to 16 bits.

The whole forward can be captured into a hipGraph (``torch.cuda.graph``) after
one eager forward: every launch goes to the current torch stream, workspaces
come from torch's caching allocator.
"""
from __future__ import annotations

import torch
from torch import nn

from . import _lib
from .cvit import _Node, weight_versions
from .ops import (TORCH16, Conv3x3Res, ConvLayer, KANLinearLayer, avgpool_f32, fold_bn, pack_input_s2d, s2d_weight,
                  sigmoid)
from .resvitkan import _init_tensor
from .weights import resnet34_blocks, reskan_param_specs

SUPPORTED = dict(num_classes=2, include_top=False, include_top_kan=True)
BN_EPS = 1e-5
MEAN = (0.485, 0.456, 0.406)     # helpers/loader.py:9 (the training normalisation)
STD = (0.229, 0.224, 0.225)
_BUFFERS = ("rmean", "rvar", "nbt", "kgrid")
_NO_CPU = "ResKan (gfx950 HIP path) needs its input on a GPU device; there is no CPU fallback"


class ResNet(nn.Module):
    # the maps whose second conv runs on fac_conv3x3_res; a BasicBlock at any
    # other map keeps fac_conv_nd with FAC_CONV_RESID | FAC_CONV_RELU2
    # (profiles/reskan_bench.txt holds both routes' times per map)
    RES_KERNEL_MAPS = (56, 28, 14, 7)

    def __init__(self, block=None, blocks_num=(3, 4, 6, 3), set_device=None, num_classes=1000, include_top=False,
                 include_top_kan=True, groups=1, width_per_group=64, *, dtype: str = "fp16"):
        super().__init__()
        cfg = dict(num_classes=num_classes, include_top=include_top, include_top_kan=include_top_kan)
        if cfg != SUPPORTED or list(blocks_num) != [3, 4, 6, 3] or groups != 1 or width_per_group != 64 or \
                getattr(block, "expansion", 1) != 1:
            raise NotImplementedError(f"the gfx950 ResKan path implements resnet34 (BasicBlock [3,4,6,3]) with "
                                      f"{SUPPORTED}, got {cfg}, blocks_num={list(blocks_num)}")
        if dtype not in _lib.DTYPES:
            raise ValueError(f"dtype must be one of {list(_lib.DTYPES)}")
        self.dtype_name = dtype
        self.include_top, self.include_top_kan = include_top, include_top_kan
        for name, shape, kind in reskan_param_specs(num_classes=num_classes):
            *path, leaf = name.split(".")
            mod = self
            for p in path:
                if p not in mod._modules:
                    mod.add_module(p, _Node())
                mod = mod._modules[p]
            t = _init_tensor(name, shape, kind)
            if kind in _BUFFERS:
                mod.register_buffer(leaf, t)
            else:
                mod.register_parameter(leaf, nn.Parameter(t))
        self._prep = None          # (device index, versions) the packed layers belong to
        self.eval()

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        out = super().load_state_dict(state_dict, strict=strict, assign=assign)
        self._prep = None
        return out

    def train(self, mode: bool = True):
        if mode:
            raise RuntimeError("the gfx950 ResKan path is inference-only (BatchNorm is folded into the convs)")
        return super().train(False)

    def _prepare(self, device: torch.device):
        idx = device.index if device.index is not None else torch.cuda.current_device()
        v = weight_versions(self)
        if self._prep == (idx, v):
            return
        sd = self.state_dict()
        dt = self.dtype_name

        def folded(ck, bnp):
            return fold_bn(sd[ck], None, sd[bnp + ".weight"], sd[bnp + ".bias"], sd[bnp + ".running_mean"],
                           sd[bnp + ".running_var"], BN_EPS)

        def conv(ck, bnp, stride=1, pad=0):
            return ConvLayer(*folded(ck, bnp), stride, pad, dtype=dt, device=device)

        # conv1 7x7/2 (3 channels) as a 4x4/1 conv over space-to-depth cells (ops.s2d_weight)
        w1, b1 = folded("conv1.weight", "bn1")
        self._conv1 = ConvLayer(s2d_weight(w1), b1, 1, 0, dtype=dt, device=device)
        self._blocks = []
        h = 56
        for p, _inp, _ch, s, ds in resnet34_blocks():
            h //= s
            c1 = conv(p + ".conv1.weight", p + ".bn1", s, 1)
            if h in self.RES_KERNEL_MAPS:
                c2 = Conv3x3Res(*folded(p + ".conv2.weight", p + ".bn2"), h, dtype=dt, device=device)
            else:
                c2 = conv(p + ".conv2.weight", p + ".bn2", 1, 1)
            self._blocks.append((c1, c2, conv(p + ".downsample.0.weight", p + ".downsample.1", s) if ds else None))
        self._kan = [KANLinearLayer(sd[f"kan.layers.{i}.grid"], sd[f"kan.layers.{i}.base_weight"],
                                    sd[f"kan.layers.{i}.spline_weight"], sd[f"kan.layers.{i}.spline_scaler"], device)
                     for i in range(2)]
        self._prep = (idx, v)

    # ------------------------------------------------------------------ forward
    def features16(self, x16: torch.Tensor, taps: list | None = None) -> torch.Tensor:
        """ResNet.forward up to layer4 (kan_resnet.py:236-244) on space-to-depth
        packed 16-bit cells [B,1,115,115,16] (ops.pack_input_s2d) ->
        [B,1,7,7,512] 16-bit NHWC.  With `taps`: the max-pool output and every
        BasicBlock's output are appended to it."""
        tap = taps.append if taps is not None else (lambda t: None)
        # 7x7/2 + bn1 + ReLU + MaxPool2d(3, 2, 1) in one launch (conv_s2d4_mp)
        x = self._conv1(x16, maxpool3s2=True)
        tap(x)
        for c1, c2, ds in self._blocks:
            identity = ds(x, relu=False) if ds is not None else x
            h = c1(x)
            if isinstance(c2, Conv3x3Res):
                x = c2(h, identity)                                  # bn2, + identity, ReLU
            else:
                x = c2(h, relu=False, residual=identity, relu2=True)
            tap(x)
        return x

    def _check_u8(self, crops: torch.Tensor):
        if crops.dtype != torch.uint8 or crops.dim() != 4 or tuple(crops.shape[1:]) != (224, 224, 3):
            raise ValueError(f"expected uint8 crops [B,224,224,3], got {crops.dtype} {tuple(crops.shape)}")
        if not crops.is_cuda:
            raise RuntimeError(_NO_CPU)
        if crops.shape[0] < 1:
            raise ValueError("expected at least one crop")

    def stage_outputs(self, crops: torch.Tensor) -> list:
        """For uint8 crops [B,224,224,3]: what a forward hook on the reference's
        ``maxpool``, each ``layerN[b]`` (17 tensors, NHWC 16-bit) and
        ``avgpool`` (fp32 [B,512]) sees, for per-block parity."""
        self._check_u8(crops)
        self._prepare(crops.device)
        x16 = pack_input_s2d(crops, dtype=self.dtype_name, u8=True, div=255.0, mean=MEAN, std=STD)
        taps = []
        taps.append(avgpool_f32(self.features16(x16, taps)))
        return taps

    def _run(self, x16: torch.Tensor, want_probs: bool):
        pooled = avgpool_f32(self.features16(x16))
        logits = self._kan[1](self._kan[0](pooled))
        return logits, (sigmoid(logits) if want_probs else None)

    def forward(self, img: torch.Tensor) -> torch.Tensor:
        if not img.is_cuda:
            raise RuntimeError(_NO_CPU)
        if img.dim() != 4 or tuple(img.shape[1:]) != (3, 224, 224) or img.shape[0] < 1:
            raise ValueError(f"expected img [B,3,224,224], got {tuple(img.shape)}")
        self._prepare(img.device)
        x16 = pack_input_s2d(img.float(), dtype=self.dtype_name, u8=False)
        return self._run(x16, False)[0]

    def forward_u8(self, crops: torch.Tensor, pos_index=None, return_probs: bool = False):
        """uint8 NHWC RGB crops [B,224,224,3]; x/255 + ImageNet Normalize fused
        into the input packing.  ``pos_index`` is accepted and ignored (the
        model has no pos_embedding), so the CViT scoring helpers
        (prediction.predict_crops, video.predict_videos) take this model."""
        self._check_u8(crops)
        self._prepare(crops.device)
        x16 = pack_input_s2d(crops, dtype=self.dtype_name, u8=True, div=255.0, mean=MEAN, std=STD)
        logits, probs = self._run(x16, return_probs)
        return (logits, probs) if return_probs else logits

    def forward_u8_pipelined(self, crops: torch.Tensor, pos_index=None, chunk: int = 256, equal: bool = False):
        """forward_u8 in chunks of at most ``chunk`` crops, concatenated (the
        call video.score_selected makes for more crops than one batch).  A
        crop's logits do not depend on its batch, so this equals one
        forward_u8 bit for bit; ``pos_index`` and ``equal`` are ignored."""
        self._check_u8(crops)
        step = max(int(chunk), 1)
        return torch.cat([self.forward_u8(crops[i:i + step]) for i in range(0, crops.shape[0], step)])


def resnet34(set_device=None, num_classes=1000, include_top=False, include_top_kan=True, *, dtype: str = "fp16"):
    """kan_resnet.py:258-260."""
    return ResNet(None, [3, 4, 6, 3], set_device=set_device, num_classes=num_classes, include_top=include_top,
                  include_top_kan=include_top_kan, dtype=dtype)


__all__ = ["ResNet", "resnet34", "TORCH16"]
