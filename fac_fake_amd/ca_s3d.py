"""Drop-in ``CA_S3D_v3`` and ``ContextBlock3d`` on gfx950 HIP kernels.

Mirrors ``sx_exp_deepfakedetect-master/S3D/CA_S3D.py::CA_S3D_v3`` (:9-60):
the S3D of fac_fake_amd/s3d.py with a GCNet context block
(``new_model/context_block_3d.py::ContextBlock3d``, 'avg' pooling,
'channel_add' fusion) after Mixed_3b, 4b, 4c, 4d, 4e and 5b.  Same
constructor ``CA_S3D_v3(num_class, SRM_net)``, the same 501-key
``state_dict`` (``base.{0..21}``: the context blocks are ``base.6, 10, 12, 14,
16, 20`` with ``channel_add_conv.{0,1,3}``), the same ``forward`` on a raw clip.

Every S3D layer runs as in s3d.S3D; each context block is one
``fac_context_add`` call (csrc/context.hip), in place on the Mixed block's
output: fp32 global mean over (T, H, W), Conv1x1x1(C -> C/16) +
LayerNorm + ReLU6 + Conv1x1x1(C/16 -> C) in fp32, one fp32 add and one
16-bit rounding per element.  Inference only; no CPU fallback.
"""
from __future__ import annotations

import torch
from torch import nn

from . import _lib
from .ops import TORCH16, ContextAdd
from .s3d import LN_EPS, S3D, custom_round, custom_video_round, video_predictions
from .weights import ca_s3d_base, ca_s3d_param_specs


class CA_S3D_v3(S3D):
    def _base_desc(self):
        return ca_s3d_base(self._srm)

    def _param_specs(self):
        return ca_s3d_param_specs(self.num_class, self._srm)


class ContextBlock3d(nn.Module):
    """``ContextBlock3d(inplanes, ratio, pooling_type, fusion_types)`` with the
    reference's attributes and state_dict (``channel_add_conv.0`` Conv3d,
    ``.1`` LayerNorm([planes, 1, 1, 1]), ``.2`` ReLU6, ``.3`` Conv3d).  Built
    here: ``pooling_type='avg'`` with ``fusion_types=('channel_add',)``, what
    CA_S3D_v3 instantiates.  ``forward`` takes the reference's ``[N, C, T, H,
    W]`` tensor on a GPU (any float type; it is rounded to `dtype`, as the
    model's activations are) and returns the same layout and type;
    ``forward_cl`` takes and returns the project's 16-bit channels-last
    ``[N, T, H, W, C]``."""

    def __init__(self, inplanes, ratio, pooling_type="att", fusion_types=("channel_add",), *, dtype: str = "fp16"):
        super().__init__()
        assert pooling_type in ["avg", "att"]
        assert isinstance(fusion_types, (list, tuple))
        assert all(f in ["channel_add", "channel_mul"] for f in fusion_types)
        assert len(fusion_types) > 0, "at least one fusion should be used"
        if pooling_type != "avg" or tuple(fusion_types) != ("channel_add",):
            raise NotImplementedError(
                f"ContextBlock3d(pooling_type={pooling_type!r}, fusion_types={tuple(fusion_types)!r}): the gfx950 "
                "path supports pooling_type='avg' with fusion_types=('channel_add',) only (attention pooling "
                "'att' and the 'channel_mul' fusion are not built)")
        if dtype not in _lib.DTYPES:
            raise ValueError(f"dtype must be one of {list(_lib.DTYPES)}")
        self.inplanes = inplanes
        self.ratio = ratio
        self.planes = int(inplanes * ratio)
        self.pooling_type = pooling_type
        self.fusion_types = fusion_types
        self.dtype_name = dtype
        self.avg_pool = nn.AdaptiveAvgPool3d(1)
        self.channel_add_conv = nn.Sequential(
            nn.Conv3d(self.inplanes, self.planes, kernel_size=1),
            nn.LayerNorm([self.planes, 1, 1, 1]),
            nn.ReLU6(inplace=True),
            nn.Conv3d(self.planes, self.inplanes, kernel_size=1))
        self.channel_mul_conv = None
        self._prep = None
        self.eval()

    def train(self, mode: bool = True):
        if mode:
            raise RuntimeError("the gfx950 ContextBlock3d is inference-only")
        return super().train(False)

    def _layer(self, device) -> ContextAdd:
        a = self.channel_add_conv
        ps = (a[0].weight, a[0].bias, a[1].weight, a[1].bias, a[3].weight, a[3].bias)
        key = (device, tuple((t.data_ptr(), t._version) for t in ps))
        if self._prep is None or self._prep[0] != key:
            self._prep = (key, ContextAdd(*ps, eps=a[1].eps, dtype=self.dtype_name, device=device))
        return self._prep[1]

    def forward_cl(self, x16: torch.Tensor, inplace: bool = False, route: int = 0) -> torch.Tensor:
        if not x16.is_cuda:
            raise RuntimeError("ContextBlock3d (gfx950 HIP path) needs its input on a GPU device; no CPU fallback")
        return self._layer(x16.device)(x16, inplace=inplace, route=route)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 5 or x.shape[1] != self.inplanes:
            raise ValueError(f"expected [N, {self.inplanes}, T, H, W], got {tuple(x.shape)}")
        # (copy=True: the in-place add below must never reach the caller's tensor)
        y = self.forward_cl(x.permute(0, 2, 3, 4, 1).to(TORCH16[self.dtype_name], copy=True).contiguous(), inplace=True)
        return y.permute(0, 4, 1, 2, 3).to(x.dtype)


__all__ = ["CA_S3D_v3", "ContextBlock3d", "LN_EPS", "custom_round", "custom_video_round", "video_predictions"]
