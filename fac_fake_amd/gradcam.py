"""Grad-CAM heatmaps of the CViT and CViT RepBn8 drop-ins on gfx950.

Interface parity with ``CViT-main/figure/utils.py::GradCAM`` (:57-181) as
``figure/gradcam_cnn.py`` uses it: the same constructor, context-manager use
and ``__call__(input_tensor, target_category=None)`` returning
``np.float32 [B,224,224]``; ``figure/utils.py`` in the repository root
re-exports the class, so ``sys.path.insert(1, 'figure'); from utils import
GradCAM`` works as in the reference.

The reference hooks the target layer and runs ``loss.backward()`` through the
whole model.  Here the target layer is fixed to the one the reference script
uses — the last BatchNorm, a 512 x 14 x 14 map before ReLU and max-pool
(``features2[-3]`` of RepBn8, ``features[-3]`` of the base CViT) — and the
gradient of the chosen logit with respect to that map comes from the HIP
backward kernels of ``csrc/gradcam.hip`` (fp32 from the logit to the map, no
weight gradients, no atomics).  There is no autograd and no CPU fallback.

``compute()`` returns device tensors without a host synchronisation;
``__call__`` is ``compute()`` plus the copy to numpy.  ``show_cam_on_image``
and ``center_crop_img`` (cv2's colormap) are not provided.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from . import cvit as _cvit
from . import repbn8 as _repbn8

TARGET_LAYER = {_cvit.CViT: "features.53", _repbn8.CViT: "features2.10"}
MAX_BATCH = _cvit.MAX_SLOTS


class GradCAM:
    def __init__(self, model, target_layers=None, reshape_transform=None, use_cuda=False):
        name = TARGET_LAYER.get(type(model))
        if name is None:
            raise NotImplementedError("GradCAM on gfx950 takes a fac_fake_amd.cvit.CViT or a fac_fake_amd.repbn8.CViT, "
                                      f"got {type(model).__name__}")
        if reshape_transform is not None:
            raise NotImplementedError("reshape_transform is not supported: only the CNN Grad-CAM of gradcam_cnn.py "
                                      f"(target layer '{name}', the last BatchNorm's 512x14x14 map) is implemented, "
                                      "not the transformer Grad-CAM of gradcam_transformer.py")
        if target_layers is not None:
            layers = [target_layers] if isinstance(target_layers, (str, torch.nn.Module)) else list(target_layers)
            if len(layers) != 1 or not self._is_target(model, layers[0], name):
                raise NotImplementedError(f"the only supported target layer of {type(model).__module__}.CViT is "
                                          f"'{name}' (the last BatchNorm, before ReLU and max-pool), given as None, "
                                          f"the name, or a one-element list; got {target_layers!r}")
        self.model = model.eval()
        self.target_layers = [name]
        self.reshape_transform = None
        self.cuda = use_cuda
        if use_cuda:
            self.model = model.cuda()

    @staticmethod
    def _is_target(model, layer, name: str) -> bool:
        if isinstance(layer, str):
            return layer == name
        return isinstance(layer, torch.nn.Module) and layer is model.get_submodule(name)

    # ------------------------------------------------------------------ device path
    def compute(self, input_tensor: torch.Tensor, target_category=None, pos_index=None):
        """(heatmap [B,224,224] fp32, cam14 [B,14,14] fp32, logits [B,2]) on the device, no host sync.
        input_tensor: normalised fp32 NCHW [B,3,224,224] or uint8 NHWC [B,224,224,3], B = 1..32."""
        x = input_tensor
        if x.dim() != 4:
            raise ValueError(f"expected a 4-d batch of crops, got {tuple(x.shape)}")
        u8 = x.dtype == torch.uint8
        if u8 and tuple(x.shape[1:]) != (224, 224, 3):
            raise ValueError(f"expected uint8 crops [B,224,224,3], got {tuple(x.shape)}")
        if not u8 and tuple(x.shape[1:]) != (3, 224, 224):
            raise ValueError(f"expected img [B,3,224,224], got {tuple(x.shape)}")
        B = x.shape[0]
        if B < 1:
            raise ValueError("GradCAM needs at least one crop")
        if B > MAX_BATCH:
            # the forward's own error past 32 crops (`x += self.pos_embedding[0:B]`, cvit.py:175)
            raise RuntimeError(f"The size of tensor a ({B}) must match the size of tensor b ({MAX_BATCH}) "
                               f"at non-singleton dimension 0")
        if self.cuda:
            x = x.cuda()
        if not x.is_cuda:
            raise RuntimeError("GradCAM (gfx950 HIP path) needs its input on a GPU device; there is no CPU fallback")
        x = x.contiguous() if u8 else x.to(torch.float32).contiguous()
        target = self._targets(target_category, B, x.device)
        m = self.model
        a, feat = m.gradcam_features(x, u8)
        logits, gfeat = m.gradcam_tail(feat, pos_index, target)
        lib = _lib.load()
        dti = _lib.DTYPES[m.dtype_name]
        st = torch.cuda.current_stream(x.device).cuda_stream
        ga = torch.empty(B, 14, 14, 512, dtype=torch.float32, device=x.device)
        _lib.check(lib.fac_relu_pool_bwd(dti, a.data_ptr(), gfeat.data_ptr(), B, 7, 512, ga.data_ptr(), st), None,
                   "fac_relu_pool_bwd")
        cam14 = torch.empty(B, 14, 14, dtype=torch.float32, device=x.device)
        heat = torch.empty(B, 224, 224, dtype=torch.float32, device=x.device)
        _lib.check(lib.fac_gradcam_cam(dti, a.data_ptr(), ga.data_ptr(), B, None, cam14.data_ptr(), heat.data_ptr(),
                                       st), None, "fac_gradcam_cam")
        return heat, cam14, logits

    @staticmethod
    def _targets(target_category, B: int, device) -> torch.Tensor:
        """int32 [B] on the device; -1 = the argmax of the crop's logits (taken on the device)."""
        if target_category is None:
            return torch.full((B,), -1, dtype=torch.int32, device=device)
        if isinstance(target_category, (int, np.integer)):
            t = [int(target_category)] * B
        elif isinstance(target_category, torch.Tensor):
            t = target_category.reshape(-1).tolist()
        else:
            t = [int(v) for v in target_category]
        assert len(t) == B, "target_category needs one entry per crop"     # utils.py:150
        if any(v not in (0, 1) for v in t):
            raise IndexError(f"target_category entries must be 0 or 1, got {t}")
        return torch.tensor(t, dtype=torch.int32).to(device)

    def __call__(self, input_tensor, target_category=None, pos_index=None) -> np.ndarray:
        heat, _, _ = self.compute(input_tensor, target_category, pos_index)
        return heat.cpu().numpy()

    # ------------------------------------------------------------------ the reference's context-manager protocol
    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc_value, exc_tb):
        if isinstance(exc_value, IndexError):     # utils.py:176-180
            print(f"An exception occurred in CAM with block: {exc_type}. Message: {exc_value}")
            return True


__all__ = ["GradCAM", "TARGET_LAYER"]
