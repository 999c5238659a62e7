"""Drop-in CViT RepBn8 variant on gfx950 HIP kernels.

Mirrors ``CViT-main/model/cvit_GGCA_ADD_DEConv_RepBn8.py::CViT`` (:343-455),
the variant most of the reference's recorded predictions come from
(``wprediction/4090RepBn8_*.csv``): the same constructor, the same 359-key
``state_dict`` (names, shapes, order — DEConv's five kernels, GGCA,
LinearNorm's counters and its unused RepBN branch, the unused top-level
``Deconv``) and ``forward(img, mask=None)`` on a normalised fp32 NCHW
``[B,3,224,224]`` batch returning fp32 logits ``[B,2]`` in eval mode, with
the reference's batch-slot ``pos_embedding`` rule.

Arithmetic (no CPU fallback, every layer is a HIP kernel of libfac_cvit.so):

* The 18 convs of ``features1`` / ``features2`` run on the CViT's own
  conv-stack kernels: each DEConv (:320-340) is folded on the host at load
  time into the single 3x3 kernel its eval forward convolves with
  (``deconv_fold``, the reference's weight algebra in its op order, fp32),
  eval BatchNorm is folded on top; the first block (conv, DEConv, DEConv,
  pool — the CViT's conv1-3 shape) is the fused ``fac_stem224`` kernel with
  the input normalisation, every later conv one ``fac_conv3x3`` launch
  (halo-staged implicit GEMM, 16-bit NHWC, fp32 accumulation, the 2x2
  max-pool and the ReLU in its epilogue — no ReLU after ``features1.26``,
  :390-392).
* ``x = x * GGCA(x)`` (:144-207, :436-437) is one ``fac_ggca`` launch.
* Patch embedding, cls/pos, the transformer and the head are the CViT tail
  kernels (``fac_forward_features`` on a "tail_only" context); the
  FeedForward PreNorm is LinearNorm, whose eval branch is LayerNorm(eps 1e-6)
  (:22-48), set with the context option ``ffn_ln_eps_exp`` = 6.

The whole forward is stream-ordered on the current torch stream and can be
captured into a hipGraph.  All of that is ``variants.VariantCViT`` on this
class's ``weights.CVIT_FAMILY`` entry; what this module adds is the ``fac_ggca``
launch as the stem's GGCA step and the two halves of Grad-CAM.
"""
from __future__ import annotations

import torch

from . import _lib
from .ops import TORCH16, sigmoid
from .variants import SUPPORTED, VariantCViT, _pos_index, deconv_fold
from .weights import REPBN8_NAME


class CViT(VariantCViT):
    """cvit_GGCA_ADD_DEConv_RepBn8.CViT on gfx950 (inference)."""

    variant = REPBN8_NAME

    def features(self, src: torch.Tensor, u8: bool, layers=None) -> torch.Tensor:
        """features1 + features2 (:432-435) -> [B,7,7,512] 16-bit NHWC.  src:
        uint8 NHWC crops (u8) or normalised fp32 NCHW images.  layers: the
        steps of self._steps to run (default all before the GGCA combine)."""
        return self._walk(src, u8, self._steps[:-1] if layers is None else layers)

    # ------------------------------------------------------------------ Grad-CAM (fac_fake_amd/gradcam.py)
    def gradcam_features(self, src: torch.Tensor, u8: bool):
        """(A, feat): features2[-3]'s output, the last BatchNorm before ReLU and MaxPool (16-bit NHWC
        [B,14,14,512]), and features2's output as features() gives it ([B,7,7,512], bit-identical): the
        last conv runs twice on the same input, once with relu = pool = 0."""
        self._prepare(src.device)
        x = self.features(src, u8, self._steps[:-2])
        s, _run, ops = self._steps[-2]
        a = torch.empty(x.shape[0], s.H, s.H, s.co, dtype=x.dtype, device=x.device)
        feat = torch.empty(x.shape[0], s.H // 2, s.H // 2, s.co, dtype=x.dtype, device=x.device)
        st = torch.cuda.current_stream(x.device).cuda_stream
        for out, pl, relu in ((a, 0, 0), (feat, 1, 1)):
            self._conv3x3(x, s, ops, pl, relu, out, st)
        return a, feat

    def gradcam_tail(self, feat: torch.Tensor, pos_index, target: torch.Tensor):
        """(logits [B,2], d logits[b][target[b]] / d feat as fp32 [B,7,7,512]) through x * GGCA(x) and the
        tail; target int32 [B] on the device, -1 = the crop's argmax."""
        self._prepare(feat.device)
        lib = _lib.load()
        B, dev = feat.shape[0], feat.device
        st = torch.cuda.current_stream(dev).cuda_stream
        pidx = _pos_index(B, pos_index, dev)
        wf = self.weighted_features16(feat)
        logits = torch.empty(B, 2, dtype=torch.float32, device=dev)
        gw = torch.empty(B, 7, 7, 512, dtype=torch.float32, device=dev)
        _lib.check(lib.fac_gradcam_tail(self._ctx, wf.data_ptr(), B, pidx.data_ptr(), target.data_ptr(),
                                        logits.data_ptr(), gw.data_ptr(), st), self._ctx, "fac_gradcam_tail")
        grad = torch.empty_like(gw)
        w1, b1, bn4, w2, b2 = self._ggca
        _lib.check(lib.fac_ggca_mul_bwd(_lib.DTYPES[self.dtype_name], feat.data_ptr(), gw.data_ptr(), B, 7, 7, 512, 4,
                                        w1.data_ptr(), b1.data_ptr(), bn4.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                                        grad.data_ptr(), st), None, "fac_ggca_mul_bwd")
        return logits, grad

    def weighted_features16(self, f: torch.Tensor) -> torch.Tensor:
        """x * GGCA(x) (:436-437) on [B,(1,)7,7,512] 16-bit NHWC."""
        B, (H, W, C) = f.shape[0], f.shape[-3:]
        out = torch.empty_like(f)
        w1, b1, bn4, w2, b2 = self._ggca
        _lib.check(_lib.load().fac_ggca(_lib.DTYPES[self.dtype_name], f.data_ptr(), B, H, W, C, 4, w1.data_ptr(),
                                        b1.data_ptr(), bn4.data_ptr(), w2.data_ptr(), b2.data_ptr(), out.data_ptr(),
                                        torch.cuda.current_stream(f.device).cuda_stream), None, "fac_ggca")
        return out

    ggca_combine16 = weighted_features16     # the stem's ggca step: fac_ggca, not fac_ggca_apply's op 0


__all__ = ["CViT", "SUPPORTED", "TORCH16", "deconv_fold", "sigmoid"]
