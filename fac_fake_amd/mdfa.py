"""Drop-ins for ``CViT-main/model/other/cvit_GGCA4_MDFA5.py``, ``cvit_MDFA_BFM.py``
and ``cvit_BFM_MDFA.py`` on gfx950 HIP kernels, and their MDFA block as one
``fac_mdfa`` call.

The three classes are the (4, 1) plain CViT stem with ``x = MDFA(C, C)(x)`` on
a feature map (256x14x14 after ``features1``, or 512x7x7 after the stem) and
GGCA or ``BFM(x, x)`` at the other site; they keep the CViT's channel / pool
plan, patch, 2-token tail and ``pos_embedding`` rule, so each is
``variants.VariantCViT`` on its ``weights.MDFA_VARIANTS`` entry.  The two BFM
classes also carry a ``self.ggca`` that their forward never calls: its tensors
are in the ``state_dict`` (loaded, kept, returned) and never uploaded.  This
module holds the block's host fold, packing and launch (the ``mdfa`` step) and
the factory by name.

The block (mdfa.hip has the derivation).  Four conv branches of one map (a 1x1
and three 3x3 with padding = dilation = 6, 12, 18), each conv -> BatchNorm ->
ReLU, a fifth branch from the crop's channel means, the 5C-channel cat, the
hebing gate ``max(cat * t_b, cat * s_p)``, times cat, through ``conv_cat``.  On
a 7..14 wide map most dilated taps lie outside it for every pixel; the cat is
non-negative, so the gate is one scalar ``m_p = max(t_b, s_p)`` per pixel that
commutes with the 1x1 ``conv_cat``; branch 5 is one vector per crop.  What runs
is ``out = ReLU(m_p (W'cat[:, :4C] cat4_p^2 + e_b) + b'cat)``.

Every eval BatchNorm is folded into its conv on the host in fp32
(``mdfa_fold``) before the one rounding to 16 bits (``fac_mdfa_pack``).

Grad-CAM is not implemented for the classes.
"""
from __future__ import annotations

import torch

from . import _lib
from .variants import BN_EPS, VariantCViT, variant_class
from .weights import MDFA_NAMES, MDFA_VARIANTS

PACK_ORDER = ("w1", "w2", "w3", "w4", "bias4", "w5", "b5", "wcat", "bcat", "ws", "wt")


def _bn_fold(sd, conv: str, bn: str):
    f = lambda k: sd[k].detach().to("cpu", torch.float32)  # noqa: E731
    s = f(bn + ".weight") / torch.sqrt(f(bn + ".running_var") + BN_EPS)
    w = f(conv + ".weight")
    return ((w * s.view(-1, 1, 1, 1)).contiguous(),
            ((f(conv + ".bias") - f(bn + ".running_mean")) * s + f(bn + ".bias")).contiguous())


def mdfa_fold(sd, prefix: str = "mdfa"):
    """The MDFA block (state_dict prefix) as fac_mdfa_pack's operands, fp32 on
    the host, every BatchNorm folded: dict(w1 [c,c], w2 w3 w4 [c,c,3,3]
    (dilation 6, 12, 18), bias4 [4,c], w5 [c,c], b5 [c], wcat [c,5c], bcat [c],
    ws [5c] = Hebing.kongjian's, wt [5c] = Hebing.tongdao's)."""
    p = prefix + "."
    ops, bias = {}, []
    for i in range(1, 5):
        w, b = _bn_fold(sd, f"{p}branch{i}.0", f"{p}branch{i}.1")
        ops[f"w{i}"] = w.reshape(w.shape[0], w.shape[1]).contiguous() if i == 1 else w
        bias.append(b)
    ops["bias4"] = torch.stack(bias).contiguous()
    w5, ops["b5"] = _bn_fold(sd, p + "branch5_conv", p + "branch5_bn")
    ops["w5"] = w5.reshape(w5.shape[0], w5.shape[1]).contiguous()
    wc, ops["bcat"] = _bn_fold(sd, p + "conv_cat.0", p + "conv_cat.1")
    ops["wcat"] = wc.reshape(wc.shape[0], wc.shape[1]).contiguous()
    ops["ws"] = sd[p + "Hebing.kongjian.Conv1x1.weight"].detach().to("cpu", torch.float32).reshape(-1).contiguous()
    ops["wt"] = sd[p + "Hebing.tongdao.fc.weight"].detach().to("cpu", torch.float32).reshape(-1).contiguous()
    c = ops["bcat"].shape[0]
    want = dict(w1=(c, c), w2=(c, c, 3, 3), w3=(c, c, 3, 3), w4=(c, c, 3, 3), bias4=(4, c), w5=(c, c), b5=(c,),
                wcat=(c, 5 * c), bcat=(c,), ws=(5 * c,), wt=(5 * c,))
    for k, shape in want.items():
        if tuple(ops[k].shape) != shape:
            raise ValueError(f"MDFA {k}: expected {list(shape)}, got {list(ops[k].shape)}")
    return ops


def mdfa_pack(ops: dict, dtype: str, device) -> torch.Tensor:
    """fac_mdfa_pack of mdfa_fold's operands -> the device blob mdfa16 takes."""
    lib = _lib.load()
    c = ops["bcat"].shape[0]
    n = lib.fac_mdfa_packed_bytes(c)
    if n == 0:
        raise ValueError(f"MDFA with {c} channels is not a fac_mdfa shape")
    host = [ops[k].detach().to("cpu", torch.float32).contiguous() for k in PACK_ORDER]
    out = torch.empty(n, dtype=torch.uint8)
    _lib.check(lib.fac_mdfa_pack(_lib.DTYPES[dtype], c, *[t.data_ptr() for t in host], out.data_ptr()), None,
               "fac_mdfa_pack")
    return out.to(device)


def mdfa16(x: torch.Tensor, packed: torch.Tensor, dtype: str, scratch: torch.Tensor | None = None) -> torch.Tensor:
    """MDFA(x) on a [B,h,w,c] 16-bit NHWC device tensor (one fac_mdfa call,
    four launches).  scratch: at least fac_mdfa_scratch_bytes(B, h, w, c) bytes
    on x's device; allocated per call when None."""
    B, h, w, c = x.shape
    lib = _lib.load()
    need = lib.fac_mdfa_scratch_bytes(B, h, w, c)
    if need == 0:
        raise ValueError(f"[{B},{h},{w},{c}] is not a fac_mdfa shape")
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=x.device)
    elif scratch.numel() * scratch.element_size() < need:
        raise ValueError(f"fac_mdfa needs {need} scratch bytes, got {scratch.numel() * scratch.element_size()}")
    out = torch.empty_like(x)
    _lib.check(lib.fac_mdfa(_lib.DTYPES[dtype], x.data_ptr(), B, h, w, c, packed.data_ptr(), out.data_ptr(),
                            scratch.data_ptr(), torch.cuda.current_stream(x.device).cuda_stream), None, "fac_mdfa")
    return out


class FusedMDFA:
    """The block as one fac_mdfa call on operands packed once; the scratch is
    kept and grown with the largest batch seen."""

    def __init__(self, ops: dict, dtype: str, device):
        self.packed = mdfa_pack(ops, dtype, device)
        self.dtype = dtype
        self._scratch = None

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        need = _lib.load().fac_mdfa_scratch_bytes(*x.shape)
        if self._scratch is None or self._scratch.numel() < need or self._scratch.device != x.device:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=x.device)
        return mdfa16(x, self.packed, self.dtype, self._scratch)


MdfaCViT = VariantCViT       # the classes have no body of their own


def mdfa_class(name: str) -> type:
    """The drop-in class of reference file ``model/other/<name>.py`` (its ``CViT``)."""
    if name not in MDFA_VARIANTS:
        raise KeyError(f"unknown MDFA CViT {name!r}; known: {', '.join(MDFA_NAMES)}")
    return variant_class(name)


def CViT(name: str, *args, **kwargs) -> VariantCViT:
    """``mdfa_class(name)(*args, **kwargs)``: the reference's constructor arguments plus ``dtype``."""
    return mdfa_class(name)(*args, **kwargs)


__all__ = ["CViT", "FusedMDFA", "MDFA_NAMES", "MDFA_VARIANTS", "MdfaCViT", "PACK_ORDER", "mdfa16", "mdfa_class",
           "mdfa_fold", "mdfa_pack"]
