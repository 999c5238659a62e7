"""Drop-ins for four ``CViT-main/model/other/cvit_*.py`` classes on gfx950 HIP kernels.

``cvit_GGCA``, ``cvit_GGCA4``, ``cvit_GGCA_ADD3`` and ``cvit_GGCA_SMFA`` keep
the CViT's channel / pool plan, the single 7x7 patch, the 2-token tail and the
batch-slot ``pos_embedding`` rule, so they are ``variants.VariantCViT`` on one
``weights.OTHER_VARIANTS`` entry each; this module holds the SMFA block's host
fold, packing and launch (the ``smfa`` step) and the factory by name:

* ``cvit_GGCA``       ``x = GGCA(512,7,7)(x)`` after the stem: the module's own
                      output ``x * att_h * att_w`` (``fac_ggca_scale``), where
                      variants.py's classes combine ``x * GGCA(x)`` or ``x + GGCA(x)``;
* ``cvit_GGCA4``      ``x = GGCA(256,14,14)(x)`` between ``features1`` and
                      ``features2`` (``fac_ggca_apply``'s LDS route, 4 groups);
* ``cvit_GGCA_ADD3``  the same site, ``x = x + GGCA(x)``;
* ``cvit_GGCA_SMFA``  ``x = x + SMFA(256)(x)`` on the 256x14x14 map between
                      ``features1`` and ``features2`` (one ``fac_smfa`` call,
                      smfa.hip), then ``x = x + GGCA(512,7,7)(x)`` after the stem.

The contract is ``VariantCViT``'s: the reference's constructor, ``state_dict``
(keys, shapes, order), ``forward(img, mask=None, pos_index=None)``,
``forward_u8``, ``reserve`` (which also sizes ``fac_smfa``'s scratch, kept per
model), an inference-only ``train()`` and no CPU fallback.
``other_class(name)`` gives the class the ``model/other/<name>.py`` shims
export.  Grad-CAM is not implemented for these classes.
"""
from __future__ import annotations

import torch

from . import _lib
from .variants import VariantCViT, variant_class
from .weights import OTHER_NAMES, OTHER_VARIANTS, SMFA_DIM


def smfa_fold(sd, prefix: str = "smfa"):
    """The SMFA block (state_dict prefix) as fac_smfa_pack's operands, fp32 on
    the host: dict(w0 [2c,c], b0 [2c], gate4 [4,c] = alpha, dw_conv's centre
    tap, dw_conv's bias, belt, w1 [c,c], b1 [c], dww [2c,9], dwb [2c], wpw
    [2c,2c], bpw [2c], wcat [c,3c] = [linear_2.W | linear_2.W conv_1.W], bcat
    [c] = linear_2.b + linear_2.W conv_1.b)."""
    f = lambda k: sd[f"{prefix}.{k}"].detach().to("cpu", torch.float32)  # noqa: E731
    c = f("alpha").numel()
    w2 = f("linear_2.weight").reshape(c, c)
    wc1 = f("lde.conv_1.weight").reshape(c, 2 * c)
    ops = dict(
        w0=f("linear_0.weight").reshape(2 * c, c), b0=f("linear_0.bias"),
        gate4=torch.stack([f("alpha").reshape(c), f("dw_conv.weight")[:, 0, 1, 1], f("dw_conv.bias"),
                           f("belt").reshape(c)]),
        w1=f("linear_1.weight").reshape(c, c), b1=f("linear_1.bias"),
        dww=f("lde.conv_0.0.weight").reshape(2 * c, 9), dwb=f("lde.conv_0.0.bias"),
        wpw=f("lde.conv_0.1.weight").reshape(2 * c, 2 * c), bpw=f("lde.conv_0.1.bias"),
        wcat=torch.cat([w2, w2 @ wc1], 1), bcat=f("linear_2.bias") + w2 @ f("lde.conv_1.bias"))
    return {k: v.contiguous() for k, v in ops.items()}


_PACK_ORDER = ("w0", "b0", "gate4", "w1", "b1", "dww", "dwb", "wpw", "bpw", "wcat", "bcat")


def smfa_pack(ops: dict, dtype: str, device) -> torch.Tensor:
    """fac_smfa_pack of smfa_fold's operands -> the device blob fac_smfa takes."""
    lib = _lib.load()
    c = ops["b1"].numel()
    nbytes = lib.fac_smfa_packed_bytes(c)
    if nbytes == 0:
        raise ValueError(f"SMFA with {c} channels is not a fac_smfa shape")
    host = [ops[k].detach().to("cpu", torch.float32).contiguous() for k in _PACK_ORDER]
    blob = torch.empty(nbytes, dtype=torch.uint8)
    _lib.check(lib.fac_smfa_pack(_lib.DTYPES[dtype], c, *[t.data_ptr() for t in host], blob.data_ptr()), None,
               "fac_smfa_pack")
    return blob.to(device)


def smfa16(x: torch.Tensor, wpk: torch.Tensor, dtype: str, residual: bool = True, gate_out=None, scratch=None):
    """SMFA(x) or x + SMFA(x) on a [B,h,w,c] 16-bit NHWC device tensor (one fac_smfa call)."""
    lib = _lib.load()
    B, h, w, c = x.shape
    if scratch is None:
        scratch = torch.empty(max(lib.fac_smfa_scratch_bytes(B, h, w, c), 16), dtype=torch.uint8, device=x.device)
    out = torch.empty_like(x)
    _lib.check(lib.fac_smfa(_lib.DTYPES[dtype], x.data_ptr(), B, h, w, c, wpk.data_ptr(), int(residual),
                            out.data_ptr(), gate_out.data_ptr() if gate_out is not None else None,
                            scratch.data_ptr(), torch.cuda.current_stream(x.device).cuda_stream), None, "fac_smfa")
    return out


OtherCViT = VariantCViT      # the model/other/ classes have no body of their own


def other_class(name: str) -> type:
    """The drop-in class of reference file ``model/other/<name>.py`` (its ``CViT``)."""
    if name not in OTHER_VARIANTS:
        raise KeyError(f"unknown model/other CViT {name!r}; known: {', '.join(OTHER_NAMES)}")
    return variant_class(name)


def CViT(name: str, *args, **kwargs) -> VariantCViT:
    """``other_class(name)(*args, **kwargs)``: the reference's constructor arguments plus ``dtype``."""
    return other_class(name)(*args, **kwargs)


__all__ = ["CViT", "OTHER_NAMES", "OTHER_VARIANTS", "OtherCViT", "SMFA_DIM", "other_class", "smfa16", "smfa_fold",
           "smfa_pack"]
