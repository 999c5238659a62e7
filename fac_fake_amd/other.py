"""Drop-ins for four ``CViT-main/model/other/cvit_*.py`` classes on gfx950 HIP kernels.

``cvit_GGCA``, ``cvit_GGCA4``, ``cvit_GGCA_ADD3`` and ``cvit_GGCA_SMFA`` keep
the CViT's channel / pool plan, the single 7x7 patch, the 2-token tail and the
batch-slot ``pos_embedding`` rule, so they run on ``variants.VariantCViT``'s
stem walk and tail; what differs is one ``weights.OTHER_VARIANTS`` entry each:

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
from .ops import TORCH16
from .variants import GGCA_GROUPS, GGCA_OPS, VariantCViT
from .weights import OTHER_NAMES, OTHER_VARIANTS, SMFA_DIM, other_param_specs


GGCA_ATT = 2        # this module's third GGCA op: out = GGCA(x) (fac_ggca_scale)
SMFA_HW = 14        # the SMFA block's site: the 256x14x14 map after features1


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


class OtherCViT(VariantCViT):
    """One model/other/ CViT on gfx950 (inference); subclasses set ``variant``."""

    _smfa_scratch = None          # fac_smfa's scratch (cvit_GGCA_SMFA), see _scratch_for
    _smfa_outgrown: list = []

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._smfa_outgrown = []

    def _table(self):
        return OTHER_VARIANTS.get(self.variant)

    def _param_specs(self, **kw):
        return other_param_specs(self.variant, **kw)

    ggca_ops = {**GGCA_OPS, "att": GGCA_ATT}

    def ggca_combine16(self, f: torch.Tensor) -> torch.Tensor:
        """The class's GGCA step on [B,H,W,C] 16-bit NHWC: GGCA(x) (cvit_GGCA, cvit_GGCA4) or x + GGCA(x)."""
        _after, (C, H, W), op, (w1, b1, bn4, w2, b2) = self._ggca
        if op != GGCA_ATT:
            return super().ggca_combine16(f)
        if tuple(f.shape[1:]) != (H, W, C):
            raise ValueError(f"expected features [B,{H},{W},{C}], got {tuple(f.shape)}")
        out = torch.empty_like(f)
        _lib.check(_lib.load().fac_ggca_scale(_lib.DTYPES[self.dtype_name], f.data_ptr(), f.shape[0], H, W, C,
                                              GGCA_GROUPS, w1.data_ptr(), b1.data_ptr(), bn4.data_ptr(),
                                              w2.data_ptr(), b2.data_ptr(), out.data_ptr(),
                                              torch.cuda.current_stream(f.device).cuda_stream), None, "fac_ggca_scale")
        return out

    def _prepare_stem(self, sd, device):
        super()._prepare_stem(sd, device)
        self._smfa = None
        if self.table["smfa"] is not None:
            seqs = [l[0] for l in self.table["layers"]]
            after = max(i for i, s in enumerate(seqs) if s == self.table["smfa"]) + 1 - 3
            self._smfa = (after, smfa_pack(smfa_fold(sd), self.dtype_name, device))

    def _scratch_for(self, B: int, device) -> torch.Tensor:
        """fac_smfa's scratch for B crops: one buffer per model, grown when a
        larger batch comes and otherwise reused, so that after reserve(max_batch)
        a forward of up to max_batch crops allocates none.  A buffer that was
        outgrown is kept: a graph captured with it still points at it."""
        need = _lib.load().fac_smfa_scratch_bytes(B, SMFA_HW, SMFA_HW, SMFA_DIM)
        buf = self._smfa_scratch
        if buf is None or buf.numel() < need or buf.device != torch.device(device):
            if buf is not None:
                self._smfa_outgrown.append(buf)
            self._smfa_scratch = buf = torch.empty(need, dtype=torch.uint8, device=device)
        return buf

    def reserve(self, max_batch: int, device=None):
        super().reserve(max_batch, device)
        if self._smfa is not None:
            self._scratch_for(int(max_batch), self._smfa[1].device)

    def stem_features(self, src: torch.Tensor, u8: bool, upto=None) -> torch.Tensor:
        """The conv stem with the class's blocks at their sites -> [B,7,7,512]
        16-bit NHWC.  src: uint8 NHWC crops (u8) or normalised fp32 NCHW images.
        upto="features1": the [B,14,14,256] map before the block that follows
        features1 (GGCA4, GGCA_ADD3, GGCA_SMFA); upto="smfa" / "ggca": stop
        right after that combine."""
        lib = _lib.load()
        dti = _lib.DTYPES[self.dtype_name]
        B, dev = src.shape[0], src.device
        st = torch.cuda.current_stream(dev).cuda_stream
        x = torch.empty(B, 112, 112, 32, dtype=TORCH16[self.dtype_name], device=dev)
        w1, b1, w2, b2, w3, b3 = self._stem
        _lib.check(lib.fac_stem224(dti, int(u8), src.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                                   b2.data_ptr(), w3.data_ptr(), b3.data_ptr(), x.data_ptr(), B, st), None,
                   "fac_stem224")
        ggca_at = self._ggca[0] if self._ggca is not None else None
        smfa_at = self._smfa[0] if self._smfa is not None else None
        f1 = max(i for i, l in enumerate(self.table["layers"]) if l[0] in ("features1", "features")) + 1 - 3
        for i, (wpk, b, H, ci, co, pl, relu) in enumerate(self._layers):
            Ho = H // 2 if pl else H
            y = torch.empty(B, Ho, Ho, co, dtype=x.dtype, device=dev)
            _lib.check(lib.fac_conv3x3(dti, x.data_ptr(), wpk.data_ptr(), b.data_ptr(), y.data_ptr(), B, H, ci, co,
                                       int(pl), int(relu), self._zero.data_ptr(), st), None, "fac_conv3x3")
            x = y
            if upto == "features1" and f1 == i + 1:
                return x
            if smfa_at == i + 1:
                x = smfa16(x, self._smfa[1], self.dtype_name, residual=True, scratch=self._scratch_for(B, dev))
                if upto == "smfa":
                    return x
            if ggca_at == i + 1:
                x = self.ggca_combine16(x)
                if upto == "ggca":
                    return x
        return x


_CLASSES: dict = {}


def other_class(name: str) -> type:
    """The drop-in class of reference file ``model/other/<name>.py`` (its ``CViT``)."""
    if name not in OTHER_VARIANTS:
        raise KeyError(f"unknown model/other CViT {name!r}; known: {', '.join(OTHER_NAMES)}")
    if name not in _CLASSES:
        _CLASSES[name] = type("CViT", (OtherCViT,), {"variant": name, "__module__": __name__,
                                                     "__qualname__": f"CViT[{name}]",
                                                     "__doc__": f"other/{name}.CViT on gfx950 (inference)."})
    return _CLASSES[name]


def CViT(name: str, *args, **kwargs) -> OtherCViT:
    """``other_class(name)(*args, **kwargs)``: the reference's constructor arguments plus ``dtype``."""
    return other_class(name)(*args, **kwargs)


__all__ = ["CViT", "OTHER_NAMES", "OTHER_VARIANTS", "OtherCViT", "SMFA_DIM", "other_class", "smfa16", "smfa_fold",
           "smfa_pack"]
