"""Drop-ins for eight more ``CViT-main/model/cvit_*.py`` classes on gfx950 HIP kernels.

``cvit_DEConv``, ``cvit_GGCA_ADD``, ``cvit_GGCA_ADD_DEConv``,
``cvit_GGCA_ADD_RepBn`` and ``cvit_GGCA_ADD_DEConv_RepBn{,3,4,5}`` recombine
the parts of ``repbn8.CViT``; what differs is data, one ``VARIANTS`` entry each
(fac_fake_amd/weights.py, beside ``REPBN8_LAYERS`` whose format its layer lists
share):

* the conv stem: one, two or three ``nn.Sequential``s of plain convs and
  DEConvs.  Every variant keeps the CViT's channel / pool plan, so the first
  block (three convs + pool, DEConvs folded) is the fused ``fac_stem224`` kernel
  and every later conv one ``fac_conv3x3`` launch, as in repbn8.py;
* the GGCA site: none (``cvit_DEConv``), the 512x7x7 stem output, or — RepBn3 —
  the 64x56x56 map after ``features1``; and its combine, ``x * GGCA(x)`` or
  ``x + GGCA(x)``.  Both are one ``fac_ggca_apply`` call (ggca.hip: LDS-resident
  on 7x7, the streaming pool / MLP / apply path on 56x56);
* the FeedForward PreNorm: ``nn.LayerNorm`` (eps 1e-5) or LinearNorm, whose
  eval branch is LayerNorm(eps 1e-6) — the tail context's ``ffn_ln_eps_exp``;
* whether the unused top-level ``Deconv`` is in the state_dict.

Each class has the reference's constructor, ``state_dict`` (keys, shapes,
order), batch-slot ``pos_embedding`` rule and ``forward(img, mask=None)``, plus
``forward_u8`` / ``reserve`` / inference-only ``train()`` exactly as
``repbn8.CViT``; there is no CPU fallback.  ``CViT(name, ...)`` builds one by
the reference file's name, ``variant_class(name)`` gives the class (what the
``model/<name>.py`` shims export).  Grad-CAM is not implemented for these.
"""
from __future__ import annotations

import ctypes

import torch
from torch import nn

from . import _lib
from .cvit import _Node, reference_mask_poisons, weight_versions
from .ops import TORCH16, fold_bn
from .repbn8 import _BUFFERS, BN_EPS, SUPPORTED, _init_tensor, _pos_index, deconv_fold
from .weights import VARIANT_NAMES, VARIANTS, variant_param_specs

GGCA_GROUPS = 4
GGCA_OPS = {"mul": 0, "add": 1}          # fac_ggca_apply's op
FF_LN_EPS_EXP = {"layernorm": 5, "linearnorm": 6}


class VariantCViT(nn.Module):
    """One CViT variant on gfx950 (inference); subclasses set ``variant``."""

    variant: str = ""
    ggca_ops = GGCA_OPS          # table op name -> what ggca_combine16 dispatches on (other.py adds one)

    def __init__(self, image_size=224, patch_size=7, num_classes=2, channels=512, dim=1024, depth=6, heads=8,
                 mlp_dim=2048, *, dtype: str = "fp16"):
        super().__init__()
        table = self._table()
        if table is None:
            raise TypeError("build a variant with variants.CViT(name) or variants.variant_class(name)")
        cfg = dict(image_size=image_size, patch_size=patch_size, num_classes=num_classes, channels=channels, dim=dim,
                   depth=depth, heads=heads, mlp_dim=mlp_dim)
        if cfg != SUPPORTED:
            raise NotImplementedError(f"the gfx950 {self.variant} path implements {SUPPORTED}, got {cfg}")
        if dtype not in _lib.DTYPES:
            raise ValueError(f"dtype must be one of {list(_lib.DTYPES)}")
        self.dtype_name = dtype
        self.patch_size = patch_size
        self.table = table
        for name, shape, kind in self._param_specs(dim=dim, depth=depth, mlp_dim=mlp_dim, num_classes=num_classes,
                                                   channels=channels, patch_size=patch_size):
            *path, leaf = name.split(".")
            mod = self
            for p in path:
                if p not in mod._modules:
                    mod.add_module(p, _Node())
                mod = mod._modules[p]
            t = _init_tensor(shape, kind)
            if kind in _BUFFERS:
                mod.register_buffer(leaf, t)
            else:
                mod.register_parameter(leaf, nn.Parameter(t))
        self._prep = None
        self._ctx = None
        self.eval()

    # what a subclass with another stem replaces (dconv.py): the table, the
    # state_dict's layout, _prepare_stem and stem_features
    def _table(self):
        return VARIANTS.get(self.variant)

    def _param_specs(self, **kw):
        return variant_param_specs(self.variant, **kw)

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        out = super().load_state_dict(state_dict, strict=strict, assign=assign)
        self._prep = None
        return out

    def train(self, mode: bool = True):
        if mode:
            raise RuntimeError(f"the gfx950 {self.variant} path is inference-only (DEConv and BatchNorm are folded)")
        return super().train(False)

    def _release(self):
        if self._ctx is not None:
            _lib.load().fac_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def folded_layers(self):
        """(weight, bias, relu, pool) per conv, DEConv and BatchNorm folded in fp32."""
        sd = self.state_dict()
        out = []
        for seq, idx, kind, _ci, _co, bn, relu, pl in self.table["layers"]:
            p = f"{seq}.{idx}"
            w, b = (sd[p + ".weight"], sd[p + ".bias"]) if kind == "conv" else deconv_fold(sd, p)
            if bn is not None:
                q = f"{seq}.{bn}"
                w, b = fold_bn(w, b, sd[q + ".weight"], sd[q + ".bias"], sd[q + ".running_mean"],
                               sd[q + ".running_var"], BN_EPS)
            else:
                w, b = fold_bn(w, b, None, None, None, None, BN_EPS)
            out.append((w, b, relu, pl))
        return out

    def _prepare(self, device: torch.device):
        idx = device.index if device.index is not None else torch.cuda.current_device()
        v = weight_versions(self)
        if self._prep == (idx, v):
            return
        sd = self.state_dict()
        self._prepare_stem(sd, device)
        self._zero = torch.zeros(128, dtype=torch.int16, device=device)   # zero-padding source page
        self._prepare_ggca(sd, device, self._ggca_after())
        self._prepare_tail(sd, idx)
        self._prep = (idx, v)

    def _packed_conv(self, w, H, device):
        """fac_conv3x3_pack of a folded fp32 weight [co][ci][3][3] (H = 0: the fused block's conv 3->32)."""
        dt = self.dtype_name
        lib = _lib.load()
        dti = _lib.DTYPES[dt]
        co, ci = w.shape[:2]
        wf = w.reshape(co, ci, 9).contiguous()
        if H == 0:
            out = torch.empty(32 * 64, dtype=torch.int16)
            _lib.check(lib.fac_stem224_pack_conv1(dti, wf.data_ptr(), out.data_ptr()), None, "pack_conv1")
        else:
            n = lib.fac_conv3x3_packed_elems(H, ci, co)
            if n == 0:
                raise ValueError(f"conv {ci}->{co} at {H}x{H} is not a fac_conv3x3 shape")
            out = torch.empty(n, dtype=torch.int16)
            _lib.check(lib.fac_conv3x3_pack(dti, H, ci, co, wf.data_ptr(), out.data_ptr()), None, "pack_conv3x3")
        return out.view(TORCH16[dt]).to(device)

    def _prepare_stem(self, sd, device):
        """The fused first block's operands (self._stem) and one entry per later conv (self._layers)."""
        layers, H = [], 224
        for i, (w, b, relu, pl) in enumerate(self.folded_layers()):
            co, ci = w.shape[:2]
            layers.append((self._packed_conv(w, 0 if i == 0 else H, device), b.to(device), H, ci, co, pl, relu))
            if pl:
                H //= 2
        (w1, b1, *_), (w2, b2, *_), (w3, b3, *_) = layers[:3]
        self._stem = (w1, b1, w2, b2, w3, b3)
        self._layers = layers[3:]

    def _ggca_after(self):
        """After how many of self._layers the GGCA combine runs (None: no GGCA)."""
        if self.table["ggca"] is None:
            return None
        site = self.table["ggca"][0]
        seqs = [l[0] for l in self.table["layers"]]
        after = len(seqs) if site == "stem" else max(i for i, s in enumerate(seqs) if s == site) + 1
        return after - 3

    def _prepare_ggca(self, sd, device, after):
        """self._ggca: the site (index into self._layers), its shape, op and device weights."""
        self._ggca = None
        if self.table["ggca"] is not None:
            _site, chw, op = self.table["ggca"]
            g = "ggca.shared_conv."
            f32 = lambda t: t.detach().to(device=device, dtype=torch.float32).contiguous()  # noqa: E731
            cr, cg = sd[g + "0.weight"].shape[:2]
            self._ggca = (after, chw, self.ggca_ops[op],
                          (f32(sd[g + "0.weight"].reshape(cr, cg)), f32(sd[g + "0.bias"]),
                           f32(torch.stack([sd[g + "1.running_mean"], sd[g + "1.running_var"], sd[g + "1.weight"],
                                            sd[g + "1.bias"]])),
                           f32(sd[g + "3.weight"].reshape(cg, cr)), f32(sd[g + "3.bias"])))

    def _prepare_tail(self, sd, idx):
        """The CViT tail (embedding .. head) on a context without a conv stem."""
        lib = _lib.load()
        self._release()
        h = ctypes.c_void_p()
        _lib.check(lib.fac_create(idx, _lib.DTYPES[self.dtype_name], ctypes.byref(h)), None, "fac_create")
        self._ctx = h
        _lib.check(lib.fac_set_option(h, b"tail_only", 1), h, "fac_set_option")
        _lib.check(lib.fac_set_option(h, b"ffn_ln_eps_exp", FF_LN_EPS_EXP[self.table["ff_norm"]]), h,
                   "fac_set_option")
        tail = {}
        for k, t in sd.items():
            if k in ("pos_embedding", "cls_token") or k.startswith("patch_to_embedding.") or \
                    k.startswith("mlp_head."):
                tail[k] = t
            elif k.startswith("transformer."):
                if ".1.fn.norm.norm1." in k:          # LinearNorm's eval branch
                    tail[k.replace(".norm.norm1.", ".norm.")] = t
                elif ".1.fn.norm." not in k or self.table["ff_norm"] == "layernorm":
                    tail[k] = t
        keep, descs = [], []
        for k, t in tail.items():
            hst = t.detach().to("cpu", torch.float32).contiguous()
            keep.append(hst)
            d = _lib.TensorDesc()
            d.name, d.data, d.ndim = k.encode(), hst.data_ptr(), hst.dim()
            for i, s in enumerate(hst.shape):
                d.shape[i] = s
            descs.append(d)
        arr = (_lib.TensorDesc * len(descs))(*descs)
        _lib.check(lib.fac_load_weights(h, ctypes.cast(arr, ctypes.c_void_p), len(descs)), h, "fac_load_weights")

    def reserve(self, max_batch: int, device=None):
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._prepare(dev)
        _lib.check(_lib.load().fac_reserve(self._ctx, int(max_batch)), self._ctx, "fac_reserve")

    # ------------------------------------------------------------------ forward
    def ggca_combine16(self, f: torch.Tensor) -> torch.Tensor:
        """x * GGCA(x) or x + GGCA(x), the variant's, on [B,H,W,C] 16-bit NHWC."""
        _after, (C, H, W), op, (w1, b1, bn4, w2, b2) = self._ggca
        if tuple(f.shape[1:]) != (H, W, C):
            raise ValueError(f"expected features [B,{H},{W},{C}], got {tuple(f.shape)}")
        out = torch.empty_like(f)
        _lib.check(_lib.load().fac_ggca_apply(_lib.DTYPES[self.dtype_name], f.data_ptr(), f.shape[0], H, W, C,
                                              GGCA_GROUPS, w1.data_ptr(), b1.data_ptr(), bn4.data_ptr(),
                                              w2.data_ptr(), b2.data_ptr(), op, out.data_ptr(),
                                              torch.cuda.current_stream(f.device).cuda_stream), None, "fac_ggca_apply")
        return out

    def stem_features(self, src: torch.Tensor, u8: bool, upto=None) -> torch.Tensor:
        """The conv stem with the GGCA combine at its site -> [B,7,7,512] 16-bit
        NHWC.  src: uint8 NHWC crops (u8) or normalised fp32 NCHW images.
        upto="ggca": stop right after the combine (RepBn3: the [B,56,56,64] map)."""
        lib = _lib.load()
        dti = _lib.DTYPES[self.dtype_name]
        B, dev = src.shape[0], src.device
        st = torch.cuda.current_stream(dev).cuda_stream
        x = torch.empty(B, 112, 112, 32, dtype=TORCH16[self.dtype_name], device=dev)
        w1, b1, w2, b2, w3, b3 = self._stem
        _lib.check(lib.fac_stem224(dti, int(u8), src.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                                   b2.data_ptr(), w3.data_ptr(), b3.data_ptr(), x.data_ptr(), B, st), None,
                   "fac_stem224")
        site = self._ggca[0] if self._ggca is not None else None
        for i, (wpk, b, H, ci, co, pl, relu) in enumerate(self._layers):
            Ho = H // 2 if pl else H
            y = torch.empty(B, Ho, Ho, co, dtype=x.dtype, device=dev)
            _lib.check(lib.fac_conv3x3(dti, x.data_ptr(), wpk.data_ptr(), b.data_ptr(), y.data_ptr(), B, H, ci, co,
                                       int(pl), int(relu), self._zero.data_ptr(), st), None, "fac_conv3x3")
            x = y
            if site == i + 1:
                x = self.ggca_combine16(x)
                if upto == "ggca":
                    return x
        return x

    def _run(self, src: torch.Tensor, u8: bool, pos_index, want_probs: bool):
        B = src.shape[0]
        dev = src.device
        pidx = _pos_index(B, pos_index, dev)
        f = self.stem_features(src, u8)
        logits = torch.empty(B, SUPPORTED["num_classes"], dtype=torch.float32, device=dev)
        probs = torch.empty_like(logits) if want_probs else None
        _lib.check(_lib.load().fac_forward_features(self._ctx, f.data_ptr(), B, pidx.data_ptr(), None,
                                                    logits.data_ptr(), probs.data_ptr() if want_probs else None,
                                                    torch.cuda.current_stream(dev).cuda_stream), self._ctx,
                   "fac_forward_features")
        return logits, probs

    def forward(self, img: torch.Tensor, mask=None, pos_index=None) -> torch.Tensor:
        poison = mask is not None and reference_mask_poisons(mask, img.shape[0])
        if not img.is_cuda:
            raise RuntimeError(f"CViT {self.variant} (gfx950 HIP path) needs its input on a GPU device; there is no "
                               "CPU fallback")
        if img.dim() != 4 or tuple(img.shape[1:]) != (3, 224, 224):
            raise ValueError(f"expected img [B,3,224,224], got {tuple(img.shape)}")
        self._prepare(img.device)
        logits = self._run(img.float().contiguous(), False, pos_index, False)[0]
        return logits.fill_(float("nan")) if poison else logits

    def forward_u8(self, crops: torch.Tensor, pos_index=None, return_probs: bool = False):
        """uint8 NHWC RGB crops [B,224,224,3]; x/255 + Normalize fused into the first conv block."""
        if crops.dtype != torch.uint8 or crops.dim() != 4 or tuple(crops.shape[1:]) != (224, 224, 3):
            raise ValueError(f"expected uint8 crops [B,224,224,3], got {crops.dtype} {tuple(crops.shape)}")
        if not crops.is_cuda:
            raise RuntimeError(f"CViT {self.variant} (gfx950 HIP path) needs its input on a GPU device; there is no "
                               "CPU fallback")
        self._prepare(crops.device)
        logits, probs = self._run(crops.contiguous(), True, pos_index, return_probs)
        return (logits, probs) if return_probs else logits


_CLASSES: dict = {}


def variant_class(name: str) -> type:
    """The drop-in class of reference file ``model/<name>.py`` (its ``CViT``)."""
    if name not in VARIANTS:
        raise KeyError(f"unknown CViT variant {name!r}; known: {', '.join(VARIANT_NAMES)}")
    if name not in _CLASSES:
        _CLASSES[name] = type("CViT", (VariantCViT,), {"variant": name, "__module__": __name__,
                                                       "__qualname__": f"CViT[{name}]",
                                                       "__doc__": f"{name}.CViT on gfx950 (inference)."})
    return _CLASSES[name]


def CViT(name: str, *args, **kwargs) -> VariantCViT:
    """``variant_class(name)(*args, **kwargs)``: the reference's constructor arguments plus ``dtype``."""
    return variant_class(name)(*args, **kwargs)


__all__ = ["CViT", "VARIANTS", "VARIANT_NAMES", "VariantCViT", "variant_class"]
