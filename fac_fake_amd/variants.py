"""Drop-ins for fourteen ``CViT-main/model/**/cvit_*.py`` classes on gfx950 HIP kernels.

RepBn8, the eight of ``weights.VARIANTS``, ``cvit_GGCA_ADD_DConv`` and the four
of ``weights.OTHER_VARIANTS`` keep the CViT's channel / pool plan, the single
7x7 patch, the 2-token tail and the batch-slot ``pos_embedding`` rule; what
differs is data, one ``weights.CVIT_FAMILY`` entry each (its format is described
there).  ``VariantCViT`` is the one class body for all of them:

* the conv stem is compiled from the entry into a flat list of launches
  (``stem_plan``, a function of the entry alone; ``_prepare_stem`` adds the
  device operands) that ``stem_features`` walks:

    stem224  ``fac_stem224``, the fused first block (three convs + pool, DEConvs
             folded, the input normalisation), where the entry's first three
             layers are convs or DEConvs;
    pack32   otherwise ``fac_pack_input`` to 32 channels (zeros beyond 3, so the
             first conv's zero padding lands in normalised space; that conv's
             folded weight is zero beyond input channel 3);
    conv     ``fac_conv3x3``: every other conv, DEConvs and eval BatchNorm
             folded on the host, the 2x2 max-pool and the ReLU in its epilogue;
    idw      ``fac_idwconv``: InceptionDWConv2d -> BatchNorm -> ReLU (-> pool);
    smfa     ``fac_smfa``: x + SMFA(x), with a scratch buffer kept per model;
    bfm      BFM(x, x) = 4 (ReLU conv3 + ReLU conv5 + ReLU conv7)(x) on the route
             ``bfm.bfm_prepare`` gives (three ``fac_conv_nd`` + ``fac_ew``, or
             one ``fac_bfm``), the entries of ``weights.BFM_VARIANTS`` (bfm.py);
    mdfa     ``fac_mdfa``: MDFA(x), with a scratch buffer kept per model, the
             entries of ``weights.MDFA_VARIANTS`` (mdfa.py);
    scconv   ``fac_scconv``: ScConv -> BatchNorm -> ReLU (-> pool), with one
             scratch buffer kept per model for its sites, the entries of
             ``weights.SCCONV_VARIANTS`` (scconv.py);
    odconv   ``fac_odconv``: ODConv2d -> BatchNorm -> ReLU (-> pool) in place of a
             conv, or the bare block after a sequential, with one scratch buffer
             kept per model for its sites, the entries of
             ``weights.ODCONV_VARIANTS`` (odconv.py);
    wt       ``fac_wtconv``: WTConv2d -> BatchNorm -> ReLU (-> pool) in one
             launch with no scratch, the entries of ``weights.WTCONV_VARIANTS``
             (wtconv.py);
    ggca     ``fac_ggca_apply`` (x * GGCA(x), x + GGCA(x)) or ``fac_ggca_scale``
             (GGCA(x)) at the entry's site;

* the tail (embedding .. head) is ``fac_forward_features`` on a "tail_only"
  context, the FeedForward PreNorm ``nn.LayerNorm`` (eps 1e-5) or LinearNorm,
  whose eval branch is LayerNorm(eps 1e-6) — the context's ``ffn_ln_eps_exp``.

Each class has the reference's constructor, ``state_dict`` (keys, shapes,
order) and ``forward(img, mask=None)``, plus ``forward_u8`` / ``reserve`` and an
inference-only ``train()``; there is no CPU fallback.  The whole forward is
stream-ordered on the current torch stream and can be captured into a hipGraph.
``variant_class(name)`` gives the class the ``model/<name>.py`` shims export;
``CViT(name, ...)`` builds one of the eight ``VARIANTS``.  Grad-CAM exists for
RepBn8 only (repbn8.py).

To add a variant: add its entry to a table in weights.py; add a step kind here
(a ``stem_plan`` line, its operands in ``_prepare_stem``, a ``_step_<kind>``
method) only if it brings a new kernel.
"""
from __future__ import annotations

import ctypes
import importlib
from collections import namedtuple

import torch
from torch import nn

from . import _lib
from .cvit import MAX_SLOTS, _Node, reference_mask_poisons, weight_versions
from .ops import TORCH16, fold_bn, pack_input
from .weights import (BFM_VARIANTS, CVIT_FAMILY, MDFA_VARIANTS, ODCONV_VARIANTS, REPBN8_NAME, SCCONV_VARIANTS,
                      VARIANT_NAMES, VARIANTS, WTCONV_VARIANTS, family_entry, param_specs)

SUPPORTED = dict(image_size=224, patch_size=7, num_classes=2, channels=512, dim=1024, depth=6, heads=8,
                 mlp_dim=2048)
BN_EPS = 1e-5
MEAN = (0.485, 0.456, 0.406)     # cvit_prediction.py:41
STD = (0.229, 0.224, 0.225)      # cvit_prediction.py:42
GGCA_GROUPS = 4
GGCA_OPS = {"mul": 0, "add": 1, "att": 2}    # fac_ggca_apply's op; 2: fac_ggca_scale
GGCA_ATT = GGCA_OPS["att"]
FF_LN_EPS_EXP = {"layernorm": 5, "linearnorm": 6}
_BUFFERS = ("rmean", "rvar", "nbt", "warm", "step")


def deconv_fold(sd, p: str):
    """DEConv.forward's effective 3x3 weight and bias (cvit_GGCA_ADD_DEConv_RepBn8.py:329-338):
    the sum of Conv2d_cd (:221-228), Conv2d_hd (:292-297), Conv2d_vd (:310-315),
    Conv2d_ad with theta 1 (:242-246) and the plain conv1_5, evaluated with
    the reference's tensor ops in its order, in fp32 on the CPU."""
    f = lambda k: sd[f"{p}.{k}"].detach().to("cpu", torch.float32)  # noqa: E731
    w1 = f("conv1_1.conv.weight")
    o, i = w1.shape[:2]
    t = w1.reshape(o, i, 9)
    cd = torch.zeros(o, i, 9)
    cd[:, :, :] = t[:, :, :]
    cd[:, :, 4] = t[:, :, 4] - t[:, :, :].sum(2)
    h = f("conv1_2.conv.weight")
    hd = torch.zeros(o, i, 9)
    hd[:, :, [0, 3, 6]] = h[:, :, :]
    hd[:, :, [2, 5, 8]] = -h[:, :, :]
    v = f("conv1_3.conv.weight")
    vd = torch.zeros(o, i, 9)
    vd[:, :, [0, 1, 2]] = v[:, :, :]
    vd[:, :, [6, 7, 8]] = -v[:, :, :]
    a = f("conv1_4.conv.weight").reshape(o, i, 9)
    ad = a - 1.0 * a[:, :, [3, 0, 1, 6, 4, 2, 7, 8, 5]]
    w = (cd.reshape(o, i, 3, 3) + hd.reshape(o, i, 3, 3) + vd.reshape(o, i, 3, 3) + ad.reshape(o, i, 3, 3)
         + f("conv1_5.weight"))
    b = f("conv1_1.conv.bias") + f("conv1_2.conv.bias") + f("conv1_3.conv.bias") + f("conv1_4.conv.bias") + \
        f("conv1_5.bias")
    return w, b


def _init_tensor(shape, kind):
    if kind in ("nbt", "warm"):
        return torch.zeros((), dtype=torch.long)
    if kind == "step":
        return torch.tensor(300000)
    if kind in ("rmean", "beta", "lbias", "cbias", "od_arm", "od_rmean"):
        return torch.zeros(shape)
    if kind in ("rvar", "gamma", "alpha", "od_arv", "od_rvar"):
        return torch.ones(shape)
    if kind == "emb":
        return torch.randn(shape)
    t = torch.empty(shape)
    fan_in = 1
    for s in shape[1:]:
        fan_in *= s
    return t.uniform_(-1.0 / fan_in ** 0.5, 1.0 / fan_in ** 0.5)


def _pos_index(B: int, pos_index, device) -> torch.Tensor:
    if pos_index is None:
        if B > MAX_SLOTS:   # `x += self.pos_embedding[0:shape]` raises past 32
            raise RuntimeError(f"The size of tensor a ({B}) must match the size of tensor b ({MAX_SLOTS}) "
                               f"at non-singleton dimension 0")
        return torch.arange(B, dtype=torch.int32, device=device)
    p = torch.as_tensor(pos_index)
    if p.shape != (B,):
        raise ValueError(f"pos_index must have shape ({B},), got {tuple(p.shape)}")
    if p.numel() and not torch.cuda.is_current_stream_capturing() and (int(p.min()) < 0 or int(p.max()) >= MAX_SLOTS):
        raise IndexError(f"pos_index values must lie in [0, {MAX_SLOTS})")
    return p.to(device=device, dtype=torch.int32).contiguous()


# One launch of the stem.  labels: the values of stem_features' `upto` that stop
# right after it ("after n entries of the table's layers", "features1", "smfa",
# "ggca", "bfm", "mdfa", "odconv"); H: the side of the map it runs on; ci, co: its input / output channels;
# pool, relu: fac_conv3x3's and fac_idwconv's epilogue; op: the ggca step's GGCA_OPS name.
Step = namedtuple("Step", "kind labels H ci co pool relu op", defaults=(False, False, None))


def stem_plan(entry) -> list:
    """The launches of one CVIT_FAMILY, BFM_VARIANTS, MDFA_VARIANTS, SCCONV_VARIANTS,
    ODCONV_VARIANTS or WTCONV_VARIANTS entry's conv stem, in order (kinds: the module docstring's).  The first block is the
    fused stem224 if and only if the entry's first three layers are convs or
    DEConvs.  Where several blocks follow one sequential they run smfa, ggca,
    bfm, mdfa, odconv (no reference forward has mdfa or the bare odconv beside another block at one site)."""
    layers = entry["layers"]
    seqs = [l[0] for l in layers]
    end = lambda s: len(layers) if s == "stem" else max(i for i, q in enumerate(seqs) if q == s) + 1  # noqa: E731
    ggca_at = end(entry["ggca"][0]) if entry["ggca"] is not None else None
    smfa_at = end(entry["smfa"]) if entry["smfa"] is not None else None
    bfm = entry.get("bfm")
    bfm_at = end(bfm[0]) if bfm is not None else None
    mdfa = entry.get("mdfa")
    mdfa_at = end(mdfa[0]) if mdfa is not None else None
    od = entry.get("odconv")
    od_at = end(od[0]) if od is not None else None
    f1 = end(seqs[0])
    fused = all(l[2] not in ("idw", "wt") for l in layers[:3])
    if fused:
        assert [l[3:5] + l[6:] for l in layers[:3]] == [(3, 32, True, False), (32, 32, True, False),
                                                         (32, 32, True, True)] and \
            min(f1, ggca_at or 4, smfa_at or 4, bfm_at or 4, mdfa_at or 4, od_at or 4) > 3
        plan, H, done = [Step("stem224", (3,), 224, 3, 32, True, True)], 112, 3
    else:
        plan, H, done = [Step("pack32", (), 224, 3, 32)], 224, 0
    for n, (_seq, _idx, kind, ci, co, _bn, relu, pool) in enumerate(layers[done:], done + 1):
        labels = (n, "features1") if n == f1 else (n,)
        if kind == "idw":
            plan.append(Step("idw", labels, H, co, co, pool, True))
        elif kind == "sc":
            plan.append(Step("scconv", labels, H, co, co, pool, True))
        elif kind == "od":
            plan.append(Step("odconv", labels, H, co, co, pool, relu))
        elif kind == "wt":
            plan.append(Step("wt", labels, H, co, co, pool, True))
        else:
            plan.append(Step("conv", labels, H, 32 if n == 1 else ci, co, pool, relu))
        if pool:
            H //= 2
        if n == smfa_at:
            plan.append(Step("smfa", ("smfa",), H, co, co))
        if n == ggca_at:
            C, Hg, _W = entry["ggca"][1]
            plan.append(Step("ggca", ("ggca",), Hg, C, C, op=entry["ggca"][2]))
        if n == bfm_at:
            assert co == bfm[1], (co, bfm)
            plan.append(Step("bfm", ("bfm",), H, co, co))
        if n == mdfa_at:
            assert co == mdfa[1], (co, mdfa)
            plan.append(Step("mdfa", ("mdfa",), H, co, co))
        if n == od_at:                         # the bare block: no BatchNorm, no ReLU, no pool
            assert co == od[1], (co, od)
            plan.append(Step("odconv", ("odconv",), H, co, co))
    return plan


def steps_upto(plan, upto) -> int:
    """How many steps of `plan` run for stem_features' `upto`: None all of them;
    an int n up to and including the n-th entry of the table's layers;
    "features1" the first sequential, before the block that follows it; "smfa" /
    "ggca" / "bfm" / "mdfa" / "odconv" that block.  ValueError where the plan has no such stop: an int
    inside the fused first block or past the last layer, a block the class lacks."""
    if upto is None:
        return len(plan)
    for i, s in enumerate(plan, 1):
        if upto in s.labels:
            return i
    raise ValueError(f"this stem has no stop {upto!r}; it has {[l for s in plan for l in s.labels]}")


class VariantCViT(nn.Module):
    """One CViT variant on gfx950 (inference); subclasses set ``variant``."""

    variant: str = ""

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        if cls.__dict__.get("variant"):
            _CLASSES[cls.variant] = cls

    def __init__(self, image_size=224, patch_size=7, num_classes=2, channels=512, dim=1024, depth=6, heads=8,
                 mlp_dim=2048, *, dtype: str = "fp16"):
        super().__init__()
        if not any(self.variant in table for table in (CVIT_FAMILY, BFM_VARIANTS, MDFA_VARIANTS, SCCONV_VARIANTS,
                                                           ODCONV_VARIANTS, WTCONV_VARIANTS)):
            raise TypeError("build a variant with variants.variant_class(name)")
        cfg = dict(image_size=image_size, patch_size=patch_size, num_classes=num_classes, channels=channels, dim=dim,
                   depth=depth, heads=heads, mlp_dim=mlp_dim)
        if cfg != SUPPORTED:
            raise NotImplementedError(f"the gfx950 {self.variant} path implements {SUPPORTED}, got {cfg}")
        if dtype not in _lib.DTYPES:
            raise ValueError(f"dtype must be one of {list(_lib.DTYPES)}")
        self.dtype_name = dtype
        self.patch_size = patch_size
        self.table = family_entry(self.variant)
        for name, shape, kind in param_specs(self.table, dim=dim, depth=depth, mlp_dim=mlp_dim,
                                             num_classes=num_classes, channels=channels, patch_size=patch_size):
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
        self._smfa_scratch = None          # fac_smfa's scratch, see _scratch_for
        self._smfa_outgrown = []
        self._mdfa_scratch = None          # fac_mdfa's, the same rule
        self._mdfa_outgrown = []
        self._scconv_scratch = None        # fac_scconv's, one buffer for all its sites, the same rule
        self._scconv_outgrown = []
        self._odconv_scratch = None        # fac_odconv's, the same rule
        self._odconv_outgrown = []
        self.eval()

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        for seq, idx, kind, *_ in self.table["layers"]:
            g = state_dict.get(f"{seq}.{idx}.SRU.gn.weight") if kind == "sc" else None
            if g is not None:             # ScConv divides by sum(gamma)
                tot = float(torch.as_tensor(g).detach().float().sum())
                if tot == 0.0 or tot != tot or tot in (float("inf"), float("-inf")):
                    raise ValueError(f"{seq}.{idx}.SRU.gn.weight sums to {tot}: ScConv divides by it")
            if kind == "wt":              # wt_levels 1 only: a deeper WTConv2d's keys are refused, not ignored
                deeper = [k for k in state_dict if k.startswith(f"{seq}.{idx}.wavelet_convs.") and
                          not k.startswith(f"{seq}.{idx}.wavelet_convs.0.")]
                if deeper:
                    raise ValueError(f"{seq}.{idx} has more than one wavelet level ({deeper[0]}); the gfx950 WTConv2d "
                                     "implements wt_levels=1")
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

    def _fold(self, sd):
        """Per table layer its operands in fp32 on the host: (weight, bias) with
        the DEConv and the BatchNorm folded, dconv.idw_fold's five,
        scconv.scconv_fold's dict, odconv.odconv_fold's dict or wtconv.wt_fold's dict."""
        from .dconv import idw_fold
        from .odconv import odconv_fold
        from .scconv import scconv_fold
        from .wtconv import wt_fold
        for seq, idx, kind, _ci, _co, bn, _relu, _pool in self.table["layers"]:
            p, q = f"{seq}.{idx}", f"{seq}.{bn}"
            if kind == "idw":
                yield idw_fold(sd, p, q)
                continue
            if kind == "sc":
                yield scconv_fold(sd, p, q)
                continue
            if kind == "od":
                yield odconv_fold(sd, p, q)
                continue
            if kind == "wt":
                yield wt_fold(sd, p, q)
                continue
            w, b = (sd[p + ".weight"], sd[p + ".bias"]) if kind == "conv" else deconv_fold(sd, p)
            if bn is not None:
                yield fold_bn(w, b, sd[q + ".weight"], sd[q + ".bias"], sd[q + ".running_mean"],
                              sd[q + ".running_var"], BN_EPS)
            else:
                yield fold_bn(w, b, None, None, None, None, BN_EPS)

    def folded_layers(self):
        """(weight, bias, relu, pool) per conv; for a table with InceptionDWConv2d
        layers, ("conv", weight, bias, pool) or ("idw", w_hw, w_w, w_h, scale, shift, pool); for one with
        ScConv layers, ("conv", weight, bias, pool) or ("sc", scconv_fold's dict, pool); for one with
        ODConv layers, ("conv", weight, bias, pool) or ("od", odconv_fold's dict, pool); for one with
        WTConv layers, ("conv", weight, bias, pool) or ("wt", wt_fold's dict, pool)."""
        layers = self.table["layers"]
        ops = self._fold(self.state_dict())
        if any(l[2] == "wt" for l in layers):
            return [("wt", o, l[7]) if l[2] == "wt" else ("conv", *o, l[7]) for l, o in zip(layers, ops)]
        if any(l[2] == "od" for l in layers):
            return [("od", o, l[7]) if l[2] == "od" else ("conv", *o, l[7]) for l, o in zip(layers, ops)]
        if any(l[2] == "sc" for l in layers):
            return [("sc", o, l[7]) if l[2] == "sc" else ("conv", *o, l[7]) for l, o in zip(layers, ops)]
        if any(l[2] == "idw" for l in layers):
            return [("idw" if l[2] == "idw" else "conv", *o, l[7]) for l, o in zip(layers, ops)]
        return [(*o, l[6], l[7]) for l, o in zip(layers, ops)]

    def _prepare(self, device: torch.device):
        idx = device.index if device.index is not None else torch.cuda.current_device()
        v = weight_versions(self)
        if self._prep == (idx, v):
            return
        sd = self.state_dict()
        self._zero = torch.zeros(128, dtype=torch.int16, device=device)   # zero-padding source page
        self._prepare_stem(sd, device)
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
        """self._steps: per stem_plan step (step, the class's _step_<kind> function,
        its device operands); self._ggca / self._smfa / self._bfm / self._mdfa: those steps' operands or None."""
        from .bfm import bfm_fold, bfm_prepare
        from .mdfa import mdfa16, mdfa_fold, mdfa_pack
        self._mdfa16 = mdfa16
        from .other import smfa16, smfa_fold, smfa_pack
        self._smfa16 = smfa16          # bound here: other.py imports this module
        from .scconv import scconv16, scconv_pack
        self._scconv16 = scconv16
        from .odconv import odconv16, odconv_fold, odconv_pack
        self._odconv16 = odconv16
        from .wtconv import wt_pack, wtconv16
        self._wtconv16 = wtconv16
        folded = list(self._fold(sd))
        f32 = lambda t: t.detach().to(device=device, dtype=torch.float32).contiguous()  # noqa: E731
        self._ggca = self._smfa = self._bfm = self._mdfa = None
        self._steps = []
        for s in stem_plan(self.table):
            if s.kind == "stem224":
                ops = tuple(t for i, (w, b) in enumerate(folded[:3])
                            for t in (self._packed_conv(w, 0 if i == 0 else 224, device), b.to(device)))
            elif s.kind == "conv":
                w, b = folded[s.labels[0] - 1]
                if w.shape[1] < s.ci:      # 3 -> 32 on the 32-channel packed input
                    w = torch.cat([w, torch.zeros(w.shape[0], s.ci - w.shape[1], 3, 3)], 1)
                ops = (self._packed_conv(w, s.H, device), b.to(device))
            elif s.kind == "idw":
                ops = tuple(t.to(device) for t in folded[s.labels[0] - 1])
            elif s.kind == "scconv":
                ops = scconv_pack(folded[s.labels[0] - 1], self.dtype_name, device)
            elif s.kind == "odconv":           # a table layer, or the bare top-level self.odconv
                ops = odconv_pack(folded[s.labels[0] - 1] if s.labels != ("odconv",) else odconv_fold(sd, "odconv"),
                                  self.dtype_name, device)
            elif s.kind == "wt":
                ops = wt_pack(folded[s.labels[0] - 1], device)
            elif s.kind == "smfa":
                ops = self._smfa = smfa_pack(smfa_fold(sd), self.dtype_name, device)
            elif s.kind == "bfm":
                ops = self._bfm = bfm_prepare(bfm_fold(sd), self.dtype_name, device)
            elif s.kind == "mdfa":
                ops = self._mdfa = mdfa_pack(mdfa_fold(sd), self.dtype_name, device)
            elif s.kind == "ggca":
                g = "ggca.shared_conv."
                cr, cg = sd[g + "0.weight"].shape[:2]
                ops = self._ggca = (f32(sd[g + "0.weight"].reshape(cr, cg)), f32(sd[g + "0.bias"]),
                                    f32(torch.stack([sd[g + "1.running_mean"], sd[g + "1.running_var"],
                                                     sd[g + "1.weight"], sd[g + "1.bias"]])),
                                    f32(sd[g + "3.weight"].reshape(cg, cr)), f32(sd[g + "3.bias"]))
            else:
                ops = ()
            self._steps.append((s, getattr(type(self), "_step_" + s.kind), ops))

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

    def _scratch_for(self, B: int, s: Step, device) -> torch.Tensor:
        """fac_smfa's scratch for B crops: one buffer per model, grown when a
        larger batch comes and otherwise reused, so that after reserve(max_batch)
        a forward of up to max_batch crops allocates none.  A buffer that was
        outgrown is kept: a graph captured with it still points at it."""
        need = _lib.load().fac_smfa_scratch_bytes(B, s.H, s.H, s.co)
        buf = self._smfa_scratch
        if buf is None or buf.numel() < need or buf.device != torch.device(device):
            if buf is not None:
                self._smfa_outgrown.append(buf)
            self._smfa_scratch = buf = torch.empty(need, dtype=torch.uint8, device=device)
        return buf

    def _mdfa_scratch_for(self, B: int, s: Step, device) -> torch.Tensor:
        """fac_mdfa's scratch for B crops, kept and grown like _scratch_for's."""
        need = _lib.load().fac_mdfa_scratch_bytes(B, s.H, s.H, s.co)
        buf = self._mdfa_scratch
        if buf is None or buf.numel() < need or buf.device != torch.device(device):
            if buf is not None:
                self._mdfa_outgrown.append(buf)
            self._mdfa_scratch = buf = torch.empty(need, dtype=torch.uint8, device=device)
        return buf

    def _site_scratch_for(self, kind: str, B: int, device) -> torch.Tensor:
        """The scratch of fac_<kind> (scconv, odconv) for B crops: one buffer
        (self._<kind>_scratch) sized for the largest of the class's sites of that
        kind (they run one after the other on one stream), kept and grown like
        _scratch_for's, the outgrown ones in self._<kind>_outgrown."""
        size = getattr(_lib.load(), f"fac_{kind}_scratch_bytes")
        need = max(size(B, s.H, s.H, s.co) for s, _run, _ops in self._steps if s.kind == kind)
        buf = getattr(self, f"_{kind}_scratch")
        if buf is None or buf.numel() < need or buf.device != torch.device(device):
            if buf is not None:
                getattr(self, f"_{kind}_outgrown").append(buf)
            buf = torch.empty(need, dtype=torch.uint8, device=device)
            setattr(self, f"_{kind}_scratch", buf)
        return buf

    def reserve(self, max_batch: int, device=None):
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._prepare(dev)
        _lib.check(_lib.load().fac_reserve(self._ctx, int(max_batch)), self._ctx, "fac_reserve")
        for s, _run, ops in self._steps:
            if s.kind == "smfa":
                self._scratch_for(int(max_batch), s, ops.device)
            elif s.kind == "mdfa":
                self._mdfa_scratch_for(int(max_batch), s, ops.device)
        for kind in ("scconv", "odconv"):
            if any(s.kind == kind for s, _run, _ops in self._steps):
                self._site_scratch_for(kind, int(max_batch), dev)

    # ------------------------------------------------------------------ the stem's launches
    # _step_<kind>(x, s, ops, u8, st) -> the step's output, a new tensor; x: the
    # map before it, for the first step the forward's input; st: the current stream
    def _step_stem224(self, src, s, ops, u8, st):
        x = torch.empty(src.shape[0], 112, 112, 32, dtype=TORCH16[self.dtype_name], device=src.device)
        _lib.check(_lib.load().fac_stem224(_lib.DTYPES[self.dtype_name], int(u8), src.data_ptr(),
                                           *[t.data_ptr() for t in ops], x.data_ptr(), src.shape[0], st), None,
                   "fac_stem224")
        return x

    def _step_pack32(self, src, s, ops, u8, st):
        norm = dict(div=255.0, mean=MEAN, std=STD) if u8 else {}
        x = pack_input(src, dtype=self.dtype_name, u8=u8, spatial=(s.H, s.H), c_pad=s.co, **norm)
        return x.view(src.shape[0], s.H, s.H, s.co)

    def _conv3x3(self, x, s, ops, pool, relu, y, st):
        wpk, b = ops
        _lib.check(_lib.load().fac_conv3x3(_lib.DTYPES[self.dtype_name], x.data_ptr(), wpk.data_ptr(), b.data_ptr(),
                                           y.data_ptr(), x.shape[0], s.H, s.ci, s.co, pool, relu,
                                           self._zero.data_ptr(), st), None, "fac_conv3x3")
        return y

    def _step_conv(self, x, s, ops, u8, st):
        Ho = s.H // 2 if s.pool else s.H
        y = torch.empty(x.shape[0], Ho, Ho, s.co, dtype=TORCH16[self.dtype_name], device=x.device)
        return self._conv3x3(x, s, ops, int(s.pool), int(s.relu), y, st)

    def _step_idw(self, x, s, ops, u8, st):
        Ho = s.H // 2 if s.pool else s.H
        y = torch.empty(x.shape[0], Ho, Ho, s.co, dtype=TORCH16[self.dtype_name], device=x.device)
        _lib.check(_lib.load().fac_idwconv(_lib.DTYPES[self.dtype_name], x.data_ptr(), y.data_ptr(), x.shape[0], s.H,
                                           s.H, s.co, *[t.data_ptr() for t in ops], int(s.pool), st), None,
                   "fac_idwconv")
        return y

    def _step_scconv(self, x, s, ops, u8, st):
        return self._scconv16(x, ops, self.dtype_name, pool=s.pool, scratch=self._site_scratch_for("scconv", x.shape[0], x.device))

    def _step_odconv(self, x, s, ops, u8, st):
        return self._odconv16(x, ops, self.dtype_name, relu=s.relu, pool=s.pool,
                              scratch=self._site_scratch_for("odconv", x.shape[0], x.device))

    def _step_wt(self, x, s, ops, u8, st):
        return self._wtconv16(x, ops, self.dtype_name, pool=s.pool)

    def _step_smfa(self, x, s, ops, u8, st):
        return self._smfa16(x, ops, self.dtype_name, residual=True,
                            scratch=self._scratch_for(x.shape[0], s, x.device))

    def _step_ggca(self, x, s, ops, u8, st):
        return self.ggca_combine16(x)

    def _step_bfm(self, x, s, ops, u8, st):
        return ops(x)

    def _step_mdfa(self, x, s, ops, u8, st):
        return self._mdfa16(x, ops, self.dtype_name, scratch=self._mdfa_scratch_for(x.shape[0], s, x.device))

    def ggca_combine16(self, f: torch.Tensor) -> torch.Tensor:
        """The class's GGCA step on [B,H,W,C] 16-bit NHWC: x * GGCA(x), x + GGCA(x) or GGCA(x)."""
        _site, (C, H, W), op = self.table["ggca"]
        if tuple(f.shape[1:]) != (H, W, C):
            raise ValueError(f"expected features [B,{H},{W},{C}], got {tuple(f.shape)}")
        out = torch.empty_like(f)
        lib = _lib.load()
        st = torch.cuda.current_stream(f.device).cuda_stream
        head = (_lib.DTYPES[self.dtype_name], f.data_ptr(), f.shape[0], H, W, C, GGCA_GROUPS,
                *[t.data_ptr() for t in self._ggca])
        if GGCA_OPS[op] == GGCA_ATT:
            _lib.check(lib.fac_ggca_scale(*head, out.data_ptr(), st), None, "fac_ggca_scale")
        else:
            _lib.check(lib.fac_ggca_apply(*head, GGCA_OPS[op], out.data_ptr(), st), None, "fac_ggca_apply")
        return out

    # ------------------------------------------------------------------ forward
    def _walk(self, x, u8: bool, steps):
        st = torch.cuda.current_stream(x.device).cuda_stream
        for s, run, ops in steps:
            x = run(self, x, s, ops, u8, st)
        return x

    def stem_features(self, src: torch.Tensor, u8: bool, upto=None) -> torch.Tensor:
        """The conv stem with the class's blocks at their sites -> [B,7,7,512]
        16-bit NHWC.  src: uint8 NHWC crops (u8) or normalised fp32 NCHW images.
        upto stops early and returns that map (steps_upto)."""
        steps = self._steps
        return self._walk(src, u8, steps[:steps_upto([s for s, _run, _ops in steps], upto)])

    def _run(self, src: torch.Tensor, u8: bool, pos_index, want_probs: bool):
        B = src.shape[0]
        dev = src.device
        pidx = _pos_index(B, pos_index, dev)
        f = self._walk(src, u8, self._steps)
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


_CLASSES: dict = {}      # variant name -> class, filled by VariantCViT.__init_subclass__
_MODULES = {REPBN8_NAME: "repbn8"}   # classes with methods of their own live in a module of theirs


def variant_class(name: str) -> type:
    """The drop-in class of reference file ``model/<name>.py`` or ``model/other/<name>.py`` (its ``CViT``)."""
    family_entry(name)       # KeyError for a name of neither table
    if name not in _CLASSES:
        if name in _MODULES:
            importlib.import_module(f"{__package__}.{_MODULES[name]}")
        else:
            type("CViT", (VariantCViT,), {"variant": name, "__module__": __name__, "__qualname__": f"CViT[{name}]",
                                          "__doc__": f"{name}.CViT on gfx950 (inference)."})
    return _CLASSES[name]


def CViT(name: str, *args, **kwargs) -> VariantCViT:
    """One of the eight ``VARIANTS``: ``variant_class(name)(*args, **kwargs)``, the reference's constructor
    arguments plus ``dtype``."""
    if name not in VARIANTS:
        raise KeyError(f"unknown CViT variant {name!r}; known: {', '.join(VARIANT_NAMES)}")
    return variant_class(name)(*args, **kwargs)


__all__ = ["CViT", "VARIANTS", "VARIANT_NAMES", "VariantCViT", "deconv_fold", "stem_plan", "steps_upto",
           "variant_class"]
