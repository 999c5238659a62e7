"""CPU reference of cvit_GGCA4_BFM5 (fac_fake_amd/bfm.py); test infrastructure,
beside smfa_ref.py and variants_ref.py, whose stem walk, GGCA and tail it reuses.

The project's own restatement of ``CViT-main/model/other/cvit_GGCA4_BFM5.py``,
functional over the state_dict, on PyTorch CPU ops:

* ``bfm_fold``         the BFM block's state_dict entries as fac_bfm_pack's
                        operands (w3, w5, w7, bias3); the tfam.* tensors do
                        not enter.
* ``bfm_block``        BFM(x, x) = scale * sum_k ReLU(conv_k(x) + b_k) the way
                        bfm.hip computes it, in float64 or fp32, optionally
                        with the kernel's single rounding point, the output,
                        or the composed route's four (the caller rounds the
                        weights and the input: they are 16-bit operands before
                        a kernel sees them).
* ``bfm_mixed_sign``   the share of output elements whose three
                        pre-activations do not all have one sign: where
                        ReLU(a) + ReLU(b) + ReLU(c) differs from ReLU(a + b + c).
* ``forward_fp32``     CViT.forward of the class, fp32.
* ``forward_emulated`` the same with 16-bit rounding exactly where the gfx950
                        path rounds (variants_ref's points plus bfm_block's
                        for MODEL_ROUTE, the route the model's step takes).

Pinned against tests/golden/bfm_golden.npz, which tools/make_golden_bfm.py
produced from the reference's own class.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.cvit_torch import BN_EPS, LN_EPS, round_to, to_torch_sd
from variants_ref import _fold, _layer_weights, _layers, _tail, ggca, ggca_combine, ggca_weights

_PLAIN = "ccc ccc ccc cccc cccc"
_LN = ("1.fn.norm", LN_EPS)
# name -> (layers, ggca (site, (C, H, W), op), bfm (site, C)); op "att": x = GGCA(x)
TABLE = {
    "cvit_GGCA4_BFM5": (_layers((4, 1), _PLAIN), ("features1", (256, 14, 14), "att"), ("stem", 512)),
}
NAMES = tuple(TABLE)
N_KEYS = {"cvit_GGCA4_BFM5": 216}
BFM_MAPS = ["pool5", "bfm"]          # the map before and after the block
BFM_SCALE = 4.0
MODEL_ROUTE = "composed"             # bfm.MODEL_ROUTE: the route the model's bfm step takes
KS = (3, 5, 7)
CONVS = ("conv1", "conv2", "conv3")  # MultiScaleFeatureExtractor's 3x3, 5x5, 7x7


def bfm_fold(sd, prefix="bfm"):
    """fac_bfm_pack's operands from the state_dict, fp32 (bfm.bfm_fold must equal this bitwise)."""
    f = lambda k: torch.as_tensor(sd[f"{prefix}.multi_scale_extractor.{k}"]).detach().float().contiguous()  # noqa: E731
    ops = {f"w{k}": f(f"{name}.weight") for name, k in zip(CONVS, KS)}
    ops["bias3"] = torch.stack([f(f"{name}.bias") for name in CONVS]).contiguous()
    return ops


def _pre(x, ops, dtype):
    """The three pre-activations conv_k(x) + b_k on NCHW x, zero padding k // 2."""
    x = x.to(dtype)
    return [F.conv2d(x, ops[f"w{k}"].to(dtype), ops["bias3"][i].to(dtype), padding=k // 2) for i, k in enumerate(KS)]


def bfm_block(x, ops, scale=BFM_SCALE, dtype=torch.float64, round=None, route="fused"):
    """bfm.hip's arithmetic on NCHW x: ((ReLU(p3) + ReLU(p5)) + ReLU(p7)) * scale.
    round: None, or "fp16" / "bf16" for the rounding points of `route` (dtype
    must then be fp32): "fused", fac_bfm's one, the output; "composed",
    bfm.ComposedBFM's four: each ReLU'd conv at its store, their sum, the
    scaled sum."""
    assert round is None or dtype == torch.float32
    assert route in ("fused", "composed")
    r = (lambda v: round_to(v, round)) if round and route == "composed" else (lambda v: v)
    p3, p5, p7 = _pre(x, ops, dtype)
    out = r(r((r(F.relu(p3)) + r(F.relu(p5))) + r(F.relu(p7))) * scale)
    return round_to(out, round) if round and route == "fused" else out


def bfm_mixed_sign(x, ops, dtype=torch.float64) -> float:
    """Share of output elements with pre-activations of mixed sign across the three convs."""
    pos = torch.stack([p > 0 for p in _pre(x, ops, dtype)]).sum(0)
    return float(((pos > 0) & (pos < 3)).double().mean())


def _site(layers, seq):
    return len(layers) if seq == "stem" else max(i for i, l in enumerate(layers) if l[0] == seq) + 1


def _forward(name, sd, img, pos_index, rnd, return_features):
    layers, g, bfm = TABLE[name]
    sd = to_torch_sd(sd)
    ggca_at, bfm_at = _site(layers, g[0]), _site(layers, bfm[0])
    r = rnd[0] if rnd else (lambda t: t)
    h = r(img.float())
    maps = {}
    for i, layer in enumerate(layers):
        if rnd is None:
            w, b = _layer_weights(sd, layer)
            h = F.conv2d(h, w, b, padding=1)
            q = f"{layer[0]}.{layer[5]}."
            h = F.batch_norm(h, sd[q + "running_mean"], sd[q + "running_var"], sd[q + "weight"], sd[q + "bias"],
                             False, 0.1, BN_EPS)
        else:
            w, b = _fold(sd, layer)
            h = F.conv2d(h, r(w), b, padding=1)
        h = F.relu(h)
        if layer[7]:
            h = F.max_pool2d(h, 2, 2)
        h = r(h)
        if layer[7]:
            maps[f"pool{len([k for k in maps if k.startswith('pool')]) + 1}"] = h
        if ggca_at == i + 1:
            gw = ggca_weights(sd)
            h = maps["ggca"] = r(ggca(gw, h) if g[2] == "att" else ggca_combine(gw, h, g[2]))
        if bfm_at == i + 1:
            ops = bfm_fold(sd)
            if rnd:
                ops = {k: (v if k == "bias3" else r(v)) for k, v in ops.items()}
            h = maps["bfm"] = bfm_block(h, ops, BFM_SCALE, dtype=torch.float32, round=rnd[1] if rnd else None,
                                        route=MODEL_ROUTE)
    lin = None if rnd is None else (lambda inp, w, b=None: F.linear(r(inp), r(w), b))
    out = _tail(sd, h, pos_index, _LN, lin=lin)
    return (out, maps) if return_features else out


@torch.no_grad()
def forward_fp32(name, sd, img, pos_index=None, return_features=False):
    """CViT.forward of model/other/<name>.py on normalised fp32 NCHW input.
    return_features: (logits, {"pool1".."pool5", "ggca", "bfm": the map})."""
    return _forward(name, sd, img, pos_index, None, return_features)


@torch.no_grad()
def forward_emulated(name, sd, img, pos_index=None, dtype="bf16", return_features=False):
    """The gfx950 path's rounding points (module doc), fp32 accumulation everywhere."""
    return _forward(name, sd, img, pos_index, (lambda t: round_to(t, dtype), dtype), return_features)
