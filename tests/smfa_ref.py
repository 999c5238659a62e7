"""CPU reference of the four model/other/ CViTs (fac_fake_amd/other.py); test
infrastructure, beside variants_ref.py whose stem walk, GGCA and tail it reuses.

The project's own restatement of ``CViT-main/model/other/cvit_GGCA{,4,_ADD3,_SMFA}.py``,
functional over the state_dict, on PyTorch CPU ops:

* ``smfa_fold``        the SMFA block's state_dict entries as fac_smfa_pack's
                        operands (Wcat = [linear_2.W | linear_2.W conv_1.W]).
* ``smfa_block``       SMFA(x) / x + SMFA(x) for 8 <= h, w <= 15 the way
                        smfa.hip computes it, in float64 or fp32, optionally
                        with the kernel's 16-bit rounding points: the weights
                        W0, Wpw, Wcat; t = linear_0(x); the depthwise operand;
                        the GELU map h; the x * g operand; the output.  The
                        statistics (max, unbiased variance) are taken from the
                        rounded x half of t; the gate path is never rounded.
* ``forward_fp32``     CViT.forward of one of the four classes, fp32.
* ``forward_emulated`` the same with 16-bit rounding exactly where the gfx950
                        path rounds (variants_ref's points plus smfa_block's).

Pinned against tests/golden/other_golden.npz, which tools/make_golden_other.py
produced from the reference's own classes.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.cvit_torch import BN_EPS, LN_EPS, round_to, to_torch_sd
from variants_ref import _fold, _layer_weights, _layers, _tail, ggca, ggca_combine, ggca_weights

_PLAIN = "ccc ccc ccc cccc cccc"
_LN = ("1.fn.norm", LN_EPS)
# name -> (layers, ggca (site, (C, H, W), op), the sequential x + SMFA(x) follows | None); op "att": x = GGCA(x)
TABLE = {
    "cvit_GGCA": (_layers((5,), _PLAIN), ("stem", (512, 7, 7), "att"), None),
    "cvit_GGCA4": (_layers((4, 1), _PLAIN), ("features1", (256, 14, 14), "att"), None),
    "cvit_GGCA_ADD3": (_layers((4, 1), _PLAIN), ("features1", (256, 14, 14), "add"), None),
    "cvit_GGCA_SMFA": (_layers((4, 1), _PLAIN), ("stem", (512, 7, 7), "add"), "features1"),
}
NAMES = tuple(TABLE)
N_KEYS = {"cvit_GGCA": 202, "cvit_GGCA4": 202, "cvit_GGCA_ADD3": 202, "cvit_GGCA_SMFA": 218}
SMFA_MAPS = ["pool4", "smfa", "pool5", "ggca"]


def smfa_fold(sd, prefix="smfa"):
    """fac_smfa_pack's operands from the state_dict, fp32 (other.smfa_fold must equal this bitwise)."""
    f = lambda k: torch.as_tensor(sd[f"{prefix}.{k}"]).detach().float()  # noqa: E731
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


def _gelu(v):
    return F.gelu(v)       # approximate='none': the exact erf form, as nn.GELU()


def smfa_block(x, ops, residual, dtype=torch.float64, round=None, return_gate=False):
    """smfa.hip's arithmetic on NCHW x with 8 <= h, w <= 15.  round: None, or
    "fp16" / "bf16" for the kernel's rounding points (dtype must then be fp32)."""
    N, c, H, W = x.shape
    assert 8 <= H <= 15 and 8 <= W <= 15, "SMFA's pooled map is 1x1 only for 8..15"
    assert round is None or dtype == torch.float32
    r = (lambda v: round_to(v, round)) if round else (lambda v: v)
    o = {k: v.to(dtype) for k, v in ops.items()}
    x = x.to(dtype)
    pw = lambda v, w, b: F.conv2d(v, w.view(*w.shape, 1, 1), b)  # noqa: E731
    t = r(pw(x, r(o["w0"]), o["b0"]))
    y, xx = t[:, :c], t[:, c:]
    alpha, cw, cb, belt = o["gate4"]
    u = alpha * (cw * xx.amax(dim=(2, 3)) + cb) + belt * xx.var(dim=(2, 3), unbiased=True)
    g = _gelu(u @ o["w1"].t() + o["b1"])                                            # [N, c], never rounded
    d = r(F.conv2d(y, o["dww"].view(2 * c, 1, 3, 3), o["dwb"], padding=1, groups=c))
    h = r(_gelu(pw(d, r(o["wpw"]), o["bpw"])))
    out = pw(torch.cat([r(xx * g.view(N, c, 1, 1)), h], 1), r(o["wcat"]), o["bcat"])
    out = r(out + x if residual else out)
    return (out, g) if return_gate else out


def smfa_unfolded(x, sd, prefix="smfa", dtype=torch.float64):
    """SMFA(x) with linear_2 and conv_1 as two convs (no Wcat fold), for the fold's own test."""
    f = lambda k: torch.as_tensor(sd[f"{prefix}.{k}"]).to(dtype)  # noqa: E731
    N, c, H, W = x.shape
    x = x.to(dtype)
    y, xx = F.conv2d(x, f("linear_0.weight"), f("linear_0.bias")).chunk(2, dim=1)
    u = f("alpha").view(1, c) * (f("dw_conv.weight")[:, 0, 1, 1] * xx.amax(dim=(2, 3)) + f("dw_conv.bias")) + \
        f("belt").view(1, c) * xx.var(dim=(2, 3), unbiased=True)
    g = _gelu(u @ f("linear_1.weight").view(c, c).t() + f("linear_1.bias"))
    d = F.conv2d(y, f("lde.conv_0.0.weight"), f("lde.conv_0.0.bias"), padding=1, groups=c)
    h = _gelu(F.conv2d(d, f("lde.conv_0.1.weight"), f("lde.conv_0.1.bias")))
    y_d = F.conv2d(h, f("lde.conv_1.weight"), f("lde.conv_1.bias"))
    return F.conv2d(xx * g.view(N, c, 1, 1) + y_d, f("linear_2.weight"), f("linear_2.bias"))


def _site(layers, seq):
    return len(layers) if seq == "stem" else max(i for i, l in enumerate(layers) if l[0] == seq) + 1


def _forward(name, sd, img, pos_index, rnd, return_features):
    layers, g, smfa = TABLE[name]
    sd = to_torch_sd(sd)
    ggca_at = _site(layers, g[0])
    smfa_at = None if smfa is None else _site(layers, smfa)
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
        if smfa_at == i + 1:
            h = maps["smfa"] = smfa_block(h, smfa_fold(sd), True, dtype=torch.float32, round=rnd[1] if rnd else None)
        if ggca_at == i + 1:
            gw = ggca_weights(sd)
            h = maps["ggca"] = r(ggca(gw, h) if g[2] == "att" else ggca_combine(gw, h, g[2]))
    lin = None if rnd is None else (lambda inp, w, b=None: F.linear(r(inp), r(w), b))
    out = _tail(sd, h, pos_index, _LN, lin=lin)
    return (out, maps) if return_features else out


@torch.no_grad()
def forward_fp32(name, sd, img, pos_index=None, return_features=False):
    """CViT.forward of model/other/<name>.py on normalised fp32 NCHW input.
    return_features: (logits, {"pool1".."pool5", "ggca", and for cvit_GGCA_SMFA "smfa": the map})."""
    return _forward(name, sd, img, pos_index, None, return_features)


@torch.no_grad()
def forward_emulated(name, sd, img, pos_index=None, dtype="bf16", return_features=False):
    """The gfx950 path's rounding points (module doc), fp32 accumulation everywhere."""
    return _forward(name, sd, img, pos_index, (lambda t: round_to(t, dtype), dtype), return_features)
