"""CPU reference of the eight CViT variants of fac_fake_amd/variants.py
(test infrastructure; oracle/ is frozen, so it lives here as ca_s3d_ref.py does).

Table-driven over its own restatement of the variant table (checked against
``fac_fake_amd.weights.VARIANTS`` in test_variants.py), functional over the
state_dict, with the PyTorch CPU ops the reference classes call:

* ``ggca``             GGCA.forward (cvit_GGCA_ADD*.py :144-207 / :12-75) for any
                        (C, H, W): returns x * att_h * att_w.
* ``ggca_combine``     the caller's ``x * ggca(x)`` or ``x + ggca(x)``.
* ``forward_fp32``     CViT.forward of variant ``name``, fp32.
* ``forward_emulated`` the same with operands rounded to 16 bits where the
                        gfx950 path rounds them: the normalised input, the folded
                        conv weights, every conv output, the GGCA combine's
                        output, the tail's weight matrices and GEMM inputs.

Pinned against tests/golden/variants_golden.npz, produced from the reference's
own class code (tools/make_golden_variants.py).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.cvit_torch import BN_EPS, LN_EPS, _pos_rows, _transformer, round_to, to_torch_sd
from oracle.repbn8_torch import FF_LN_EPS, deconv_fold

GROUPS = 4


def _layers(split, kinds, bare26=False):
    """(seq, idx, kind, cin, cout, bn, relu, pool) per conv; see weights._variant_layers."""
    kinds = kinds.replace(" ", "")
    blocks = [(3, 32, 3), (32, 64, 3), (64, 128, 4 if bare26 else 3), (128, 256, 4), (256, 512, 4)]
    names = ["features"] if len(split) == 1 else [f"features{i + 1}" for i in range(len(split))]
    seq_of = [n for n, cnt in zip(names, split) for _ in range(cnt)]
    out, k, idx, prev = [], 0, 0, None
    for bi, (cin, cout, convs) in enumerate(blocks):
        if seq_of[bi] != prev:
            idx, prev = 0, seq_of[bi]
        for li in range(convs):
            kind = "conv" if kinds[k] == "c" else "deconv"
            k += 1
            ci, last = (cin if li == 0 else cout), li == convs - 1
            if bare26 and bi == 2 and li >= 2:      # Conv2d alone, then DEConv + ReLU (no BatchNorm)
                out.append((prev, idx, kind, ci, cout, None, li == 3, last))
                idx += 1 if li == 2 else 2
            else:
                out.append((prev, idx, kind, ci, cout, idx + 1, True, last))
                idx += 3
        idx += 1
    return out


_R8, _PLAIN, _MIXED = "cdd cdd cdcd cddd cddd", "ccc ccc ccc cccc cccc", "ccd cdc cdc cddc cccc"
# name -> (layers, ggca (site, (C, H, W), op) | None, FeedForward PreNorm (state_dict path, eps))
_LN, _LIN = ("1.fn.norm", LN_EPS), ("1.fn.norm.norm1", FF_LN_EPS)
TABLE = {
    "cvit_DEConv": (_layers((4, 1), _R8, True), None, _LIN),
    "cvit_GGCA_ADD": (_layers((5,), _PLAIN), ("stem", (512, 7, 7), "mul"), _LN),
    "cvit_GGCA_ADD_DEConv": (_layers((4, 1), _R8, True), ("stem", (512, 7, 7), "mul"), _LN),
    "cvit_GGCA_ADD_RepBn": (_layers((5,), _PLAIN), ("stem", (512, 7, 7), "add"), _LIN),
    "cvit_GGCA_ADD_DEConv_RepBn": (_layers((4, 1), _MIXED), ("stem", (512, 7, 7), "add"), _LIN),
    "cvit_GGCA_ADD_DEConv_RepBn3": (_layers((2, 2, 1), _MIXED), ("features1", (64, 56, 56), "add"), _LIN),
    "cvit_GGCA_ADD_DEConv_RepBn4": (_layers((4, 1), "cdd cdd cdcd cddc ccdc", True), ("stem", (512, 7, 7), "add"),
                                    _LIN),
    "cvit_GGCA_ADD_DEConv_RepBn5": (_layers((4, 1), _R8, True), ("stem", (512, 7, 7), "add"), _LIN),
}
NAMES = tuple(TABLE)


def ggca_site(name):
    """How many convs run before the GGCA combine (None: the variant has no GGCA)."""
    layers, g, _ = TABLE[name]
    if g is None:
        return None
    return len(layers) if g[0] == "stem" else max(i for i, l in enumerate(layers) if l[0] == g[0]) + 1


def shared_conv(w1, b1, bn, w2, b2, v):
    """GGCA.shared_conv on [N, cg, h, w]: 1x1, BatchNorm (eval), ReLU, 1x1.
    w1 [cr, cg, 1, 1], bn = (running_mean, running_var, weight, bias)."""
    v = F.conv2d(v, w1, b1)
    v = F.batch_norm(v, bn[0], bn[1], bn[2], bn[3], False, 0.1, BN_EPS)
    return F.conv2d(F.relu(v), w2, b2)


def ggca_weights(sd):
    q = "ggca.shared_conv."
    return (sd[q + "0.weight"], sd[q + "0.bias"],
            (sd[q + "1.running_mean"], sd[q + "1.running_var"], sd[q + "1.weight"], sd[q + "1.bias"]),
            sd[q + "3.weight"], sd[q + "3.bias"])


def ggca(weights, x, groups=GROUPS):
    """GGCA.forward on fp32 NCHW [B, C, H, W] (any H, W); returns x * att_h * att_w."""
    B, C, H, W = x.shape
    gc = C // groups
    xg = x.reshape(B * groups, gc, H, W)
    z = lambda v: shared_conv(*weights, v)  # noqa: E731
    att_h = torch.sigmoid(z(F.adaptive_avg_pool2d(xg, (H, 1))) + z(F.adaptive_max_pool2d(xg, (H, 1))))
    att_w = torch.sigmoid(z(F.adaptive_avg_pool2d(xg, (1, W))) + z(F.adaptive_max_pool2d(xg, (1, W))))
    out = x.view(B, groups, gc, H, W) * att_h.view(B, groups, gc, H, 1) * att_w.view(B, groups, gc, 1, W)
    return out.view(B, C, H, W)


def ggca_combine(weights, x, op, groups=GROUPS):
    g = ggca(weights, x, groups)
    return x * g if op in ("mul", 0) else x + g


def _layer_weights(sd, layer):
    seq, idx, kind, *_ = layer
    p = f"{seq}.{idx}"
    return (sd[p + ".weight"], sd[p + ".bias"]) if kind == "conv" else deconv_fold(sd, p)


def _fold(sd, layer):
    """Conv (+ DEConv fold) + eval BN folded in fp32: W' = W s, b' = (b - mean) s + beta."""
    w, b = _layer_weights(sd, layer)
    seq, bn = layer[0], layer[5]
    if bn is None:
        return w, b
    q = f"{seq}.{bn}."
    s = sd[q + "weight"] / torch.sqrt(sd[q + "running_var"] + torch.tensor(BN_EPS, dtype=torch.float32))
    return w * s.view(-1, 1, 1, 1), (b - sd[q + "running_mean"]) * s + sd[q + "bias"]


def _tail(sd, h, pos_index, ff, lin=None):
    B = h.shape[0]
    y = h.permute(0, 2, 3, 1).reshape(B, 1, -1)          # 'b c (h p1) (w p2) -> b (h w) (p1 p2 c)'
    lin = lin or (lambda inp, w, b=None: F.linear(inp, w, b))
    y = lin(y, sd["patch_to_embedding.weight"], sd["patch_to_embedding.bias"])
    x = torch.cat((sd["cls_token"].expand(B, -1, -1), y), 1) + _pos_rows(sd, pos_index, B)
    x = _transformer(sd, x, lin=lin, ff_norm=ff[0], ff_eps=ff[1])
    hid = F.relu(lin(x[:, 0], sd["mlp_head.0.weight"], sd["mlp_head.0.bias"]))
    return F.linear(hid, sd["mlp_head.2.weight"], sd["mlp_head.2.bias"])


def _forward(name, sd, img, pos_index, rnd, return_features):
    layers, g, ff = TABLE[name]
    sd = to_torch_sd(sd)
    site = ggca_site(name)
    r = rnd or (lambda t: t)
    h = r(img.float())
    pre = combined = None
    for i, layer in enumerate(layers):
        if rnd is None:
            w, b = _layer_weights(sd, layer)
            h = F.conv2d(h, w, b, padding=1)
            if layer[5] is not None:
                q = f"{layer[0]}.{layer[5]}."
                h = F.batch_norm(h, sd[q + "running_mean"], sd[q + "running_var"], sd[q + "weight"], sd[q + "bias"],
                                 False, 0.1, BN_EPS)
        else:
            w, b = _fold(sd, layer)
            h = F.conv2d(h, r(w), b, padding=1)
        if layer[6]:
            h = F.relu(h)
        if layer[7]:
            h = F.max_pool2d(h, 2, 2)
        h = r(h)
        if site == i + 1:
            pre = h
            h = combined = r(ggca_combine(ggca_weights(sd), h, g[2]))
    if pre is None:
        pre = h
    lin = None if rnd is None else (lambda inp, w, b=None: F.linear(r(inp), r(w), b))
    out = _tail(sd, h, pos_index, ff, lin=lin)
    return (out, pre, combined) if return_features else out


@torch.no_grad()
def forward_fp32(name, sd, img, pos_index=None, return_features=False):
    """The reference CViT.forward of variant `name` on normalised fp32 NCHW
    input.  return_features: (logits, the GGCA's input map - the stem output
    [B,512,7,7], RepBn3: features1's [B,64,56,56] -, that map after the combine
    or None for cvit_DEConv)."""
    return _forward(name, sd, img, pos_index, None, return_features)


@torch.no_grad()
def forward_emulated(name, sd, img, pos_index=None, dtype="bf16", return_features=False):
    """The gfx950 path's rounding points (module doc), fp32 accumulation everywhere."""
    return _forward(name, sd, img, pos_index, lambda t: round_to(t, dtype), return_features)
