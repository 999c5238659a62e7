"""CPU reference of the MDFA block and the three MDFA CViT classes
(fac_fake_amd/mdfa.py); test infrastructure, beside bfm_ref.py and
variants_ref.py, whose stem walk, GGCA, BFM and tail it reuses.

The project's own restatement of ``MDFA`` of
``CViT-main/model/other/cvit_GGCA4_MDFA5.py`` (:158-261) and of the ``CViT``
classes of ``cvit_GGCA4_MDFA5.py``, ``cvit_MDFA_BFM.py`` and
``cvit_BFM_MDFA.py``, functional over the state_dict, on PyTorch CPU ops:

* ``mdfa_fold``        the block's state_dict entries as fac_mdfa_pack's
                        operands, every eval BatchNorm folded in fp32.
* ``mdfa_module``      the block the way the reference writes it: five
                        branches, the 5c-channel cat, hebing's two products
                        and their elementwise max, larry * cat, conv_cat.
* ``mdfa_block``       the block the way mdfa.hip computes it (dropped taps,
                        one scalar m_p per pixel, branch 5 as a per-crop
                        vector), in float64 or fp32, optionally with the
                        kernel's two rounding points: q = cat^2 (fp16: clamped
                        to 65504) and the output.  The caller rounds the input
                        and the 16-bit weights (``round_ops``).
* ``kept_taps``        the taps of the 28 that touch an h x w map at all.
* ``forward_fp32`` / ``forward_emulated``  CViT.forward of a class.

Pinned against tests/golden/mdfa_golden.npz, which tools/make_golden_mdfa.py
produced from the reference's own classes.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

import bfm_ref
from oracle.cvit_torch import BN_EPS, LN_EPS, round_to, to_torch_sd
from variants_ref import _fold, _layer_weights, _layers, _tail, ggca, ggca_weights

_PLAIN = "ccc ccc ccc cccc cccc"
_LN = ("1.fn.norm", LN_EPS)
_L41 = _layers((4, 1), _PLAIN)
# name -> (layers, ggca (site, (C, H, W), op) | None, mdfa (site, C), bfm (site, C) | None, unused ggca (C, H, W) | None)
TABLE = {
    "cvit_GGCA4_MDFA5": (_L41, ("stem", (512, 7, 7), "att"), ("features1", 256), None, None),
    "cvit_MDFA_BFM": (_L41, None, ("features1", 256), ("stem", 512), (256, 14, 14)),
    "cvit_BFM_MDFA": (_L41, None, ("stem", 512), ("features1", 256), (256, 14, 14)),
}
NAMES = tuple(TABLE)
DILATIONS = (6, 12, 18)
F16_MAX = 65504.0
W16 = ("w1", "w2", "w3", "w4")          # the operands that are 16-bit in the kernel, with wcat[:, :4c]


def _bn_fold(sd, conv, bn, dtype=torch.float32):
    f = lambda k: torch.as_tensor(sd[k]).detach().to(dtype)  # noqa: E731
    s = f(bn + ".weight") / torch.sqrt(f(bn + ".running_var") + BN_EPS)
    w = f(conv + ".weight")
    return (w * s.view(-1, 1, 1, 1)).contiguous(), ((f(conv + ".bias") - f(bn + ".running_mean")) * s + f(bn + ".bias")).contiguous()


def mdfa_fold(sd, prefix="mdfa", dtype=torch.float32):
    """fac_mdfa_pack's operands from the state_dict, fp32 (mdfa.mdfa_fold must
    equal this bitwise); dtype float64 folds in float64, for the comparison with
    the reference module in float64."""
    p = prefix + "."
    ops, bias = {}, []
    for i in range(1, 5):
        w, b = _bn_fold(sd, f"{p}branch{i}.0", f"{p}branch{i}.1", dtype)
        ops[f"w{i}"] = w.reshape(w.shape[0], w.shape[1]).contiguous() if i == 1 else w
        bias.append(b)
    ops["bias4"] = torch.stack(bias).contiguous()
    w5, ops["b5"] = _bn_fold(sd, p + "branch5_conv", p + "branch5_bn", dtype)
    ops["w5"] = w5.reshape(w5.shape[0], w5.shape[1]).contiguous()
    wc, ops["bcat"] = _bn_fold(sd, p + "conv_cat.0", p + "conv_cat.1", dtype)
    ops["wcat"] = wc.reshape(wc.shape[0], wc.shape[1]).contiguous()
    ops["ws"] = torch.as_tensor(sd[p + "Hebing.kongjian.Conv1x1.weight"]).detach().to(dtype).reshape(-1).contiguous()
    ops["wt"] = torch.as_tensor(sd[p + "Hebing.tongdao.fc.weight"]).detach().to(dtype).reshape(-1).contiguous()
    return ops


def round_ops(ops, dt):
    """The operands as the kernel holds them: w1..w4 and wcat[:, :4c] on the 16-bit grid, the rest fp32."""
    out = {k: (round_to(v, dt) if k in W16 else v) for k, v in ops.items()}
    c = ops["bcat"].shape[0]
    out["wcat"] = torch.cat([round_to(ops["wcat"][:, :4 * c], dt), ops["wcat"][:, 4 * c:]], 1)
    return out


def kept_taps(h, w):
    """[(branch 1..4, ky, kx)] of the 28 taps (ky, kx in -1..1; branch 1 has the
    centre only) that are inside an h x w map for at least one pixel."""
    taps = [(1, 0, 0)]
    for b, d in enumerate(DILATIONS, 2):
        taps += [(b, ky, kx) for ky in (-1, 0, 1) for kx in (-1, 0, 1) if abs(ky) * d < h and abs(kx) * d < w]
    return taps


def in_map_taps(h, w, d):
    """Per pixel, how many of a dilation-d 3x3 conv's taps are inside the map: [h, w] float64."""
    ys, xs = torch.arange(h).view(h, 1), torch.arange(w).view(1, w)
    rows = sum(((ys + k * d >= 0) & (ys + k * d < h)).double() for k in (-1, 0, 1))
    cols = sum(((xs + k * d >= 0) & (xs + k * d < w)).double() for k in (-1, 0, 1))
    return rows * cols


def branches(x, ops, dtype=torch.float64, drop=False):
    """cat4 = [b1 b2 b3 b4] on NCHW x: ReLU(conv_i(x) + bias_i), BN folded.
    drop: the 3x3 weights with every tap outside kept_taps(h, w) set to zero."""
    x = x.to(dtype)
    h, w = x.shape[2:]
    keep = set(kept_taps(h, w))
    c = ops["bias4"].shape[1]
    outs = [F.conv2d(x, ops["w1"].to(dtype).view(c, c, 1, 1), ops["bias4"][0].to(dtype))]
    for i, d in enumerate(DILATIONS, 2):
        wt = ops[f"w{i}"].to(dtype)
        if drop:
            wt = wt.clone()
            for ky in (-1, 0, 1):
                for kx in (-1, 0, 1):
                    if (i, ky, kx) not in keep:
                        wt[:, :, ky + 1, kx + 1] = 0
        outs.append(F.conv2d(x, wt, ops["bias4"][i - 1].to(dtype), padding=d, dilation=d))
    return F.relu(torch.cat(outs, 1))


def branch5(x, ops, dtype=torch.float64):
    """g [B, c]: ReLU(W5 mean_hw(x) + b5)."""
    return F.relu(F.linear(x.to(dtype).mean((2, 3)), ops["w5"].to(dtype), ops["b5"].to(dtype)))


def gates(cat4, g, ops, dtype=torch.float64):
    """(s [B,h,w], t [B]): sigmoid(w_s . cat_p) and ReLU(w_t . mean_p cat_p), g's shares as per-crop scalars."""
    c4 = cat4.shape[1]
    ws, wt = ops["ws"].to(dtype), ops["wt"].to(dtype)
    s = torch.sigmoid(torch.einsum("bchw,c->bhw", cat4, ws[:c4]) + (g @ ws[c4:]).view(-1, 1, 1))
    t = F.relu(torch.einsum("bchw,c->bhw", cat4, wt[:c4]).mean((1, 2)) + g @ wt[c4:])
    return s, t


def mdfa_block(x, ops, dtype=torch.float64, round=None, parts=False):
    """mdfa.hip's arithmetic on NCHW x: out = ReLU(m_p (Wcat[:, :4c] q_p + e_b) + bcat)
    with q = cat4^2, e_b = Wcat[:, 4c:] g_b^2, m_p = max(t_b, s_p).  round: None,
    or "fp16" / "bf16" for the kernel's rounding points (dtype must then be
    fp32).  parts: also return dict(cat4, g, s, t, m)."""
    assert round is None or dtype == torch.float32
    c = ops["bcat"].shape[0]
    cat4 = branches(x, ops, dtype, drop=True)
    g = branch5(x, ops, dtype)
    s, t = gates(cat4, g, ops, dtype)
    m = torch.maximum(t.view(-1, 1, 1), s)
    q = cat4 * cat4
    if round:
        q = round_to(q.clamp(max=F16_MAX) if round == "fp16" else q, round)
    wcat = ops["wcat"].to(dtype)
    acc = F.conv2d(q, wcat[:, :4 * c].reshape(c, 4 * c, 1, 1))
    e = (g * g) @ wcat[:, 4 * c:].t()
    out = F.relu(m.unsqueeze(1) * (acc + e.view(-1, c, 1, 1)) + ops["bcat"].to(dtype).view(1, c, 1, 1))
    if round:
        out = round_to(out, round)
    return (out, dict(cat4=cat4, g=g, s=s, t=t, m=m)) if parts else out


def mdfa_module(x, ops, dtype=torch.float64):
    """The block in the reference's own form (BN folded): the 5c-channel cat
    with branch 5 upsampled from 1x1 (bilinear, align_corners: a constant map),
    hebing = max(tongdao(cat), kongjian(cat)) elementwise, larry * cat, conv_cat."""
    B, c, h, w = x.shape
    g = branch5(x, ops, dtype)
    gmap = F.interpolate(g.view(B, c, 1, 1), (h, w), None, "bilinear", True)
    cat = torch.cat([branches(x, ops, dtype, drop=False), gmap], 1)
    ws, wt = ops["ws"].to(dtype).view(1, 5 * c, 1, 1), ops["wt"].to(dtype).view(1, 5 * c, 1, 1)
    kong = cat * torch.sigmoid(F.conv2d(cat, ws))
    y = F.relu(F.conv2d(F.adaptive_avg_pool2d(cat, 1), wt))
    tong = cat * F.interpolate(y, size=(h, w), mode="nearest").expand_as(cat)
    larry = torch.max(tong, kong)
    return F.relu(F.conv2d(larry * cat, ops["wcat"].to(dtype).view(c, 5 * c, 1, 1), ops["bcat"].to(dtype)))


def t_share(x, ops, dtype=torch.float64) -> float:
    """Share of pixels where the channel gate t_b is the larger side of max(t_b, s_p)."""
    _, p = mdfa_block(x, ops, dtype, parts=True)
    return float((p["t"].view(-1, 1, 1) > p["s"]).double().mean())


def _site(layers, seq):
    return len(layers) if seq == "stem" else max(i for i, l in enumerate(layers) if l[0] == seq) + 1


def _forward(name, sd, img, pos_index, rnd, return_features):
    layers, g, mdfa, bfm, _unused = TABLE[name]
    sd = to_torch_sd(sd)
    at = lambda s: _site(layers, s[0]) if s is not None else None  # noqa: E731
    ggca_at, mdfa_at, bfm_at = at(g), at(mdfa), at(bfm)
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
        # at one site the reference forwards run at most one of the blocks before the next sequential, and ggca last
        if bfm_at == i + 1:
            maps["bfm_in"] = h
            ops = bfm_ref.bfm_fold(sd)
            if rnd:
                ops = {k: (v if k == "bias3" else r(v)) for k, v in ops.items()}
            h = maps["bfm"] = bfm_ref.bfm_block(h, ops, bfm_ref.BFM_SCALE, dtype=torch.float32,
                                                round=rnd[1] if rnd else None, route=bfm_ref.MODEL_ROUTE)
        if mdfa_at == i + 1:
            maps["mdfa_in"] = h
            ops = mdfa_fold(sd)
            if rnd:
                ops = round_ops(ops, rnd[1])
            h = maps["mdfa"] = mdfa_block(h, ops, dtype=torch.float32, round=rnd[1] if rnd else None)
        if ggca_at == i + 1:
            h = maps["ggca"] = r(ggca(ggca_weights(sd), h))
    lin = None if rnd is None else (lambda inp, w, b=None: F.linear(r(inp), r(w), b))
    out = _tail(sd, h, pos_index, _LN, lin=lin)
    return (out, maps) if return_features else out


@torch.no_grad()
def forward_fp32(name, sd, img, pos_index=None, return_features=False):
    """CViT.forward of model/other/<name>.py on normalised fp32 NCHW input.
    return_features: (logits, {"mdfa_in", "mdfa", ["bfm_in", "bfm"], ["ggca"]: the maps})."""
    return _forward(name, sd, img, pos_index, None, return_features)


@torch.no_grad()
def forward_emulated(name, sd, img, pos_index=None, dtype="bf16", return_features=False):
    """The gfx950 path's rounding points (variants_ref's, bfm_block's for the
    model's route, mdfa_block's two), fp32 accumulation everywhere."""
    return _forward(name, sd, img, pos_index, (lambda t: round_to(t, dtype), dtype), return_features)
