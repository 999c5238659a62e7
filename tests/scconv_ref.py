"""CPU reference of the ScConv block and of cvit_GGCA_ADD_ScConv
(fac_fake_amd/scconv.py); test infrastructure, beside mdfa_ref.py and
variants_ref.py, whose stem walk, GGCA and tail it reuses.

The project's own restatement of ``ScConv`` of
``CViT-main/model/other/cvit_GGCA_ADD_ScConv.py`` (:311-353, with its defaults)
and of that file's ``CViT``, written from the block's formulas, functional over
the state_dict, on PyTorch CPU ops:

* ``scconv_fold``     the block's state_dict entries and the BatchNorm that
                      follows it as fac_scconv_pack's operands (fp32; k_c =
                      gamma_c / sum(gamma), the BatchNorm as scale and shift).
* ``round_ops``       the operands as the kernel holds them: the five conv
                      weights on the 16-bit grid.
* ``gn_t``            step 1: t = gamma (x - mu_g) rstd_g + beta, from the
                      input or from given (mu, rstd) statistics.
* ``scconv_block``    ScConv -> scale, shift -> ReLU -> optional 2x2 max-pool in
                      float64 or fp32, the gate taken as z > 0 (what r > 0.5 is
                      in exact arithmetic), optionally with the kernel's declared
                      roundings: y (the gated map), u | l, the output; the means
                      behind the softmax then come from the rounded u | l.
* ``linear_means``    the 2C means behind the softmax from sums of u and l alone
                      (total, border rows and columns, corners), as scconv.hip
                      takes them.
* ``near_mask`` / ``excluded``  the near-threshold band of the hard gate.
* ``forward_fp32`` / ``forward_emulated``  CViT.forward of the class.

Pinned against tests/golden/scconv_*.npz, which tools/make_golden_scconv.py
produced from the reference's own module and class.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.cvit_torch import BN_EPS, LN_EPS, round_to, to_torch_sd
from variants_ref import _fold, _layer_weights, _layers, _tail, ggca, ggca_weights

NAME = "cvit_GGCA_ADD_ScConv"
NAMES = (NAME,)
GN_EPS = 1e-5
GN_GROUPS = 4
SC_AT = (4, 7, 10, 12)            # the convs of the plain (4, 1) stem that are ScConv blocks
LAYERS = [((l[0], l[1], "sc", l[4], l[4]) + l[5:]) if i in SC_AT else l
          for i, l in enumerate(_layers((4, 1), "ccc ccc ccc cccc cccc"))]
GGCA = ("stem", (512, 7, 7), "add")
_LN = ("1.fn.norm", LN_EPS)
PACK_ORDER = ("gamma", "beta", "kc", "squeeze1", "squeeze2", "gwc_w", "gwc_b", "pwc1", "pwc2", "scale", "shift")
W16 = ("squeeze1", "squeeze2", "gwc_w", "pwc1", "pwc2")     # the operands that are 16-bit in the kernel


def scconv_fold(sd, prefix, bn_prefix=None, dtype=torch.float32):
    """fac_scconv_pack's operands from the state_dict (scconv.scconv_fold must
    equal this bitwise in fp32).  bn_prefix None: scale 1, shift 0 (the bare
    block).  ValueError where sum(gamma) is 0 or not finite."""
    f = lambda k: torch.as_tensor(sd[k]).detach().to(dtype)  # noqa: E731
    p = prefix + "."
    g = f(p + "SRU.gn.weight")
    c = g.shape[0]
    tot = g.sum()
    if not bool(torch.isfinite(tot)) or float(tot) == 0.0:
        raise ValueError(f"ScConv {prefix}: sum(gn.weight) is {float(tot)}; the block divides by it")
    ops = dict(gamma=g.contiguous(), beta=f(p + "SRU.gn.bias").contiguous(), kc=(g / tot).contiguous(),
               squeeze1=f(p + "CRU.squeeze1.weight").reshape(c // 4, c // 2).contiguous(),
               squeeze2=f(p + "CRU.squeeze2.weight").reshape(c // 4, c // 2).contiguous(),
               gwc_w=f(p + "CRU.GWC.weight").contiguous(), gwc_b=f(p + "CRU.GWC.bias").contiguous(),
               pwc1=f(p + "CRU.PWC1.weight").reshape(c, c // 4).contiguous(),
               pwc2=f(p + "CRU.PWC2.weight").reshape(3 * c // 4, c // 4).contiguous())
    if bn_prefix is None:
        ops["scale"], ops["shift"] = torch.ones(c, dtype=dtype), torch.zeros(c, dtype=dtype)
    else:
        q = bn_prefix + "."
        s = f(q + "weight") / torch.sqrt(f(q + "running_var") + BN_EPS)
        ops["scale"], ops["shift"] = s.contiguous(), (f(q + "bias") - f(q + "running_mean") * s).contiguous()
    return ops


def round_ops(ops, dt):
    return {k: (round_to(v, dt) if k in W16 else v) for k, v in ops.items()}


def gn_stats(x, dtype=torch.float64):
    """(mu, rstd) [B, 4] of GroupNorm(4, C) on NCHW x: biased variance, eps 1e-5."""
    B, C = x.shape[:2]
    xg = x.to(dtype).reshape(B, GN_GROUPS, -1)
    mu = xg.mean(2)
    var = ((xg - mu.unsqueeze(2)) ** 2).mean(2)
    return mu, 1.0 / torch.sqrt(var + GN_EPS)


def gn_t(x, ops, dtype=torch.float64, stats=None):
    """t [B, C, H, W]; stats: (mu, rstd) [B, 4] to use instead of the input's own."""
    B, C, H, W = x.shape
    mu, rstd = gn_stats(x, dtype) if stats is None else (stats[0].to(dtype), stats[1].to(dtype))
    xg = x.to(dtype).reshape(B, GN_GROUPS, C // GN_GROUPS, H, W)
    n = ((xg - mu.view(B, GN_GROUPS, 1, 1, 1)) * rstd.view(B, GN_GROUPS, 1, 1, 1)).reshape(B, C, H, W)
    return n * ops["gamma"].to(dtype).view(1, C, 1, 1) + ops["beta"].to(dtype).view(1, C, 1, 1)


def gate(x, t, ops, dtype=torch.float64):
    """y of step 2 from t: the gate is z > 0."""
    C = x.shape[1]
    x = x.to(dtype)
    z = t * ops["kc"].to(dtype).view(1, C, 1, 1)
    r = torch.sigmoid(z)
    on = z > 0
    w1 = torch.where(on, torch.ones_like(r), r)
    w2 = torch.where(on, torch.zeros_like(r), r)
    x1, x2 = w1 * x, w2 * x
    h = C // 2
    return torch.cat([x1[:, :h] + x2[:, h:], x1[:, h:] + x2[:, :h]], 1)


def squeeze(y, ops, dtype=torch.float64):
    C = y.shape[1]
    h, q = C // 2, C // 4
    u = F.conv2d(y[:, :h], ops["squeeze1"].to(dtype).view(q, h, 1, 1))
    l = F.conv2d(y[:, h:], ops["squeeze2"].to(dtype).view(q, h, 1, 1))
    return u, l


def transform(u, l, ops, dtype=torch.float64):
    """(Y1, Y2) of step 4, C channels each."""
    q = u.shape[1]
    C = 4 * q
    y1 = F.conv2d(u, ops["gwc_w"].to(dtype), ops["gwc_b"].to(dtype), padding=1, groups=2) + \
        F.conv2d(u, ops["pwc1"].to(dtype).view(C, q, 1, 1))
    y2 = torch.cat([F.conv2d(l, ops["pwc2"].to(dtype).view(3 * q, q, 1, 1)), l], 1)
    return y1, y2


def linear_means(u, l, ops, dtype=torch.float64):
    """[B, 2C]: the spatial means of cat[Y1, Y2] from sums of u and l alone.  The
    sum of a zero-padded 3x3 conv over the map is, per tap (dy, dx), the sum of
    u minus its last / first row (dy = -1 / +1) and last / first column (dx = -1
    / +1) plus the corner both took away."""
    B, q, H, W = u.shape
    C = 4 * q
    tot, r0, rl, c0, cl = u.sum((2, 3)), u[:, :, 0].sum(2), u[:, :, -1].sum(2), u[:, :, :, 0].sum(2), u[:, :, :, -1].sum(2)
    S = torch.empty(B, q, 3, 3, dtype=dtype)
    for ky in range(3):
        for kx in range(3):
            s = tot.clone()
            if ky == 0:
                s -= rl
            if ky == 2:
                s -= r0
            if kx == 0:
                s -= cl
            if kx == 2:
                s -= c0
            if ky != 1 and kx != 1:
                s += u[:, :, -1 if ky == 0 else 0, -1 if kx == 0 else 0]
            S[:, :, ky, kx] = s
    gw = ops["gwc_w"].to(dtype)                                  # [C, q/2, 3, 3], two groups
    m1 = torch.cat([torch.einsum("oikl,bikl->bo", gw[g * C // 2:(g + 1) * C // 2], S[:, g * q // 2:(g + 1) * q // 2])
                    for g in range(2)], 1)
    m1 = (m1 + tot @ ops["pwc1"].to(dtype).t()) / (H * W) + ops["gwc_b"].to(dtype)
    ml = l.sum((2, 3)) / (H * W)
    return torch.cat([m1, ml @ ops["pwc2"].to(dtype).t(), ml], 1)


def scconv_block(x, ops, dtype=torch.float64, round=None, pool=False, parts=False, stats=None, raw=False):
    """ScConv(x) -> * scale + shift -> ReLU -> optional 2x2 max-pool on NCHW x.
    round: None, or "fp16" / "bf16" for scconv.hip's declared roundings (dtype
    must then be fp32; the caller rounds the input and round_ops the weights).
    parts: also dict(t, y, u, l, s).  raw: ScConv(x) alone, what the reference
    module returns (no scale, shift, ReLU, pool or output rounding)."""
    assert round is None or dtype == torch.float32
    r = (lambda v: round_to(v, round)) if round else (lambda v: v)
    C = x.shape[1]
    t = gn_t(x, ops, dtype, stats)
    y = r(gate(x, t, ops, dtype))
    u, l = squeeze(y, ops, dtype)
    u, l = r(u), r(l)
    y1, y2 = transform(u, l, ops, dtype)
    s = torch.softmax(torch.cat([y1, y2], 1).mean((2, 3)), 1)
    out = s[:, :C, None, None] * y1 + s[:, C:, None, None] * y2
    if raw:
        return (out, dict(t=t, y=y, u=u, l=l, s=s)) if parts else out
    out = F.relu(out * ops["scale"].to(dtype).view(1, C, 1, 1) + ops["shift"].to(dtype).view(1, C, 1, 1))
    out = r(out)
    if pool:
        out = F.max_pool2d(out, 2, 2)
    return (out, dict(t=t, y=y, u=u, l=l, s=s)) if parts else out


def near_mask(t64, tau):
    """Elements whose float64 |t| <= tau: no two finite-precision evaluations agree on their side of the gate."""
    return t64.abs() <= tau


def excluded(near, pool=False):
    """[B, H, W] (pooled: [B, H/2, W/2]): output pixels with a near element in
    any channel of any input pixel of their 3x3 neighbourhood (pooled: of any of
    the window's four)."""
    pix = near.any(1, keepdim=True).to(torch.float32)
    ex = F.max_pool2d(pix, 3, 1, 1)
    if pool:
        ex = F.max_pool2d(ex, 2, 2)
    return ex[:, 0] > 0


def tau_of(x, ops, how="formula"):
    """(tau, t64): 8 x the largest |t_fp32 - t_float64| of a plain fp32 torch
    evaluation of step 1 on x: the reference's own arithmetic, never a kernel's.
    how "formula": mean, biased variance, (x - mu) / sqrt(var + eps) gamma + beta
    with torch's fp32 tensor ops (gn_t in fp32); "module": F.group_norm, what the
    reference module itself runs, whose fp32 CPU statistics are several times
    less accurate."""
    t64 = gn_t(x, ops, torch.float64)
    if how == "module":
        t32 = F.group_norm(x.float(), GN_GROUPS, ops["gamma"].float(), ops["beta"].float(), GN_EPS)
    else:
        t32 = gn_t(x.float(), ops, torch.float32)
    return 8.0 * float((t32.double() - t64).abs().max()), t64


def _bn_of(layer):
    return f"{layer[0]}.{layer[5]}"


def _forward(sd, img, pos_index, rnd, return_features):
    sd = to_torch_sd(sd)
    r = rnd[0] if rnd else (lambda t: t)
    h = r(img.float())
    maps = {}
    for i, layer in enumerate(LAYERS):
        if layer[2] == "sc":
            p = f"{layer[0]}.{layer[1]}"
            maps[p + "_in"] = h
            ops = scconv_fold(sd, p, _bn_of(layer))
            if rnd:
                ops = round_ops(ops, rnd[1])
            h = maps[p] = scconv_block(h, ops, torch.float32, round=rnd[1] if rnd else None, pool=layer[7])
            continue
        if rnd is None:
            w, b = _layer_weights(sd, layer)
            h = F.conv2d(h, w, b, padding=1)
            q = _bn_of(layer) + "."
            h = F.batch_norm(h, sd[q + "running_mean"], sd[q + "running_var"], sd[q + "weight"], sd[q + "bias"],
                             False, 0.1, BN_EPS)
        else:
            w, b = _fold(sd, layer)
            h = F.conv2d(h, r(w), b, padding=1)
        h = F.relu(h)
        if layer[7]:
            h = F.max_pool2d(h, 2, 2)
        h = r(h)
    maps["ggca_in"] = h
    h = maps["ggca"] = r(h + ggca(ggca_weights(sd), h))
    lin = None if rnd is None else (lambda inp, w, b=None: F.linear(r(inp), r(w), b))
    out = _tail(sd, h, pos_index, _LN, lin=lin)
    return (out, maps) if return_features else out


@torch.no_grad()
def forward_fp32(sd, img, pos_index=None, return_features=False):
    """CViT.forward of model/other/cvit_GGCA_ADD_ScConv.py on normalised fp32 NCHW input.
    return_features: (logits, {"features1.13_in", "features1.13", ...: each block's input and output map})."""
    return _forward(sd, img, pos_index, None, return_features)


@torch.no_grad()
def forward_emulated(sd, img, pos_index=None, dtype="bf16", return_features=False):
    """The gfx950 path's rounding points (variants_ref's, scconv_block's declared ones), fp32 accumulation everywhere."""
    return _forward(sd, img, pos_index, (lambda t: round_to(t, dtype), dtype), return_features)
