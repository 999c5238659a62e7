"""CPU restatement of CA_S3D_v3 (sx_exp_deepfakedetect-master/S3D/CA_S3D.py:9-60)
for the tests; a helper, not collected as a test.

S3D's layers come from oracle.s3d_torch; the new part is the GCNet context
block (new_model/context_block_3d.py:5-88, 'avg' pooling, 'channel_add'):

* ``context_term`` / ``context_add_ref`` - the block on a channels-last map,
  in a chosen float type (fp64: the truth the kernels are measured against;
  fp32: how far plain fp32 torch sits from it);
* ``features_fp32`` / ``forward_fp32``   - the reference's arithmetic;
* ``features_emulated`` / ``forward_emulated`` - the gfx950 path's rounding
  points: those of oracle.s3d_torch.features_emulated, plus
  ``round16(x + term)`` with ``term`` computed in fp32 from the rounded ``x``.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from fac_fake_amd.weights import ca_s3d_base
from oracle import s3d_torch as O
from oracle.cvit_torch import round_to, to_torch_sd

LN_EPS = 1e-5
CTX_KEYS = ("0.weight", "0.bias", "1.weight", "1.bias", "3.weight", "3.bias")


def load_blocks(golden):
    """The every-block fixture: one file per SRM setting (the clip keys are in the 'no' file), merged."""
    return {**golden("ca_s3d_golden_blocks.npz"), **golden("ca_s3d_golden_blocks_srm.npz")}


def logit_gate(g_blocks, g, srm, dt):
    """Bound on |logit - reference logit| for the 16-bit path on fixture `g`: twice the emulation's own
    logit envelope, taken as the larger of `g`'s and the 8-clip fixture's for the same model and dtype
    (two clips sample the rounding envelope poorly: its bf16 values differ 5x between the SRM settings)."""
    k = f"env_logit_{srm}_{dt}"
    return 2 * max(float(g[k]), float(g_blocks[k]))


def ctx_weights(sd, p):
    """The six tensors of base.{i}.channel_add_conv as (w0 [P,C], b0, ln_w, ln_b, w3 [C,P], b3)."""
    w0, b0, lw, lb, w3, b3 = (torch.as_tensor(sd[f"{p}.channel_add_conv.{k}"]) for k in CTX_KEYS)
    q, c = w0.shape[0], w0.shape[1]
    return w0.reshape(q, c), b0.reshape(q), lw.reshape(q), lb.reshape(q), w3.reshape(c, q), b3.reshape(c)


def context_term(ctx: torch.Tensor, weights, dtype=torch.float32) -> torch.Tensor:
    """term [n, C] from the pooled ctx [n, C]."""
    w0, b0, lw, lb, w3, b3 = (t.to(dtype) for t in weights)
    h = ctx.to(dtype) @ w0.t() + b0
    h = F.layer_norm(h, (h.shape[1],), lw, lb, LN_EPS)
    return h.clamp(0, 6) @ w3.t() + b3


def context_add_ref(x16: torch.Tensor, weights, dtype=torch.float64):
    """x16 [n, ..., C] 16-bit channels-last -> (x + term [n, ..., C], term [n, C]) in `dtype`."""
    n, c = x16.shape[0], x16.shape[-1]
    x = x16.to(dtype).reshape(n, -1, c)
    term = context_term(x.mean(dim=1), weights, dtype)
    return (x + term[:, None, :]).reshape(x16.shape), term


def _ctx_ncdhw(sd, p, y, terms=None):
    """ContextBlock3d.forward on y [B, C, T, H, W] fp32, with the torch ops the
    reference module calls (context_block_3d.py:30-36, :70, :85-86): the
    LayerNorm + ReLU6 cut makes the term sensitive to the last bits of the
    pooled vector, so the same ops keep the restatement on the reference."""
    a = f"{p}.channel_add_conv"
    lw = torch.as_tensor(sd[f"{a}.1.weight"])
    h = F.conv3d(F.adaptive_avg_pool3d(y, 1), torch.as_tensor(sd[f"{a}.0.weight"]), torch.as_tensor(sd[f"{a}.0.bias"]))
    h = F.relu6(F.layer_norm(h, list(lw.shape), lw, torch.as_tensor(sd[f"{a}.1.bias"]), LN_EPS))
    term = F.conv3d(h, torch.as_tensor(sd[f"{a}.3.weight"]), torch.as_tensor(sd[f"{a}.3.bias"]))
    if terms is not None:
        terms.append(term[:, :, 0, 0, 0])
    return y + term


@torch.no_grad()
def features_fp32(sd, x, srm: bool, taps=None, terms=None, skip_ctx=()):
    """`base` (CA_S3D.py:20-46).  taps: every base[i] output [B, C, T, H, W];
    terms: each context block's term [B, C]; skip_ctx: context blocks (base
    indices) replaced by the identity."""
    sd = to_torch_sd(sd)
    y = F.conv3d(x.float(), sd["SRM.hpf.weight"], padding=(0, 2, 2)) if srm else x.float()
    for i, L in enumerate(ca_s3d_base(srm)):
        p = f"base.{i}"
        if L[0] == "ctx":
            if i not in skip_ctx:
                y = _ctx_ncdhw(sd, p, y, terms)
            elif terms is not None:
                terms.append(None)
        elif L[0] == "sep":
            y = O._sep(sd, p, y, L[3], L[4], L[5])
        elif L[0] == "basic":
            y = O._basic(sd, p, y)
        elif L[0] == "pool":
            y = F.max_pool3d(y, *L[1:])
        else:
            y0 = O._basic(sd, f"{p}.branch0.0", y)
            y1 = O._sep(sd, f"{p}.branch1.1", O._basic(sd, f"{p}.branch1.0", y), 3, 1, 1)
            y2 = O._sep(sd, f"{p}.branch2.1", O._basic(sd, f"{p}.branch2.0", y), 3, 1, 1)
            y3 = O._basic(sd, f"{p}.branch3.1", F.max_pool3d(y, 3, 1, 1))
            y = torch.cat((y0, y1, y2, y3), 1)
        if taps is not None:
            taps.append(y)
    return y


@torch.no_grad()
def forward_fp32(sd, x, srm: bool):
    sd = to_torch_sd(sd)
    y = features_fp32(sd, x, srm)
    y = F.avg_pool3d(y, (2, y.size(3), y.size(4)), stride=1)
    y = F.conv3d(y, sd["fc.0.weight"], sd["fc.0.bias"])
    return torch.mean(y.view(y.size(0), y.size(1), y.size(2)), 2)


@torch.no_grad()
def features_emulated(sd, x, srm: bool, dtype: str = "bf16", taps=None):
    """`base` at the gfx950 path's rounding points."""
    sd = to_torch_sd(sd)
    r = lambda t: round_to(t, dtype)  # noqa: E731

    def conv(y, ck, bn, stride=1, pad=0):
        w, b = O._fold(sd, ck, bn)
        return r(F.relu(F.conv3d(y, r(w), b, stride=stride, padding=pad)))

    def basic(p, y):
        return conv(y, p + ".conv.weight", p + ".bn")

    def sep(p, y, k, s, pd):
        y = conv(y, p + ".conv_s.weight", p + ".bn_s", (1, s, s), (0, pd, pd))
        return conv(y, p + ".conv_t.weight", p + ".bn_t", (s, 1, 1), (pd, 0, 0))

    y = r(x.float())
    if srm:
        y = r(F.conv3d(y, r(sd["SRM.hpf.weight"]), padding=(0, 2, 2)))
    for i, L in enumerate(ca_s3d_base(srm)):
        p = f"base.{i}"
        if L[0] == "ctx":
            y = r(_ctx_ncdhw(sd, p, y))     # y is 16-bit-valued: term in fp32 from it, one rounding after the add
        elif L[0] == "sep":
            y = sep(p, y, L[3], L[4], L[5])
        elif L[0] == "basic":
            y = basic(p, y)
        elif L[0] == "pool":
            y = F.max_pool3d(y, *L[1:])
        else:
            y0 = basic(f"{p}.branch0.0", y)
            y1 = sep(f"{p}.branch1.1", basic(f"{p}.branch1.0", y), 3, 1, 1)
            y2 = sep(f"{p}.branch2.1", basic(f"{p}.branch2.0", y), 3, 1, 1)
            y3 = basic(f"{p}.branch3.1", F.max_pool3d(y, 3, 1, 1))
            y = torch.cat((y0, y1, y2, y3), 1)
        if taps is not None:
            taps.append(y)
    return y


@torch.no_grad()
def forward_emulated(sd, x, srm: bool, dtype: str = "bf16", taps=None):
    sd = to_torch_sd(sd)
    r = lambda t: round_to(t, dtype)  # noqa: E731
    y = features_emulated(sd, x, srm, dtype, taps)
    y = r(F.avg_pool3d(y, (2, y.size(3), y.size(4)), stride=1))
    y = r(y.mean(2, keepdim=True))
    y = F.conv3d(y, r(sd["fc.0.weight"]), sd["fc.0.bias"])
    return y.view(y.size(0), y.size(1))
