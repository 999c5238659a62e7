"""CPU reference of cvit_GGCA_ADD_DConv (fac_fake_amd/dconv.py); test
infrastructure, beside variants_ref.py whose GGCA and tail it imports.

The project's own restatement of ``CViT-main/model/cvit_GGCA_ADD_DConv.py``,
functional over the state_dict, on PyTorch CPU ops:

* ``idw_reference``    InceptionDWConv2d -> BatchNorm2d (eval) -> ReLU with the
                        ops the reference module calls (split, three grouped
                        ``conv2d``, cat, ``batch_norm``, ``relu``).
* ``idw_fold`` / ``idw_layer``  the same layer the way fac_idwconv computes it:
                        conv biases and BatchNorm folded into a per-channel
                        scale and shift, the taps as stored and summed in index
                        order from 0 over zero-padded shifts, then scale * y +
                        shift, ReLU, optional 2x2 max-pool.
* ``forward_fp32``     CViT.forward, fp32, the reference's ops.
* ``forward_emulated`` the same with 16-bit rounding exactly where the gfx950
                        path rounds: the normalised input, the folded 3x3 conv
                        weights, after every conv or IDW layer's ReLU (and
                        pool), after x + GGCA(x), and in the tail as
                        variants_ref does.

Pinned against tests/golden/dconv_golden.npz, which tools/make_golden_dconv.py
produced from the reference's own class.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.cvit_torch import BN_EPS, LN_EPS, POOL_AFTER, STEM, round_to, stem_indices, to_torch_sd
from variants_ref import _tail, ggca_combine, ggca_weights

NAME = "cvit_GGCA_ADD_DConv"
KINDS = "cii" "cii" "cii" "ciii" "cccc"      # per layer of the base CViT's stem: c Conv2d, i InceptionDWConv2d
BAND = 11
# (Sequential index, kind, cin, cout, BatchNorm index, pool after)
LAYERS = [(ci_, k, cin, cout, bi_, i in POOL_AFTER)
          for i, (k, (cin, cout), (ci_, bi_)) in enumerate(zip(KINDS, STEM, stem_indices()))]
_FF = ("1.fn.norm", LN_EPS)


def _bn(sd, q):
    return sd[q + ".running_mean"], sd[q + ".running_var"], sd[q + ".weight"], sd[q + ".bias"]


def idw_reference(x, w_hw, b_hw, w_w, b_w, w_h, b_h, bn):
    """The reference module's ops on fp32 NCHW x; bn = (mean, var, gamma, beta)."""
    gc = w_hw.shape[0]
    x_id, x_hw, x_w, x_h = torch.split(x, (x.shape[1] - 3 * gc, gc, gc, gc), dim=1)
    y = torch.cat((x_id, F.conv2d(x_hw, w_hw, b_hw, padding=1, groups=gc),
                   F.conv2d(x_w, w_w, b_w, padding=(0, BAND // 2), groups=gc),
                   F.conv2d(x_h, w_h, b_h, padding=(BAND // 2, 0), groups=gc)), dim=1)
    return F.relu(F.batch_norm(y, bn[0], bn[1], bn[2], bn[3], False, 0.1, BN_EPS))


def idw_fold(w_hw, b_hw, w_w, b_w, w_h, b_h, bn):
    """fac_idwconv's operands: taps [gc,9], [gc,11], [gc,11] as stored, scale =
    gamma / sqrt(var + eps), shift = beta - mean * scale (+ bias * scale on the
    conv channels), all fp32."""
    gc = w_hw.shape[0]
    mean, var, gamma, beta = bn
    scale = gamma / torch.sqrt(var + torch.tensor(BN_EPS, dtype=torch.float32))
    shift = beta - mean * scale
    shift[-3 * gc:] += torch.cat([b_hw, b_w, b_h]) * scale[-3 * gc:]
    return w_hw.reshape(gc, 9), w_w.reshape(gc, BAND), w_h.reshape(gc, BAND), scale, shift


def idw_taps(c):
    """Per branch (first channel, taps as (dy, dx) in the kernel's order)."""
    gc = c // 8
    return [(c - 3 * gc, [(t // 3 - 1, t % 3 - 1) for t in range(9)]),
            (c - 2 * gc, [(0, t - 5) for t in range(BAND)]),
            (c - gc, [(t - 5, 0) for t in range(BAND)])]


def idw_layer(x, w_hw, w_w, w_h, scale, shift, pool, dtype=torch.float32):
    """fac_idwconv's arithmetic on NCHW x (fp32 or, for a test's reference,
    float64): y = sum over taps in index order of tap * x shifted (zero
    outside the map), relu(scale * y + shift), optional MaxPool2d(2,2)."""
    x = x.to(dtype)
    N, C, H, W = x.shape
    gc = C // 8
    y = x.clone()
    xp = F.pad(x, (5, 5, 5, 5))
    for (c0, taps), w in zip(idw_taps(C), (w_hw, w_w, w_h)):
        acc = torch.zeros(N, gc, H, W, dtype=dtype)
        for t, (dy, dx) in enumerate(taps):
            acc = acc + w[:, t].to(dtype).view(1, gc, 1, 1) * xp[:, c0:c0 + gc, 5 + dy:5 + dy + H, 5 + dx:5 + dx + W]
        y[:, c0:c0 + gc] = acc
    y = F.relu(scale.to(dtype).view(1, C, 1, 1) * y + shift.to(dtype).view(1, C, 1, 1))
    return F.max_pool2d(y, 2, 2) if pool else y


def _idw_params(sd, p, q):
    return (sd[p + ".dwconv_hw.weight"], sd[p + ".dwconv_hw.bias"], sd[p + ".dwconv_w.weight"],
            sd[p + ".dwconv_w.bias"], sd[p + ".dwconv_h.weight"], sd[p + ".dwconv_h.bias"], _bn(sd, q))


def _forward(sd, img, pos_index, rnd, return_features):
    sd = to_torch_sd(sd)
    r = rnd or (lambda t: t)
    h = r(img.float())
    maps = []
    for idx, kind, _ci, _co, bn, pool in LAYERS:
        p, q = f"features.{idx}", f"features.{bn}"
        if kind == "c":
            if rnd is None:
                h = F.conv2d(h, sd[p + ".weight"], sd[p + ".bias"], padding=1)
                h = F.relu(F.batch_norm(h, *_bn(sd, q), False, 0.1, BN_EPS))
            else:
                mean, var, gamma, beta = _bn(sd, q)
                s = gamma / torch.sqrt(var + torch.tensor(BN_EPS, dtype=torch.float32))
                w, b = sd[p + ".weight"] * s.view(-1, 1, 1, 1), (sd[p + ".bias"] - mean) * s + beta
                h = F.relu(F.conv2d(h, r(w), b, padding=1))
            if pool:
                h = F.max_pool2d(h, 2, 2)
        elif rnd is None:
            h = idw_reference(h, *_idw_params(sd, p, q))
            if pool:
                h = F.max_pool2d(h, 2, 2)
        else:
            h = idw_layer(h, *idw_fold(*_idw_params(sd, p, q)), pool)
        h = r(h)
        if pool:
            maps.append(h)
    h = r(ggca_combine(ggca_weights(sd), h, "add"))
    maps.append(h)
    lin = None if rnd is None else (lambda inp, w, b=None: F.linear(r(inp), r(w), b))
    out = _tail(sd, h, pos_index, _FF, lin=lin)
    return (out, maps) if return_features else out


@torch.no_grad()
def forward_fp32(sd, img, pos_index=None, return_features=False):
    """cvit_GGCA_ADD_DConv.CViT.forward on normalised fp32 NCHW input.
    return_features: (logits, [the map after each of the five pools, the
    512x7x7 map after x + GGCA(x)])."""
    return _forward(sd, img, pos_index, None, return_features)


@torch.no_grad()
def forward_emulated(sd, img, pos_index=None, dtype="bf16", return_features=False):
    """The gfx950 path's rounding points (module doc), fp32 accumulation everywhere."""
    return _forward(sd, img, pos_index, lambda t: round_to(t, dtype), return_features)
