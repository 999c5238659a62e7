"""CPU reference of the WTConv2d block and of cvit_GGCA_ADD_WTConv
(fac_fake_amd/wtconv.py); test infrastructure, beside dconv_ref.py and
variants_ref.py, whose GGCA and tail it reuses.

The project's own restatement of ``WTConv2d(C, kernel_size=5, wt_levels=1,
wt_type='db1')`` (stride 1, eval mode), functional over the state_dict, on
PyTorch CPU ops:

* ``wt_reference``    the module's op sequence: a stride-2 grouped ``conv2d``
                      with wt_filter, the depthwise 5x5 on the 4C subbands, the
                      scale, a stride-2 grouped ``conv_transpose2d`` with
                      iwt_filter, the depthwise 5x5 with bias on the map, its
                      scale, the add.  Even sides (the reference's pad-and-crop
                      of odd ones is not restated).
* ``wt_fold`` / ``wt_layer``  the same block with the BatchNorm after it the way
                      fac_wtconv computes it: both scales folded into the taps,
                      the bias and the BatchNorm into scale and shift, the 2x2
                      filters as general per-channel operands, sums over shifted
                      zero-padded views in index order, then scale * (u + b) +
                      shift, ReLU, optional 2x2 max-pool.  Usable in float64.
* ``forward_fp32`` / ``forward_emulated``  CViT.forward, with the reference's
                      ops, or with 16-bit rounding where the gfx950 path rounds:
                      the normalised input, the folded 3x3 conv weights, every
                      conv or WT layer's output (after ReLU and pool), x +
                      GGCA(x), and the tail as variants_ref does.  Nothing
                      inside a WT layer is rounded.

Pinned against tests/golden/wtconv_*.npz, which tools/make_golden_wtconv.py
produced from the reference's own module and class.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.cvit_torch import BN_EPS, LN_EPS, round_to, to_torch_sd
from variants_ref import _fold, _layer_weights, _layers, _tail, ggca, ggca_weights

NAME = "cvit_GGCA_ADD_WTConv"
WTCONV_KINDS = "cww cww cww cwww cccc"     # per layer of the base CViT's stem: c Conv2d, w WTConv2d
WT_AT = tuple(i for i, k in enumerate(WTCONV_KINDS.replace(" ", "")) if k == "w")
LAYERS = [((l[0], l[1], "wt", l[4], l[4]) + l[5:]) if i in WT_AT else l
          for i, l in enumerate(_layers((5,), "ccc ccc ccc cccc cccc"))]
GGCA = ("stem", (512, 7, 7), "add")
# (block prefix, the BatchNorm after it, C, H of its input map, pool after it) per WT site
SITES = tuple((f"{l[0]}.{l[1]}", f"{l[0]}.{l[5]}", l[4], h, l[7])
              for l, h in zip([LAYERS[i] for i in WT_AT], (224, 224, 112, 112, 56, 56, 28, 28, 28)))
_LN = ("1.fn.norm", LN_EPS)
PACK_ORDER = ("dwt", "wtaps", "iwt", "btaps", "scale", "shift")
WT_KEYS = ("wt_filter", "iwt_filter", "base_conv.weight", "base_conv.bias", "base_scale.weight", "wavelet_convs.0.weight",
           "wavelet_scale.0.weight")


def wt_reference(x, sd, p, dtype=torch.float32, parts=False):
    """WTConv2d.forward (:269-317, wt_levels 1, stride 1) on NCHW x with even
    sides, evaluated in `dtype` with the ops the module calls.  parts: (the
    wavelet path x_tag, the base path) instead of their sum."""
    f = lambda k: torch.as_tensor(sd[f"{p}.{k}"]).detach().to(dtype)  # noqa: E731
    x = x.to(dtype)
    b, c, h, w = x.shape
    assert h % 2 == 0 and w % 2 == 0
    s = F.conv2d(x, f("wt_filter"), stride=2, groups=c, padding=0).reshape(b, c, 4, h // 2, w // 2)
    t = F.conv2d(s.reshape(b, 4 * c, h // 2, w // 2), f("wavelet_convs.0.weight"), None, padding=2, groups=4 * c)
    t = torch.mul(f("wavelet_scale.0.weight"), t).reshape(b, c, 4, h // 2, w // 2)
    u = F.conv_transpose2d(t.reshape(b, 4 * c, h // 2, w // 2), f("iwt_filter"), stride=2, groups=c, padding=0)
    v = torch.mul(f("base_scale.weight"), F.conv2d(x, f("base_conv.weight"), f("base_conv.bias"), padding=2, groups=c))
    return (u, v) if parts else v + u


def wt_fold(sd, p, q=None, dtype=torch.float32):
    """fac_wtconv's operands in their natural order (wtconv.wt_fold must equal
    this bitwise in fp32): dwt, iwt [c, 4, 2, 2], wtaps [c, 4, 25], btaps [c, 25],
    scale, shift [c].  q None: scale 1, shift = base_scale * bias."""
    f = lambda k: torch.as_tensor(sd[k]).detach().to(dtype)  # noqa: E731
    if any(k.startswith(p + ".wavelet_convs.") and not k.startswith(p + ".wavelet_convs.0.") for k in sd):
        raise ValueError(f"WTConv {p}: more than one wavelet level")
    base = f(p + ".base_conv.weight")
    c = base.shape[0]
    bscale = f(p + ".base_scale.weight").reshape(c)
    ops = dict(dwt=f(p + ".wt_filter").reshape(c, 4, 2, 2).contiguous(),
               wtaps=(f(p + ".wavelet_convs.0.weight").reshape(4 * c, 25) *
                      f(p + ".wavelet_scale.0.weight").reshape(4 * c, 1)).reshape(c, 4, 25).contiguous(),
               iwt=f(p + ".iwt_filter").reshape(c, 4, 2, 2).contiguous(),
               btaps=(base.reshape(c, 25) * bscale.view(c, 1)).contiguous())
    if q is None:
        scale, shift = torch.ones(c, dtype=dtype), torch.zeros(c, dtype=dtype)
    else:
        scale = f(q + ".weight") / torch.sqrt(f(q + ".running_var") + BN_EPS)
        shift = f(q + ".bias") - f(q + ".running_mean") * scale
    ops["scale"] = scale.contiguous()
    ops["shift"] = (shift + bscale * f(p + ".base_conv.bias") * scale).contiguous()
    return ops


def _dw5(x, taps, dtype):
    """Depthwise 5x5 of NCHW x with taps [C, 25], zero padding 2: the sum over the taps in index order."""
    N, C, H, W = x.shape
    xp = F.pad(x, (2, 2, 2, 2))
    acc = torch.zeros(N, C, H, W, dtype=dtype)
    for t in range(25):
        acc = acc + taps[:, t].view(1, C, 1, 1) * xp[:, :, t // 5:t // 5 + H, t % 5:t % 5 + W]
    return acc


def wt_layer(x, ops, pool=False, dtype=torch.float32, relu=True, parts=False):
    """fac_wtconv's arithmetic on NCHW x (fp32 or, for a test's reference,
    float64) from wt_fold's operands: the four subbands, their 5x5 sums, the
    synthesis, the base 5x5, relu?(scale * (u + b) + shift), optional
    MaxPool2d(2,2).  parts: (u, b) alone."""
    x = x.to(dtype)
    N, C, H, W = x.shape
    assert H % 2 == 0 and W % 2 == 0
    o = {k: v.to(dtype) for k, v in ops.items()}
    u = torch.zeros(N, C, H, W, dtype=dtype)
    for k in range(4):
        s = torch.zeros(N, C, H // 2, W // 2, dtype=dtype)
        for i in range(2):
            for j in range(2):
                s = s + o["dwt"][:, k, i, j].view(1, C, 1, 1) * x[:, :, i::2, j::2]
        t = _dw5(s, o["wtaps"][:, k], dtype)
        for i in range(2):
            for j in range(2):
                u[:, :, i::2, j::2] += o["iwt"][:, k, i, j].view(1, C, 1, 1) * t
    b = _dw5(x, o["btaps"], dtype)
    if parts:
        return u, b
    y = o["scale"].view(1, C, 1, 1) * (u + b) + o["shift"].view(1, C, 1, 1)
    if relu:
        y = F.relu(y)
    return F.max_pool2d(y, 2, 2) if pool else y


def _bn_of(layer):
    return f"{layer[0]}.{layer[5]}"


def _forward(sd, img, pos_index, rnd, return_features):
    sd = to_torch_sd(sd)
    r = rnd or (lambda t: t)
    h = r(img.float())
    maps = {}
    for layer in LAYERS:
        q = _bn_of(layer)
        if layer[2] == "wt":
            p = f"{layer[0]}.{layer[1]}"
            maps[p + "_in"] = h
            if rnd is None:
                h = wt_reference(h, sd, p)
                h = F.relu(F.batch_norm(h, sd[q + ".running_mean"], sd[q + ".running_var"], sd[q + ".weight"],
                                        sd[q + ".bias"], False, 0.1, BN_EPS))
                if layer[7]:
                    h = F.max_pool2d(h, 2, 2)
            else:
                h = r(wt_layer(h, wt_fold(sd, p, q), layer[7]))
            maps[p] = h
            continue
        if rnd is None:
            w, b = _layer_weights(sd, layer)
            h = F.conv2d(h, w, b, padding=1)
            h = F.batch_norm(h, sd[q + ".running_mean"], sd[q + ".running_var"], sd[q + ".weight"], sd[q + ".bias"],
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
    """cvit_GGCA_ADD_WTConv.CViT.forward on normalised fp32 NCHW input.  return_features: (logits,
    {"<block>_in", "<block>": each WT site's input map and its output after BatchNorm, ReLU and pool})."""
    return _forward(sd, img, pos_index, None, return_features)


@torch.no_grad()
def forward_emulated(sd, img, pos_index=None, dtype="bf16", return_features=False):
    """The gfx950 path's rounding points (module doc), fp32 accumulation everywhere."""
    return _forward(sd, img, pos_index, lambda t: round_to(t, dtype), return_features)
