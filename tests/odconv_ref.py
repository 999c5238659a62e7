"""CPU reference of the ODConv2d block and of cvit_GGCA_ADD_ODConv /
cvit_GGCA_ODConv (fac_fake_amd/odconv.py); test infrastructure, beside
scconv_ref.py and variants_ref.py, whose stem walk, GGCA and tail it reuses.

The project's own restatement of ``ODConv2d(C, C, 3, padding=1)`` (kernel_num 4,
attention width 16, temperature 1, no bias, eval mode), written from the
block's formula, functional over the state_dict, on PyTorch CPU ops.  Per crop b:

    p   = mean over h x w of x[b]                                   [C]
    hid = ReLU(bn_scale (fc p) + bn_shift)                          [16]
    ca  = sigmoid(channel_fc hid + channel_b)  [C]    fa = sigmoid(filter_fc hid + filter_b)  [C]
    sa  = sigmoid(spatial_fc hid + spatial_b)  [9]    ka = softmax(kernel_fc hid + kernel_b)  [4]
    out[b,o,y,x] = fa[o] sum_tap sa[tap] sum_i (sum_k ka[k] W[k,o,i,tap]) ca[i] x[b,i,y+dy,x+dx]

* ``odconv_fold``     the block's state_dict entries, its attention's BatchNorm
                      and the BatchNorm that follows it as fac_odconv_pack's
                      operands.
* ``attentions``      (ca, fa, sa, ka) of NCHW x.
* ``aggregate``       the per-crop weight sa[tap] ca[i] sum_k ka[k] W_k, [B, C, C, 3, 3].
* ``odconv_block``    ODConv -> scale, shift -> optional ReLU -> optional 2x2
                      max-pool in float64 or fp32, optionally with odconv.hip's
                      declared roundings: the aggregated weight, once, and the
                      output (the caller rounds the input).
* ``forward_fp32`` / ``forward_emulated``  CViT.forward of either class.

Pinned against tests/golden/odconv_*.npz, which tools/make_golden_odconv.py
produced from the reference's own module and classes.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.cvit_torch import BN_EPS, LN_EPS, round_to, to_torch_sd
from variants_ref import _fold, _layer_weights, _layers, _tail, ggca, ggca_weights

NAMES = ("cvit_GGCA_ADD_ODConv", "cvit_GGCA_ODConv")
OD_AT = (4, 7, 10, 12)            # the convs of the plain (4, 1) stem that are ODConv blocks in cvit_GGCA_ADD_ODConv
_PLAIN = _layers((4, 1), "ccc ccc ccc cccc cccc")
LAYERS = {NAMES[0]: [((l[0], l[1], "od", l[4], l[4]) + l[5:]) if i in OD_AT else l for i, l in enumerate(_PLAIN)],
          NAMES[1]: list(_PLAIN)}
GGCA = {NAMES[0]: ("stem", (512, 7, 7), "add"), NAMES[1]: ("stem", (512, 7, 7), "att")}
BARE = {NAMES[0]: None, NAMES[1]: ("features1", 256)}       # the bare top-level odconv's site
# (block prefix, the BatchNorm after it or None, C, H of its input map, pool after it) per ODConv site that runs
SITES = {NAMES[0]: (("features1.13", "features1.14", 64, 112, False), ("features1.23", "features1.24", 128, 56, False),
                    ("features1.33", "features1.34", 256, 28, False), ("features1.39", "features1.40", 256, 28, True)),
         NAMES[1]: (("odconv", None, 256, 14, False),)}
_LN = ("1.fn.norm", LN_EPS)
PACK_ORDER = ("weight", "fc", "bn_scale", "bn_shift", "channel_fc", "channel_b", "filter_fc", "filter_b", "spatial_fc",
              "spatial_b", "kernel_fc", "kernel_b", "scale", "shift")
KERNEL_NUM, ATT_WIDTH = 4, 16


def odconv_fold(sd, prefix, bn_prefix=None, dtype=torch.float32):
    """fac_odconv_pack's operands from the state_dict (odconv.odconv_fold must
    equal this bitwise in fp32).  bn_prefix None: scale 1, shift 0 (the bare
    block).  ValueError where kernel_num is not 4."""
    f = lambda k: torch.as_tensor(sd[k]).detach().to(dtype)  # noqa: E731
    p, a = prefix + ".", prefix + ".attention."
    w = f(p + "weight")
    if w.dim() != 5 or w.shape[0] != KERNEL_NUM:
        raise ValueError(f"ODConv {prefix}: expected a weight [4, c, c, 3, 3], got {list(w.shape)}")
    c = w.shape[1]
    s = f(a + "bn.weight") / torch.sqrt(f(a + "bn.running_var") + BN_EPS)
    ops = dict(weight=w.contiguous(), fc=f(a + "fc.weight").flatten(1).contiguous(), bn_scale=s.contiguous(),
               bn_shift=(f(a + "bn.bias") - f(a + "bn.running_mean") * s).contiguous())
    for head in ("channel", "filter", "spatial", "kernel"):
        ops[head + "_fc"] = f(a + head + "_fc.weight").flatten(1).contiguous()
        ops[head + "_b"] = f(a + head + "_fc.bias").contiguous()
    if bn_prefix is None:
        ops["scale"], ops["shift"] = torch.ones(c, dtype=dtype), torch.zeros(c, dtype=dtype)
    else:
        q = bn_prefix + "."
        s = f(q + "weight") / torch.sqrt(f(q + "running_var") + BN_EPS)
        ops["scale"], ops["shift"] = s.contiguous(), (f(q + "bias") - f(q + "running_mean") * s).contiguous()
    return ops


def attentions(x, ops, dtype=torch.float64):
    """(ca [B, C], fa [B, C], sa [B, 9], ka [B, 4]) of NCHW x, evaluated in `dtype` with torch's tensor ops."""
    o = {k: v.to(dtype) for k, v in ops.items() if k != "weight"}
    p = x.to(dtype).mean((2, 3))
    hid = F.relu((p @ o["fc"].t()) * o["bn_scale"] + o["bn_shift"])
    head = lambda n: hid @ o[n + "_fc"].t() + o[n + "_b"]  # noqa: E731
    return (torch.sigmoid(head("channel")), torch.sigmoid(head("filter")), torch.sigmoid(head("spatial")),
            torch.softmax(head("kernel"), 1))


def aggregate(ops, ca, sa, ka, dtype=torch.float64):
    """[B, C, C, 3, 3]: sa[tap] ca[i] sum_k ka[k] W[k, o, i, tap]."""
    w = torch.einsum("bk,koiyx->boiyx", ka.to(dtype), ops["weight"].to(dtype))
    B, C = ca.shape
    return w * sa.to(dtype).view(B, 1, 1, 3, 3) * ca.to(dtype).view(B, 1, C, 1, 1)


def odconv_block(x, ops, dtype=torch.float64, round=None, relu=True, pool=False, parts=False, raw=False):
    """act(ODConv(x) * scale + shift) -> optional 2x2 max-pool on NCHW x.  round:
    None, or "fp16" / "bf16" for odconv.hip's declared roundings (dtype must then
    be fp32; the caller rounds the input): the aggregated weight and the output.
    parts: also dict(ca, fa, sa, ka).  raw: ODConv(x) alone, what the reference
    module returns."""
    assert round is None or dtype == torch.float32
    r = (lambda v: round_to(v, round)) if round else (lambda v: v)
    B, C, H, W = x.shape
    x = x.to(dtype)
    ca, fa, sa, ka = attentions(x, ops, dtype)
    wagg = r(aggregate(ops, ca, sa, ka, dtype))
    out = F.conv2d(x.reshape(1, B * C, H, W), wagg.reshape(B * C, C, 3, 3), padding=1, groups=B).view(B, C, H, W)
    out = out * fa.view(B, C, 1, 1)
    att = dict(ca=ca, fa=fa, sa=sa, ka=ka)
    if raw:
        return (out, att) if parts else out
    out = out * ops["scale"].to(dtype).view(1, C, 1, 1) + ops["shift"].to(dtype).view(1, C, 1, 1)
    if relu:
        out = F.relu(out)
    out = r(out)
    if pool:
        out = F.max_pool2d(out, 2, 2)
    return (out, att) if parts else out


def att_row(att):
    """[B, 2C + 13]: ca | fa | sa | ka, fac_odconv's att_out."""
    return torch.cat([att["ca"], att["fa"], att["sa"], att["ka"]], 1)


def _bn_of(layer):
    return f"{layer[0]}.{layer[5]}"


def _forward(name, sd, img, pos_index, rnd, return_features):
    sd = to_torch_sd(sd)
    r = rnd[0] if rnd else (lambda t: t)
    rd = rnd[1] if rnd else None
    h = r(img.float())
    maps = {}
    layers = LAYERS[name]
    bare = BARE[name]
    bare_at = max(i for i, l in enumerate(layers) if l[0] == bare[0]) if bare else None
    for i, layer in enumerate(layers):
        if layer[2] == "od":
            p = f"{layer[0]}.{layer[1]}"
            maps[p + "_in"] = h
            h = maps[p] = odconv_block(h, odconv_fold(sd, p, _bn_of(layer)), torch.float32, round=rd, pool=layer[7])
        else:
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
        if i == bare_at:
            maps["odconv_in"] = h
            h = maps["odconv"] = odconv_block(h, odconv_fold(sd, "odconv"), torch.float32, round=rd, relu=False)
    maps["ggca_in"] = h
    g = ggca(ggca_weights(sd), h)
    h = maps["ggca"] = r(h + g if GGCA[name][2] == "add" else g)
    lin = None if rnd is None else (lambda inp, w, b=None: F.linear(r(inp), r(w), b))
    out = _tail(sd, h, pos_index, _LN, lin=lin)
    return (out, maps) if return_features else out


@torch.no_grad()
def forward_fp32(name, sd, img, pos_index=None, return_features=False):
    """CViT.forward of model/other/<name>.py on normalised fp32 NCHW input.  return_features: (logits,
    {"<block>_in", "<block>": each ODConv site's input map and its output after BatchNorm, ReLU and pool})."""
    return _forward(name, sd, img, pos_index, None, return_features)


@torch.no_grad()
def forward_emulated(name, sd, img, pos_index=None, dtype="bf16", return_features=False):
    """The gfx950 path's rounding points (variants_ref's, odconv_block's declared ones), fp32 accumulation everywhere."""
    return _forward(name, sd, img, pos_index, (lambda t: round_to(t, dtype), dtype), return_features)
