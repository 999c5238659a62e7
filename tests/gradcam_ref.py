"""Torch restatement of Grad-CAM (CViT-main/figure/utils.py:57-166 on
gradcam_cnn.py's target layer) for the base CViT and the RepBn8 variant, from
the pre-ReLU map A [B,512,14,14] on; a helper, not collected as a test.  torch
only: nothing here loads the library.  The gradient comes from autograd.

* ``prec``: torch.float32 or torch.float64, the arithmetic everything runs in.
* ``dtype``: None, or "fp16" / "bf16" to round where the gfx950 forward rounds
  (the GGCA-weighted features, every GEMM input, the 16-bit weight matrices).
  Roundings of activations are straight-through, ``x + (round(x) - x).detach()``:
  the value is the rounded one, the gradient passes unchanged.
* per-kernel references (``dgrad``, ``ln_bwd``, ``attention_bwd``, ``gelu_bwd``,
  ``head_bwd``, ``ggca_mul_bwd``, ``relu_pool_bwd``) are autograd of the forward
  op on given inputs, for the GPU tests of each backward kernel on its own.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cvit_torch as C
from oracle import repbn8_torch as R
from oracle.cvit_torch import LN_EPS, _pos_rows, _transformer
from oracle.repbn8_torch import FF_LN_EPS, ggca

GOLDEN = Path(__file__).resolve().parent / "golden"
T16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
MODELS = {"cvit": dict(ff_norm="1.fn.norm", ff_eps=LN_EPS, ggca=False),
          "repbn8": dict(ff_norm="1.fn.norm.norm1", ff_eps=FF_LN_EPS, ggca=True)}
TAIL_PREFIXES = ("pos_embedding", "cls_token", "patch_to_embedding.", "transformer.", "mlp_head.", "ggca.")


CROP_SEED = 5


def crops_of(src):
    """The uint8 crops [n,224,224,3] a Grad-CAM fixture's crop_src names (tools/make_golden_gradcam.py): -1, -2 =
    the two real crops of golden_real.npz, n >= 0 = crop n of make_crops(8, seed=5)."""
    from fac_fake_amd.weights import make_crops
    real = np.load(GOLDEN / "golden_real.npz")["crops"]
    pool = make_crops(8, seed=CROP_SEED)
    return np.stack([real[-1 - int(s)] if s < 0 else pool[int(s)] for s in src])


def rnd(t: torch.Tensor, dtype) -> torch.Tensor:
    """Round to the 16-bit type, keeping t's own precision (a constant: no gradient)."""
    return t if dtype is None else t.detach().to(T16[dtype]).to(t.dtype)


def ste(t: torch.Tensor, dtype) -> torch.Tensor:
    """Straight-through rounding."""
    return t if dtype is None else t + (rnd(t, dtype) - t).detach()


def tail_sd(sd, prec=torch.float32) -> dict:
    """The tensors the tail and GGCA read, in `prec`."""
    return {k: torch.as_tensor(v).to(prec) for k, v in sd.items()
            if k.startswith(TAIL_PREFIXES) and not k.endswith("num_batches_tracked")}


@torch.no_grad()
def premap(sd, img, model: str, dtype=None) -> torch.Tensor:
    """The target layer's output, fp32 [B,512,14,14]: the conv stack up to the last BatchNorm, before its ReLU
    and max-pool.  dtype None: the reference's ops (conv, eval BatchNorm, ReLU, pool) in fp32; "fp16" / "bf16":
    the gfx950 path's rounding points (oracle forward_emulated's), the map itself stored in 16 bits."""
    sd = C.to_torch_sd(sd)
    h = rnd(torch.as_tensor(img).float(), dtype)
    if model == "cvit":
        layers = [(f"features.{ci}", f"features.{bi}", True, i in C.POOL_AFTER, (ci, bi))
                  for i, (ci, bi) in enumerate(C.stem_indices())]
    else:
        layers = [(f"{L[0]}.{L[1]}", None if L[5] is None else f"{L[0]}.{L[5]}", L[6], L[7], L) for L in R.LAYERS]
    for i, (p, q, relu, pool, key) in enumerate(layers):
        if dtype is None:
            w, b = (sd[p + ".weight"], sd[p + ".bias"]) if model == "cvit" else R.layer_weights(sd, key)
            h = F.conv2d(h, w, b, padding=1)
            if q is not None:
                h = F.batch_norm(h, sd[q + ".running_mean"], sd[q + ".running_var"], sd[q + ".weight"],
                                 sd[q + ".bias"], False, 0.1, C.BN_EPS)
        else:
            w, b = C.fold_bn(sd, *key) if model == "cvit" else R.fold_layer(sd, key)
            h = F.conv2d(h, rnd(w, dtype), b, padding=1)
        if i == len(layers) - 1:
            return rnd(h, dtype)
        if relu:
            h = F.relu(h)
        if pool:
            h = F.max_pool2d(h, 2, 2)
        h = rnd(h, dtype)


def tail_logits(tsd, feat, pos_index, model: str, dtype=None, head_mask=None):
    """Pooled stem output [B,512,7,7] (after x * GGCA(x) for RepBn8) -> logits (cvit.py:170-179).
    head_mask (bool [B,2048]): the head's ReLU decisions are taken from it instead of from the hidden layer's
    own sign (for comparing gradients with a forward that made these decisions)."""
    cfg = MODELS[model]
    B = feat.shape[0]

    def lin(inp, w, b=None):
        return F.linear(ste(inp, dtype), rnd(w, dtype), b)
    y = feat.permute(0, 2, 3, 1).reshape(B, 1, -1)
    y = lin(y, tsd["patch_to_embedding.weight"], tsd["patch_to_embedding.bias"])
    x = torch.cat((tsd["cls_token"].expand(B, -1, -1), y), 1) + _pos_rows(tsd, pos_index, B)
    x = _transformer(tsd, x, lin=lin, ff_norm=cfg["ff_norm"], ff_eps=cfg["ff_eps"])
    pre = lin(x[:, 0], tsd["mlp_head.0.weight"], tsd["mlp_head.0.bias"])
    hid = F.relu(pre) if head_mask is None else pre * head_mask.to(pre.dtype)
    return F.linear(hid, tsd["mlp_head.2.weight"], tsd["mlp_head.2.bias"])


def ggca_mul(tsd, x):
    """x * GGCA(x) (cvit_GGCA_ADD_DEConv_RepBn8.py:436-437) on [B,512,7,7]."""
    return x * ggca(tsd, x)


def relu_pool(a):
    return F.max_pool2d(F.relu(a), 2, 2)


def features_from_map(tsd, a, model: str, dtype=None):
    f = relu_pool(a)
    if MODELS[model]["ggca"]:
        f = ste(ggca_mul(tsd, f), dtype)
    return f


def targets_of(logits, target_category):
    B = logits.shape[0]
    if target_category is None:
        return logits.detach().argmax(-1)
    if isinstance(target_category, int):
        return torch.full((B,), target_category, dtype=torch.long)
    t = torch.as_tensor(target_category, dtype=torch.long)
    assert t.shape == (B,)
    return t


def grad_of_target(logits, wrt, target_category):
    """GradCAM.get_loss (utils.py:80-85): the sum of output[i, target[i]], differentiated."""
    t = targets_of(logits, target_category)
    loss = logits.gather(1, t.view(-1, 1)).sum()
    return torch.autograd.grad(loss, wrt)[0]


# ---------------------------------------------------------------- the CAM arithmetic
def bilinear_resize(img: torch.Tensor, size: int) -> torch.Tensor:
    """cv2.resize(img, (size, size)) with its default INTER_LINEAR, restated for [n, s, s] maps when upscaling:
    source coordinate (dst + 0.5) * s / size - 0.5, floor, the fraction; a sample left of the first or right of
    the last centre takes the edge value."""
    n, s, _ = img.shape
    src = (torch.arange(size, dtype=img.dtype) + 0.5) * (s / size) - 0.5
    i0 = torch.floor(src)
    fr = src - i0
    i0 = i0.long()
    fr = torch.where(i0 < 0, torch.zeros_like(fr), fr)
    i0 = i0.clamp_min(0)
    fr = torch.where(i0 >= s - 1, torch.zeros_like(fr), fr)
    i0 = i0.clamp_max(s - 1)
    i1 = (i0 + 1).clamp_max(s - 1)
    rows = img[:, i0, :] * (1 - fr).view(1, -1, 1) + img[:, i1, :] * fr.view(1, -1, 1)
    return rows[:, :, i0] * (1 - fr).view(1, 1, -1) + rows[:, :, i1] * fr.view(1, 1, -1)


def scale_minmax(img: torch.Tensor) -> torch.Tensor:
    """scale_cam_image's two lines per map (utils.py:127-128)."""
    flat = img.reshape(img.shape[0], -1)
    flat = flat - flat.min(1, keepdim=True).values
    return (flat / (1e-7 + flat.max(1, keepdim=True).values)).reshape(img.shape)


def cam_from(a: torch.Tensor, g: torch.Tensor, size: int = 224, resize=None):
    """utils.py:76-134,165-166 on activations a and gradients g [B,512,14,14] -> (w [B,512], cam14, heatmap)."""
    w = g.mean((2, 3))
    cam = (w[:, :, None, None] * a).sum(1).clamp_min(0)
    cam14 = scale_minmax(cam)
    if resize is None:
        up = F.interpolate(cam14[:, None], size=(size, size), mode="bilinear", align_corners=False)[:, 0]
    else:
        up = resize(cam14, size)
    return w, cam14, scale_minmax(up.clamp_min(0))


def gradcam(sd, a, model: str, target_category=None, pos_index=None, dtype=None, prec=torch.float32):
    """From the pre-ReLU map a [B,512,14,14]: dict(logits, grad [B,512,14,14], grad_feat (w.r.t. what enters
    the patch embedding), w, cam14, heatmap), all detached in `prec`."""
    tsd = tail_sd(sd, prec)
    a = torch.as_tensor(a).detach().to(prec).requires_grad_(True)
    f = features_from_map(tsd, a, model, dtype)
    f.retain_grad()
    logits = tail_logits(tsd, f, pos_index, model, dtype)
    t = targets_of(logits, target_category)
    logits.gather(1, t.view(-1, 1)).sum().backward()
    g = a.grad.detach()
    w, cam14, heat = cam_from(a.detach(), g)
    return dict(logits=logits.detach(), grad=g, grad_feat=f.grad.detach(), w=w, cam14=cam14, heatmap=heat,
                target=t)


# ---------------------------------------------------------------- per-kernel references
def _leaf(t, prec):
    return torch.as_tensor(t).detach().to(prec).requires_grad_(True)


def dgrad(dy, w, prec=torch.float64):
    """dX = dY . W for y = x . W^T."""
    return dy.to(prec) @ w.to(prec)


def ln_bwd(x, gamma, eps, dy, prec=torch.float64):
    xl = _leaf(x, prec)
    y = F.layer_norm(xl, (xl.shape[-1],), gamma.to(prec), None, eps)
    return torch.autograd.grad(y, xl, dy.to(prec))[0]


def attention_fwd(qkv, scale):
    """attention2's contract: qkv [2B][3072] '(qkv h d)', 8 heads x 128, two tokens per crop -> [2B][1024]."""
    R = qkv.shape[0]
    q, k, v = qkv.view(R // 2, 2, 3, 8, 128).permute(2, 0, 3, 1, 4)
    att = (torch.einsum("bhid,bhjd->bhij", q, k) * scale).softmax(-1)
    return torch.einsum("bhij,bhjd->bhid", att, v).permute(0, 2, 1, 3).reshape(R, 1024)


def attention_bwd(qkv, do, scale, prec=torch.float64):
    ql = _leaf(qkv, prec)
    return torch.autograd.grad(attention_fwd(ql, scale), ql, do.to(prec))[0]


def gelu_bwd(pre, dh, prec=torch.float64):
    pl = _leaf(pre, prec)
    return torch.autograd.grad(F.gelu(pl), pl, dh.to(prec))[0]


def head_bwd(hid, w2, target, prec=torch.float64):
    """d logits[b][t_b] / d hid_pre through the ReLU: hid is the ReLU'd vector (its sign is the mask)."""
    t = torch.as_tensor(target, dtype=torch.long)
    return w2.to(prec)[t] * (hid > 0).to(prec)


def ggca_mul_bwd(tsd, x, g, prec=torch.float64):
    tsd = {k: v.to(prec) for k, v in tsd.items() if k.startswith("ggca.")}
    xl = _leaf(x, prec)
    return torch.autograd.grad(ggca_mul(tsd, xl), xl, g.to(prec))[0]


def relu_pool_bwd(a, dp, prec=torch.float64):
    al = _leaf(a, prec)
    return torch.autograd.grad(relu_pool(al), al, dp.to(prec))[0]


def rel_err(got, ref64) -> float:
    """max|got - ref| / max|ref|, the metric of every gradient check."""
    ref64 = ref64.double()
    return float((got.double() - ref64).abs().max() / ref64.abs().max().clamp_min(1e-300))
