"""CPU restatement of ResKan (CViT-main/ResKan/kan_resnet.py::resnet34 with
include_top_kan), functional over a state_dict with the PyTorch CPU ops the
reference modules call.  Test infrastructure: never shipped or measured.

* ``forward_fp32`` / ``features_fp32`` - ``ResNet.forward`` (kan_resnet.py:
  225-256): 7x7/2 conv, BN, ReLU, 3x3/2 max-pool, BasicBlock x [3,4,6,3]
  (:38-65: conv1 + bn1 + ReLU, conv2 + bn2, + identity, ReLU), global average
  pool, KAN([512, 64, 2]).  Pinned against the reference module's outputs
  (tests/golden/reskan_golden_stages.npz, tools/make_golden_reskan.py).
* ``forward_emulated`` / ``features_emulated`` - the gfx950 path's rounding
  points: 16-bit input, folded 16-bit weights, fp32 accumulation and bias,
  every conv output rounded once to 16 bits (the second conv after the fp32
  residual add and ReLU), the pool and the KAN in fp32.

``taps``: the max-pool output, the 16 block outputs (NCHW) and the pooled
features [B, 512]: 18 tensors.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.cvit_torch import round_to, to_torch_sd
from oracle.resvitkan_torch import kan_linear_fp32

from fac_fake_amd.weights import resnet34_blocks

BN_EPS = 1e-5          # nn.BatchNorm2d default (kan_resnet.py:29, :34, :166, :206)


def _bn(sd, p, h):
    return F.batch_norm(h, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"],
                        False, 0.1, BN_EPS)


def basic_block_fp32(sd, p: str, x: torch.Tensor, stride: int, ds: bool) -> torch.Tensor:
    """BasicBlock.forward (kan_resnet.py:38-65)."""
    identity = _bn(sd, p + ".downsample.1", F.conv2d(x, sd[p + ".downsample.0.weight"], stride=stride)) if ds else x
    out = F.relu(_bn(sd, p + ".bn1", F.conv2d(x, sd[p + ".conv1.weight"], stride=stride, padding=1)))
    out = _bn(sd, p + ".bn2", F.conv2d(out, sd[p + ".conv2.weight"], padding=1))
    return F.relu(out + identity)


def _kan(sd, f):
    return kan_linear_fp32(sd, "kan.layers.1", kan_linear_fp32(sd, "kan.layers.0", f))


@torch.no_grad()
def features_fp32(sd, img: torch.Tensor, taps: list | None = None) -> torch.Tensor:
    sd = to_torch_sd(sd)
    tap = taps.append if taps is not None else (lambda t: None)
    x = F.relu(_bn(sd, "bn1", F.conv2d(img.float(), sd["conv1.weight"], stride=2, padding=3)))
    x = F.max_pool2d(x, 3, 2, 1)
    tap(x)
    for p, _i, _c, s, ds in resnet34_blocks():
        x = basic_block_fp32(sd, p, x, s, ds)
        tap(x)
    f = torch.flatten(F.adaptive_avg_pool2d(x, (1, 1)), 1)
    tap(f)
    return f


@torch.no_grad()
def forward_fp32(sd, img: torch.Tensor) -> torch.Tensor:
    sd = to_torch_sd(sd)
    return _kan(sd, features_fp32(sd, img))


def fold_bn(sd, conv_key: str, bn_prefix: str):
    s = sd[bn_prefix + ".weight"] / torch.sqrt(sd[bn_prefix + ".running_var"] + torch.tensor(BN_EPS))
    return sd[conv_key] * s.view(-1, 1, 1, 1), (torch.zeros_like(s) - sd[bn_prefix + ".running_mean"]) * s + \
        sd[bn_prefix + ".bias"]


def folded_block(sd, p: str, x: torch.Tensor, stride: int, ds: bool, r=lambda t: t) -> torch.Tensor:
    """The block as the HIP path computes it: BN folded into the convs, conv2's
    epilogue = + bias (bn2), + identity, ReLU, in that order; `r` rounds
    weights and stored activations (identity: the fp32 folded form)."""
    def conv(h, ck, bnp, stride=1, pad=0):
        w, b = fold_bn(sd, ck, bnp)
        return F.conv2d(h, r(w), b, stride=stride, padding=pad)

    identity = r(conv(x, p + ".downsample.0.weight", p + ".downsample.1", stride)) if ds else x
    h = r(F.relu(conv(x, p + ".conv1.weight", p + ".bn1", stride, 1)))
    return r(F.relu(conv(h, p + ".conv2.weight", p + ".bn2", 1, 1) + identity))


@torch.no_grad()
def features_emulated(sd, img: torch.Tensor, dtype: str = "bf16", taps: list | None = None) -> torch.Tensor:
    sd = to_torch_sd(sd)
    tap = taps.append if taps is not None else (lambda t: None)
    r = lambda t: round_to(t, dtype)  # noqa: E731
    w, b = fold_bn(sd, "conv1.weight", "bn1")
    x = r(F.relu(F.conv2d(r(img.float()), r(w), b, stride=2, padding=3)))
    x = F.max_pool2d(x, 3, 2, 1)
    tap(x)
    for p, _i, _c, s, ds in resnet34_blocks():
        x = folded_block(sd, p, x, s, ds, r)
        tap(x)
    f = x.mean(dim=(2, 3))                       # fp32 mean of the 16-bit map, never rounded
    tap(f)
    return f


@torch.no_grad()
def forward_emulated(sd, img: torch.Tensor, dtype: str = "bf16") -> torch.Tensor:
    sd = to_torch_sd(sd)
    return _kan(sd, features_emulated(sd, img, dtype))


def tap_means(taps) -> list:
    """Per-channel means [B, C] (float64 numpy) of the 18 taps."""
    return [(t.double().mean(dim=(2, 3)) if t.dim() == 4 else t.double()).numpy() for t in taps]


__all__ = ["features_fp32", "forward_fp32", "features_emulated", "forward_emulated", "basic_block_fp32",
           "folded_block", "fold_bn", "tap_means"]
