"""CPU restatement of msca_S3D (sx_exp_deepfakedetect-master/S3D/msca_S3D.py:17-72,
new_model/iformer_3d.py, msca_3d.py, Conv3d.py) for the tests; a helper, not
collected as a test.  Written from the layer description, functional over a
state_dict, on [B, C, T, H, W] tensors:

* ``features`` / ``forward``  - the reference's arithmetic in the dtype of the
  state_dict handed in (``cast_sd``: fp64 is the truth the kernels are measured
  against, fp32 what the reference module itself computes);
* ``features_emulated`` / ``forward_emulated`` - the gfx950 path's rounding
  points: 16-bit input, BN-folded 16-bit weights of the dense convs, fp32
  depthwise weights and BatchNorm tables, and a 16-bit rounding wherever the
  HIP path writes a tensor (after every conv, every fac_dwsep3d, every fac_ew
  step and the BN-pool).
* ``dwsep_cl`` / ``bn_pool_cl`` / ``EW`` - the single ops on channels-last maps.

``ablate`` names a part replaced by the identity (or a swapped concat), for the
fixture generator's margins; ``bn_hook(prefix, x)`` is called before every
BatchNorm (tools/calibrate_msca_s3d.py sets its running statistics there).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from fac_fake_amd.weights import msca_s3d_base
from oracle.cvit_torch import round_to, to_torch_sd

BN_EPS = 1e-3
ABLATIONS = ("gate", "w5", "w7", "mlp", "gelu", "swap")


def cast_sd(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in to_torch_sd(sd).items()}


def gelu(x):
    return x * 0.5 * (1 + torch.erf(x * math.sqrt(0.5)))


def bn_affine(sd, p):
    s = sd[p + ".weight"] / torch.sqrt(sd[p + ".running_var"] + BN_EPS)
    return s, sd[p + ".bias"] - sd[p + ".running_mean"] * s


class _Net:
    """The reference's arithmetic, in the state_dict's dtype."""

    def __init__(self, sd, ablate=None, bn_hook=None, sites=None):
        self.sd, self.ablate, self.bn_hook, self.sites = sd, ablate or {}, bn_hook, sites

    def off(self, p, what):
        return self.ablate.get(p) == what

    def bn(self, p, x):
        if self.bn_hook is not None:
            self.bn_hook(p, x)
        s, b = bn_affine(self.sd, p)
        return x * s.view(1, -1, 1, 1, 1) + b.view(1, -1, 1, 1, 1)

    def relu6(self, p, x):
        if self.sites is not None:   # pre-activation statistics of a ReLU6 site
            self.sites.append((p, float((x > 6).double().mean()), float((x < 0).double().mean())))
        if self.ablate.get("relu") == p:   # plain ReLU at this one site
            return x.clamp(min=0)
        return x.clamp(0, 6)

    def basic(self, p, x):
        return self.relu6(p, self.bn(p + ".bn", F.conv3d(x, self.sd[p + ".conv.weight"])))

    def sep(self, p, x, s, pd, v2=False):
        x = F.conv3d(x, self.sd[p + ".conv_s.weight"], stride=(1, s, s), padding=(0, pd, pd))
        if not v2:
            x = self.relu6(p + ".s", self.bn(p + ".bn_s", x))
        x = F.conv3d(x, self.sd[p + ".conv_t.weight"], stride=(s, 1, 1), padding=(pd, 0, 0))
        return self.relu6(p + ".t", self.bn(p + ".bn_t", x))

    def dwsep(self, p, x):
        ws, wt = self.sd[p + ".conv_s.weight"], self.sd[p + ".conv_t.weight"]
        c, k, kt = ws.shape[0], ws.shape[3], wt.shape[2]
        x = F.conv3d(x, ws, padding=(0, k // 2, k // 2), groups=c)
        x = F.conv3d(x, wt, padding=(kt // 2, 0, 0), groups=c)
        return self.relu6(p, self.bn(p + ".bn_t", x))

    def conv_b(self, p, x):
        return F.conv3d(x, self.sd[p + ".weight"], self.sd[p + ".bias"])

    def gelu(self, x, gelu_in=None):
        if gelu_in is not None:
            gelu_in.append(float((x < 0).double().mean()))
        return gelu(x)

    def mixer(self, p, n, low, kt, gelu_in=None):
        c = n.shape[1]
        h = (c - low) // 2
        m, a = p + ".inceptionmixer", p + ".inceptionmixer.attn"
        g = a + ".spatial_gating_unit"
        yh1 = self.basic(m + ".maxpool_fc.1", F.max_pool3d(n[:, :h], (kt, 3, 3), 1, (kt // 2, 1, 1)))
        yh2 = self.bn(m + ".fc_dw.2", self.dwsep(m + ".fc_dw.1", self.basic(m + ".fc_dw.0", n[:, h:2 * h])))
        u = self.gelu(self.conv_b(a + ".proj_1", n[:, c - low:]), gelu_in)
        at = self.dwsep(g + ".conv0", u)
        t5 = at if self.off(p, "w5") else self.dwsep(g + ".conv0_1", at)
        t7 = at if self.off(p, "w7") else self.dwsep(g + ".conv1_1", at)
        at = self.conv_b(g + ".conv3", at + t5 + t7)
        yl = self.conv_b(a + ".proj_2", at if self.off(p, "gate") else at * u)
        if self.off(p, "swap"):
            return torch.cat([yh1, yh2, yl], 1)
        return torch.cat([yl, yh1, yh2], 1)

    def mlp(self, p, n, gelu_in=None):
        y = self.dwsep(p + ".mlp.dwconv.dwconv", self.conv_b(p + ".mlp.fc1", n))
        return self.conv_b(p + ".mlp.fc2", self.gelu(y, gelu_in))

    def block(self, p, x, L, extra=None, gelu_in=None):
        kind, _, low, kt = L
        mx = self.mixer(p, self.bn(p + ".norm1", x), low, kt, gelu_in)
        x = x + mx
        if extra is not None:
            extra.append(mx)
        if kind == "iformer_light":
            return x if self.off(p, "gelu") else self.gelu(x, gelu_in)
        if self.off(p, "mlp"):
            ml = self.bn(p + ".norm2", x)
        else:
            ml = self.mlp(p, self.bn(p + ".norm2", x), gelu_in)
        if extra is not None:
            extra.append(ml)
        return x + ml

    def mixed(self, p, x, v2):
        y0 = self.basic(p + ".branch0.0", x)
        y1 = self.sep(p + ".branch1.1", self.basic(p + ".branch1.0", x), 1, 1, v2)
        y2 = self.sep(p + ".branch2.1", self.basic(p + ".branch2.0", x), 1, 1, v2)
        y3 = self.basic(p + ".branch3.1", F.max_pool3d(x, 3, 1, 1))
        return torch.cat((y0, y1, y2, y3), 1)


@torch.no_grad()
def features(sd, x, srm: bool, taps=None, extra=None, **kw):
    """`base`; taps: the 21 base[i] outputs; extra: the 18 mixer / mlp outputs."""
    gelu_in = kw.pop("gelu_in", None)
    net = _Net(sd, **kw)
    y = x.to(sd["fc.0.weight"].dtype)
    if srm:
        y = F.conv3d(y, sd["SRM.hpf.weight"], padding=(0, 2, 2))
    for i, L in enumerate(msca_s3d_base(srm)):
        p = f"base.{i}"
        if L[0] == "sep":
            y = net.sep(p, y, L[4], L[5])
        elif L[0] == "basic":
            y = net.basic(p, y)
        elif L[0] == "pool":
            y = F.max_pool3d(y, *L[1:])
        elif L[0] in ("iformer", "iformer_light"):
            y = net.block(p, y, L, extra, gelu_in)
        else:
            y = net.mixed(p, y, L[0] == "mixed_v2")
        if taps is not None:
            taps.append(y)
    return y


@torch.no_grad()
def forward(sd, x, srm: bool, **kw):
    y = features(sd, x, srm, **kw)
    y = F.avg_pool3d(y, (2, y.size(3), y.size(4)), stride=1)
    y = F.conv3d(y, sd["fc.0.weight"], sd["fc.0.bias"])
    return torch.mean(y.view(y.size(0), y.size(1), y.size(2)), 2)


# ------------------------------------------------------------ the folded algebra
def fold_out(sd, ck, bn):
    """conv (no bias) followed by BatchNorm `bn` -> (w, b)."""
    s, t = bn_affine(sd, bn)
    return sd[ck] * s.view(-1, 1, 1, 1, 1), t


def fold_in(w, b, s, t, lo, width):
    """A 1x1x1 conv (w [co, ci, 1, 1, 1], b) reading channels [lo, lo + ci) of
    x * s + t -> (w', b') reading ALL `width` channels of x (zero columns
    outside the slice): w'[:, lo + i] = w[:, i] s[lo + i], b' = b + w t[lo:]."""
    co, ci = w.shape[0], w.shape[1]
    wf = w.new_zeros(co, width, 1, 1, 1)
    wf[:, lo:lo + ci] = w * s[lo:lo + ci].view(1, -1, 1, 1, 1)
    return wf, b + w.reshape(co, ci) @ t[lo:lo + ci]


def rank1_window(ws, wt):
    """dw(1,k,k) then dw(kt,1,1) as one depthwise (kt,k,k) window [c,1,kt,k,k]."""
    return wt * ws


# ------------------------------------------------------------ single ops, channels-last
def dwsep_cl(x, ws, wt, scale, shift, act="none", scale2=None, shift2=None):
    """fac_dwsep3d on x [N,T,H,W,C] (any float dtype; weights cast to it)."""
    dt = x.dtype
    c, k, kt = ws.shape[0], ws.shape[3], wt.shape[2]
    y = F.conv3d(x.permute(0, 4, 1, 2, 3), ws.to(dt), padding=(0, k // 2, k // 2), groups=c)
    y = F.conv3d(y, wt.to(dt), padding=(kt // 2, 0, 0), groups=c).permute(0, 2, 3, 4, 1)
    y = (y * scale.to(dt) + shift.to(dt)).clamp(0, 6)
    if act == "affine2":
        y = y * scale2.to(dt) + shift2.to(dt)
    elif act == "gelu":
        y = gelu(y)
    return y


def bn_pool_cl(x, scale, shift, kt):
    y = (x * scale.to(x.dtype) + shift.to(x.dtype)).permute(0, 4, 1, 2, 3)
    return F.max_pool3d(y, (kt, 3, 3), 1, (kt // 2, 1, 1)).permute(0, 2, 3, 4, 1)


EW = {"gelu": lambda a: gelu(a), "mul": lambda a, b: a * b, "add": lambda a, b: a + b,
      "add_gelu": lambda a, b: gelu(a + b), "clamp6": lambda a: a.clamp(0, 6), "add3": lambda a, b, c: (a + b) + c}


# ------------------------------------------------------------ the HIP path's rounding points
@torch.no_grad()
def features_emulated(sd, x, srm: bool, dtype: str = "fp16", taps=None, extra=None):
    sd = cast_sd(sd, torch.float32)
    r = lambda t: round_to(t, dtype)  # noqa: E731

    def conv(y, w, b, relu6, stride=1, pad=0):
        y = F.conv3d(y, r(w), b, stride=stride, padding=pad)
        return r(y.clamp(0, 6)) if relu6 else r(y)

    def basic(p, y):
        return conv(y, *fold_out(sd, p + ".conv.weight", p + ".bn"), True)

    def sep(p, y, s, pd, v2=False):
        if v2:
            y = conv(y, sd[p + ".conv_s.weight"], None, False, (1, s, s), (0, pd, pd))
        else:
            y = conv(y, *fold_out(sd, p + ".conv_s.weight", p + ".bn_s"), True, (1, s, s), (0, pd, pd))
        return conv(y, *fold_out(sd, p + ".conv_t.weight", p + ".bn_t"), True, (s, 1, 1), (pd, 0, 0))

    def dwsep(p, y, act="none", bn2=None):
        s, t = bn_affine(sd, p + ".bn_t")
        s2, t2 = bn_affine(sd, bn2) if bn2 else (None, None)
        return r(dwsep_cl(y.permute(0, 2, 3, 4, 1), sd[p + ".conv_s.weight"], sd[p + ".conv_t.weight"], s, t, act, s2,
                          t2)).permute(0, 4, 1, 2, 3)

    def block(p, x, L):
        kind, c, low, kt = L
        h = (c - low) // 2
        m, a = p + ".inceptionmixer", p + ".inceptionmixer.attn"
        g = a + ".spatial_gating_unit"
        s1, t1 = bn_affine(sd, p + ".norm1")
        u = r(gelu(conv(x, *fold_in(sd[a + ".proj_1.weight"], sd[a + ".proj_1.bias"], s1, t1, c - low, c), False)))
        at = dwsep(g + ".conv0", u)
        sm = r((at + dwsep(g + ".conv0_1", at)) + dwsep(g + ".conv1_1", at))
        gt = r(conv(sm, sd[g + ".conv3.weight"], sd[g + ".conv3.bias"], False) * u)
        yl = conv(gt, sd[a + ".proj_2.weight"], sd[a + ".proj_2.bias"], False)
        pl = r(bn_pool_cl(x[:, :h].permute(0, 2, 3, 4, 1), s1[:h], t1[:h], kt)).permute(0, 4, 1, 2, 3)
        yh1 = basic(m + ".maxpool_fc.1", pl)
        w, b = fold_out(sd, m + ".fc_dw.0.conv.weight", m + ".fc_dw.0.bn")
        f = conv(x, *fold_in(w, b, s1, t1, h, c), True)
        yh2 = dwsep(m + ".fc_dw.1", f, "affine2", m + ".fc_dw.2")
        mx = torch.cat([yl, yh1, yh2], 1)
        if extra is not None:
            extra.append(mx)
        if kind == "iformer_light":
            return r(gelu(x + mx))
        x = r(x + mx)
        s2, t2 = bn_affine(sd, p + ".norm2")
        y = conv(x, *fold_in(sd[p + ".mlp.fc1.weight"], sd[p + ".mlp.fc1.bias"], s2, t2, 0, c), False)
        y = dwsep(p + ".mlp.dwconv.dwconv", y, "gelu")
        ml = conv(y, sd[p + ".mlp.fc2.weight"], sd[p + ".mlp.fc2.bias"], False)
        if extra is not None:
            extra.append(ml)
        return r(x + ml)

    y = r(x.float())
    if srm:
        y = r(F.conv3d(y, r(sd["SRM.hpf.weight"]), padding=(0, 2, 2)))
    for i, L in enumerate(msca_s3d_base(srm)):
        p = f"base.{i}"
        if L[0] == "sep":
            y = sep(p, y, L[4], L[5])
        elif L[0] == "basic":
            y = basic(p, y)
        elif L[0] == "pool":
            y = F.max_pool3d(y, *L[1:])
        elif L[0] in ("iformer", "iformer_light"):
            y = block(p, y, L)
        else:
            v2 = L[0] == "mixed_v2"
            y0 = basic(f"{p}.branch0.0", y)
            y1 = sep(f"{p}.branch1.1", basic(f"{p}.branch1.0", y), 1, 1, v2)
            y2 = sep(f"{p}.branch2.1", basic(f"{p}.branch2.0", y), 1, 1, v2)
            y3 = basic(f"{p}.branch3.1", F.max_pool3d(y, 3, 1, 1))
            y = torch.cat((y0, y1, y2, y3), 1)
        if taps is not None:
            taps.append(y)
    return y


@torch.no_grad()
def forward_emulated(sd, x, srm: bool, dtype: str = "fp16", taps=None, extra=None):
    sd32 = cast_sd(sd, torch.float32)
    r = lambda t: round_to(t, dtype)  # noqa: E731
    y = features_emulated(sd, x, srm, dtype, taps, extra)
    y = r(F.avg_pool3d(y, (2, y.size(3), y.size(4)), stride=1))
    y = r(y.mean(2, keepdim=True))
    y = F.conv3d(y, r(sd32["fc.0.weight"]), sd32["fc.0.bias"])
    return y.view(y.size(0), y.size(1))


def load_blocks(golden):
    return {**golden("msca_s3d_golden_blocks.npz"), **golden("msca_s3d_golden_blocks_srm.npz")}
