"""Drop-in ``msca_S3D`` (the clip harness's ``--model_type 1``) on gfx950 HIP kernels.

Mirrors ``sx_exp_deepfakedetect-master/S3D/msca_S3D.py::msca_S3D`` (:17-72):
S3D's stem and its last two Inception blocks, all with ReLU6
(``new_model/Conv3d.py``; ``Mixed_5b`` with ``SepConv3dV2`` branches), around
11 iFormer blocks (``new_model/iformer_3d.py``, ``msca_3d.py``).  Same
constructor ``msca_S3D(num_class, SRM_net)``, the same 853-key ``state_dict``,
the same ``forward`` on a raw clip.  Inference only; no CPU fallback.

One iFormer block of width C = low + 2 h on x [N, T, H, W, C] (16-bit,
channels-last), ``n = norm1(x)`` never materialised:

* attention (the last ``low`` channels of n): ``proj_1`` with norm1 folded in,
  read over the full width through zero weight columns (fac_conv_nd), GELU
  (fac_ew), ``conv0`` (fac_dwsep3d), the MSCA sum ``a + DWSep5(a) + DWSep7(a)``
  (ops.msca_sum), ``conv3`` (fac_conv_nd), the gate ``* u`` (fac_ew),
  ``proj_2`` straight into channels [0, low) of the mixer output;
* pool branch (the first h channels): norm1 + MaxPool3d((kt,3,3)) in one
  sliced launch (fac_bn_maxpool3d), the 1x1x1 conv + BN + ReLU6 into [low, low + h);
* conv branch (the next h channels): 1x1x1 conv with norm1 folded in and its
  own BN folded out + ReLU6, then DWSep(kt,3,3) + ReLU6 + ``fc_dw.2``'s
  BatchNorm in one fac_dwsep3d launch into [low + h, C);
* ``x + mixer`` (light block: ``GELU(x + mixer)``) in one fac_ew launch;
* Mlp (full block): ``fc1`` with norm2 folded in, DWSep(3,3,3) + ReLU6 + GELU
  in one fac_dwsep3d launch, ``fc2``, ``x + mlp``.

Every tensor written is rounded to 16 bits once; everything else is fp32.
"""
from __future__ import annotations

import torch

from . import ops
from .ca_s3d import CA_S3D_v3
from .ops import ConvLayer, DWSepLayer, bn_affine, fold_bn
from .s3d import BN_EPS, S3D, custom_round, custom_video_round, video_predictions
from .weights import msca_s3d_base, msca_s3d_param_specs


def _fold_in(w, b, s, t, lo: int, width: int):
    """A 1x1x1 conv (w [co, ci, 1, 1, 1], b) on channels [lo, lo + ci) of
    x * s + t, as a conv over all `width` channels of x: zero weight columns
    outside the slice, w' = w s, b' = b + w t (fp32, on the host)."""
    co, ci = w.shape[0], w.shape[1]
    wf = torch.zeros(co, width, 1, 1, 1)
    wf[:, lo:lo + ci] = w * s[lo:lo + ci].view(1, -1, 1, 1, 1)
    return wf, b + w.reshape(co, ci) @ t[lo:lo + ci]


class msca_S3D(S3D):
    relu6 = True

    def _base_desc(self):
        return msca_s3d_base(self._srm)

    def _param_specs(self):
        return msca_s3d_param_specs(self.num_class, self._srm)

    def train(self, mode: bool = True):
        if mode:
            raise RuntimeError("the gfx950 msca_S3D path is inference-only (BatchNorm is folded into the convs)")
        return super().train(False)

    # ------------------------------------------------------------------ weights
    def _prepare_block(self, p, L, sd, device):
        kind, c, low, kt = L
        h = (c - low) // 2
        dt = self.dtype_name
        f = lambda k: sd[k].detach().float().cpu()  # noqa: E731
        m, a = f"{p}.inceptionmixer", f"{p}.inceptionmixer.attn"
        g = f"{a}.spatial_gating_unit"

        def bn(q):
            return bn_affine(sd[q + ".weight"], sd[q + ".bias"], sd[q + ".running_mean"], sd[q + ".running_var"], BN_EPS)

        def conv(w, b):
            return ConvLayer(w, b, 1, 0, dtype=dt, device=device)

        def basic(q):   # BasicConv3d: conv + BN folded (its ReLU6: the conv's ReLU, then ops.clamp6_)
            return fold_bn(sd[q + ".conv.weight"], None, sd[q + ".bn.weight"], sd[q + ".bn.bias"],
                           sd[q + ".bn.running_mean"], sd[q + ".bn.running_var"], BN_EPS)

        def dwsep(q, act="none", bn2=None):
            s2, t2 = bn(bn2) if bn2 else (None, None)
            return DWSepLayer(sd[q + ".conv_s.weight"], sd[q + ".conv_t.weight"], *bn(q + ".bn_t"), act=act, scale2=s2,
                              shift2=t2, dtype=dt, device=device)

        s1, t1 = bn(f"{p}.norm1")
        B = dict(kt=kt, low=low, h=h, light=kind == "iformer_light")
        B["proj1"] = conv(*_fold_in(f(a + ".proj_1.weight"), f(a + ".proj_1.bias"), s1, t1, c - low, c))
        B["dw0"], B["dw5"], B["dw7"] = dwsep(g + ".conv0"), dwsep(g + ".conv0_1"), dwsep(g + ".conv1_1")
        B["conv3"] = conv(f(g + ".conv3.weight"), f(g + ".conv3.bias"))
        B["proj2"] = conv(f(a + ".proj_2.weight"), f(a + ".proj_2.bias"))
        B["s1h"], B["t1h"] = s1[:h].contiguous().to(device), t1[:h].contiguous().to(device)
        B["pool_fc"] = conv(*basic(m + ".maxpool_fc.1"))
        B["fcdw0"] = conv(*_fold_in(*basic(m + ".fc_dw.0"), s1, t1, h, c))
        B["fcdw1"] = dwsep(m + ".fc_dw.1", "affine2", m + ".fc_dw.2")
        if not B["light"]:
            s2, t2 = bn(f"{p}.norm2")
            B["fc1"] = conv(*_fold_in(f(p + ".mlp.fc1.weight"), f(p + ".mlp.fc1.bias"), s2, t2, 0, c))
            B["mdw"] = dwsep(p + ".mlp.dwconv.dwconv", "gelu")
            B["fc2"] = conv(f(p + ".mlp.fc2.weight"), f(p + ".mlp.fc2.bias"))
        return B

    # ------------------------------------------------------------------ forward
    _extra = None   # block_outputs: the mixer / mlp outputs are appended here

    def _run_block(self, kind, B, x):
        low, h, kt = B["low"], B["h"], B["kt"]
        mixer = torch.empty_like(x)
        u = B["proj1"](x, relu=False)
        ops.ew("gelu", u, out=u)
        a = B["dw0"](u)
        g = B["conv3"](ops.msca_sum(a, B["dw5"], B["dw7"]), relu=False)
        ops.ew("mul", g, u, out=g)
        B["proj2"](g, relu=False, out=mixer, c_off=0)
        B["pool_fc"](ops.bn_max_pool(x, B["s1h"], B["t1h"], kt, c=h), out=mixer, c_off=low)
        ops.clamp6_(mixer, low, h)
        B["fcdw1"](ops.clamp6_(B["fcdw0"](x)), out=mixer, c_off=low + h)
        if self._extra is not None:
            self._extra.append(mixer)
        if B["light"]:
            return ops.ew("add_gelu", x, mixer)
        x = ops.ew("add", x, mixer)
        mlp = B["fc2"](B["mdw"](B["fc1"](x, relu=False)), relu=False)
        if self._extra is not None:
            self._extra.append(mlp)
        return ops.ew("add", x, mlp)

    def block_outputs(self, x: torch.Tensor) -> list:
        """For the raw clip `x`: the ``inceptionmixer`` output of each of the
        11 iFormer blocks and, behind it, the ``mlp`` output of each of the 7
        full ones, in base order (18 tensors, channels-last 16-bit): what
        forward hooks on those modules of the reference see."""
        self._extra = []
        try:
            self.features16(self._pack(x))
            return self._extra
        finally:
            self._extra = None


def harness_model(model_type: int):
    """S3D-test.py's own switch (:210-217): the class behind ``--model_type``."""
    table = {0: S3D, 1: msca_S3D, 3: CA_S3D_v3}
    if model_type not in table:
        raise ValueError(f"model_type must be one of {sorted(table)} (S3D, msca_S3D, CA_S3D_v3), got {model_type!r}")
    return table[model_type]


__all__ = ["msca_S3D", "harness_model", "custom_round", "custom_video_round", "video_predictions"]
