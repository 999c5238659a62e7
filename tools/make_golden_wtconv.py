"""Generate the fixtures of cvit_GGCA_ADD_WTConv (fac_fake_amd/wtconv.py) under
tests/golden/ from the REFERENCE's own class code.

Needs the reference checkout (``--reference DIR`` or $FAC_REFERENCE_DIR: the
directory that holds ``CViT-main/``), so it runs only where that exists.  Like
tools/make_golden_odconv.py it loads ``CViT-main/model/other/<name>.py`` with
tools.make_golden_bfm.load_reference_class and runs it unchanged, on the CPU.
The reference imports ``pywt`` for the four two-tap db1 filters; where
PyWavelets is absent this tool installs a stand-in module (``pywt_stand_in``,
the project's own text) whose ``Wavelet("db1")`` has PyWavelets' values: dec_lo
= rec_lo = [r, r], dec_hi = [-r, r], rec_hi = [r, -r], r = 2^-1/2.

The fixtures are data only (no reference source), on make_wtconv_state_dict(
seed 0) and 8 make_crops crops (seed 41, slots 0..7):

  wtconv_keys.json          the reference state_dict's keys and shapes, in order
  wtconv_block_golden.npz   "<kind>/<shape>": the reference's own WTConv2d(c)
                            module in fp32 on a small signed ("signed") and a
                            post-ReLU ("relu") input per width, with the
                            generator's weights (block_case)
  wtconv_golden.npz         "logits", "probs": the class's fp32 outputs on the 8
                            crops; per WT site its input and output map
                            ("features.3_in_sum", "_sample", ...): the float64
                            sum and every 997th value
  wtconv_envelope.json      per dtype the largest probability difference between
                            the golden and tests/wtconv_ref.py's 16-bit emulation
                            over the 8 crops; "fp32": forward_fp32's largest
                            logit distance from the reference class, floored at
                            FP32_FLOOR; "blocks":
                            per site the two ratios asserted below

It asserts (weights.WTCONV_BASE_GAIN, WTCONV_WAVE_GAIN and the two WTCONV_OUT_*
tables are what to adjust; ``--calibrate`` prints the tables, measured block by
block with wtconv_ref.wt_reference):
  * the class reports the key count 202 - 18 + 9 * 7 = 247 and its wt_filter /
    iwt_filter are weights.db1_filters' bit for bit;
  * wtconv_ref.wt_layer in float64 is the reference module (in float64) to 1e-12
    of the largest output on the block cases;
  * on the fixture crops, at every site, ||wavelet path|| / ||base path|| of the
    restatement lies in 0.25 .. 4, and ||out|| / ||in|| of the reference module's
    output after BatchNorm and ReLU lies in 0.25 .. 4;
  * no golden probability within 0.05 of 0 or 1.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import types
from pathlib import Path

sys.dont_write_bytecode = True
REPO = Path(__file__).resolve().parents[1]
OUT = REPO / "tests" / "golden"
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import wtconv_ref as R  # noqa: E402
from fac_fake_amd import weights as W  # noqa: E402
from fac_fake_amd.weights import (_wtconv_bn_specs, _wtconv_specs, db1_filters, make_crops, make_wtconv_state_dict,  # noqa: E402
                                  synthetic_state_dict, uniform)
from oracle.cvit_torch import BN_EPS  # noqa: E402
from tools.make_golden import ref_normalize  # noqa: E402
from tools.make_golden_bfm import load_reference_class  # noqa: E402
from tools.make_golden_other import _summ  # noqa: E402

NAME = R.NAME
CROP_SEED = 41
N_CROPS = 8
MARGIN = 0.05
N_KEYS = 202 - 18 + 9 * 7
# forward_fp32 calls the ops the reference class calls, so on the generating host it measures 0; another host's CPU
# kernels may sum in another order.  The recorded figure is floored at the family's floor for this comparison
# (test_odconv.py: 2e-5) over the test's margin of 1.25.
FP32_FLOOR = 2e-5 / 1.25
BLOCK_SHAPES = [(2, 32, 10, 14), (3, 64, 6, 6), (1, 256, 4, 18)]
BLOCK_KINDS = ("signed", "relu")


def pywt_stand_in():
    """A module that stands in for PyWavelets where it is absent: Wavelet("db1") with its four two-tap filters."""
    r = 2.0 ** -0.5

    class Wavelet:
        def __init__(self, name):
            if name != "db1":
                raise ValueError(f"the stand-in has db1 only, not {name!r}")
            self.dec_lo, self.dec_hi, self.rec_lo, self.rec_hi = [r, r], [-r, r], [r, r], [r, -r]

    mod, data = types.ModuleType("pywt"), types.ModuleType("pywt.data")
    mod.Wavelet, mod.data = Wavelet, data
    return mod, data


def install_pywt():
    if "pywt" in sys.modules:
        return
    try:
        import pywt  # noqa: F401
        import pywt.data  # noqa: F401
    except ImportError:
        sys.modules["pywt"], sys.modules["pywt.data"] = pywt_stand_in()


def block_case(shape, kind):
    """(state_dict of a WTConv2d(c) under prefix "wt", x NCHW fp32) of one recorded block case."""
    n, c, h, w = shape
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_state_dict(_wtconv_specs("wt", c), 0).items()}
    tag = f"{kind}/{c}x{h}x{w}"
    x = torch.from_numpy(uniform("wtconv_block_x/" + tag, n * c * h * w, 0).reshape(n, c, h, w).copy()) * 2.5
    return sd, (torch.relu(x + 0.5) if kind == "relu" else x)


def block_key(shape, kind):
    return kind + "/" + "x".join(map(str, shape))


def _load_block(WTConv2d, sd, c, dtype):
    mod = WTConv2d(in_channels=c).to(dtype).eval()
    mod.load_state_dict({k[len("wt."):]: v.to(dtype) for k, v in sd.items()})
    return mod


def _site_module(m, p):
    return m.features[int(p.split(".")[1])]


def _run(cls, sd, x):
    m = cls(image_size=224, patch_size=7, num_classes=2, channels=512, dim=1024, depth=6, heads=8, mlp_dim=2048).eval()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    got = {}
    for p, *_ in R.SITES:
        _site_module(m, p).register_forward_hook(
            lambda _m, i, o, p=p: got.update({p + "_in": i[0].detach().clone(), p + "_raw": o.detach().clone()}))
    with torch.no_grad():
        logits = m(x)
    return m, logits, got


def _r4(v):
    return float(f"{float(v):.4g}")


@torch.no_grad()
def calibrate(x):
    """One walk down the stem with wtconv_ref's ops: at every WT site the raw block output's deviation and mean
    go into the tables before the site's BatchNorm is drawn."""
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in make_wtconv_state_dict(NAME, 0).items()}
    h = x
    for layer in R.LAYERS:
        p, q = f"{layer[0]}.{layer[1]}", f"{layer[0]}.{layer[5]}"
        if layer[2] == "wt":
            u, v = R.wt_reference(h, sd, p, parts=True)
            raw = u + v
            W.WTCONV_OUT_STD[q], W.WTCONV_OUT_MEAN[q] = _r4(raw.double().std()), _r4(raw.double().mean())
            print(q, "std", W.WTCONV_OUT_STD[q], "mean", W.WTCONV_OUT_MEAN[q], "wavelet/base", float(u.norm() / v.norm()), flush=True)
            sd.update({k: torch.from_numpy(np.asarray(t)) for k, t in synthetic_state_dict(_wtconv_bn_specs(q, layer[4]), 0).items()})
            h = raw
        else:
            h = F.conv2d(h, sd[p + ".weight"], sd[p + ".bias"], padding=1)
        h = F.relu(F.batch_norm(h, sd[q + ".running_mean"], sd[q + ".running_var"], sd[q + ".weight"], sd[q + ".bias"],
                                False, 0.1, BN_EPS))
        if layer[7]:
            h = F.max_pool2d(h, 2, 2)
        print(p, layer[2], "out mean|x|", float(h.abs().mean()), "dead channels", int((h.amax((0, 2, 3)) == 0).sum()), flush=True)
    for k in ("WTCONV_OUT_STD", "WTCONV_OUT_MEAN"):
        print(k, "=", getattr(W, k))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("FAC_REFERENCE_DIR"), required="FAC_REFERENCE_DIR" not in os.environ,
                    help="the directory that holds the reference's CViT-main/")
    ap.add_argument("--dry-run", action="store_true", help="print the figures, write nothing")
    ap.add_argument("--calibrate", action="store_true", help="measure the WTCONV_OUT_* tables block by block, print them, write nothing")
    args = ap.parse_args(argv)
    torch.manual_seed(0)
    torch.set_num_threads(16)
    x = ref_normalize(make_crops(N_CROPS, seed=CROP_SEED))
    if args.calibrate:
        calibrate(x)
        return
    install_pywt()
    cls = load_reference_class(Path(args.reference), NAME)
    WTConv2d = cls.__init__.__globals__["WTConv2d"]

    gold_b = {}
    for shape in BLOCK_SHAPES:
        for kind in BLOCK_KINDS:
            sd, xb = block_case(shape, kind)
            c = shape[1]
            with torch.no_grad():
                m32, m64 = _load_block(WTConv2d, sd, c, torch.float32), _load_block(WTConv2d, sd, c, torch.float64)
                want32, want64 = m32(xb), m64(xb.double())
                got64 = R.wt_layer(xb, R.wt_fold(sd, "wt", None, torch.float64), False, torch.float64, relu=False)
                ref64 = R.wt_reference(xb, sd, "wt", torch.float64)
            d64, dr = float((got64 - want64).abs().max()), float((ref64 - want64).abs().max())
            print(f"WTConv {shape} {kind}: float64 wt_layer vs module {d64:.3e}, wt_reference vs module {dr:.3e}; fp32 module vs "
                  f"float64 module {float((want32.double() - want64).abs().max()):.3e} at values up to {float(want64.abs().max()):.3e}",
                  flush=True)
            assert d64 <= 1e-12 * float(want64.abs().max()) and dr <= 1e-12 * float(want64.abs().max()), (shape, kind, d64, dr)
            gold_b[block_key(shape, kind)] = want32.numpy()

    sd = make_wtconv_state_dict(NAME, 0)
    m, logits, got = _run(cls, sd, x)
    keys = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert len(keys) == N_KEYS, len(keys)
    fresh = cls().state_dict()                    # the class's own filters, as built through the (stand-in) pywt
    for p, _bn, c, _h, _pool in R.SITES:
        for leaf, want in zip(("wt_filter", "iwt_filter"), db1_filters(c)):
            assert np.array_equal(fresh[f"{p}.{leaf}"].numpy(), want), (p, leaf)
    gold, env = {"crop_seed": np.int64(CROP_SEED)}, {}
    p_ref = torch.sigmoid(logits)
    print(NAME, "logits", logits.numpy().tolist(), "probs", p_ref.numpy().tolist(), flush=True)
    gold["logits"], gold["probs"] = logits.numpy(), p_ref.numpy()
    out32, maps = R.forward_fp32(sd, x, return_features=True)
    d32 = float((out32 - logits).abs().max())
    print(f"forward_fp32 vs the reference class: max |dlogit| {d32:.3e} (recorded with the floor {FP32_FLOOR:.1e})", flush=True)
    env = {"fp32": max(d32, FP32_FLOOR), "blocks": {}}
    sdt = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    for p, bn, c, _h, pool in R.SITES:
        f = got[p + "_in"]
        _summ(gold, f"{p}_in", f)
        _summ(gold, p, maps[p])
        ops = R.wt_fold(sdt, p, bn)
        with torch.no_grad():
            u, b = R.wt_layer(f, ops, dtype=torch.float32, parts=True)
            post = torch.relu(got[p + "_raw"] * ops["scale"].view(1, -1, 1, 1) +
                              (ops["shift"] - ops["scale"] * sdt[p + ".base_scale.weight"].reshape(-1) *
                               sdt[p + ".base_conv.bias"]).view(1, -1, 1, 1))
            d_mod = float((R.wt_reference(f, sdt, p) - got[p + "_raw"]).abs().max())
        rec = {"wavelet_over_base": float(u.norm() / b.norm()), "ratio": float(post.norm() / f.norm()),
               "dead_channels": int((post.amax((0, 2, 3)) == 0).sum())}
        print(f"{p}: {rec}; raw output std {float(got[p + '_raw'].std()):.4g} mean {float(got[p + '_raw'].mean()):.4g}; "
              f"wt_reference vs the module {d_mod:.3e}", flush=True)
        assert 0.25 <= rec["wavelet_over_base"] <= 4 and 0.25 <= rec["ratio"] <= 4, (p, rec)
        env["blocks"][p] = rec
    assert float(p_ref.min()) >= MARGIN and float(p_ref.max()) <= 1 - MARGIN, "a golden probability is saturated"
    for dt in ("fp16", "bf16"):
        env[dt] = float((torch.sigmoid(R.forward_emulated(sd, x, dtype=dt)) - p_ref).abs().max())
    print(NAME, "envelope", env, flush=True)
    if args.dry_run:
        return
    (OUT / "wtconv_keys.json").write_text(json.dumps(keys))
    np.savez_compressed(OUT / "wtconv_block_golden.npz", **gold_b)
    np.savez_compressed(OUT / "wtconv_golden.npz", **gold)
    (OUT / "wtconv_envelope.json").write_text(json.dumps(env, indent=1))


if __name__ == "__main__":
    main()
