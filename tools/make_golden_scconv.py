"""Generate the fixtures of cvit_GGCA_ADD_ScConv (fac_fake_amd/scconv.py) under
tests/golden/ from the REFERENCE's own class code.

Needs the reference checkout (``--reference DIR`` or $FAC_REFERENCE_DIR: the
directory that holds ``CViT-main/``), so it runs only where that exists.  Like
tools/make_golden_bfm.py it parses ``CViT-main/model/other/<name>.py`` with
``ast`` and executes its imports, assignments, functions and class definitions
unchanged, on the CPU, with a stub for the absent ``torchsummary``.

The fixtures are data only (no reference source), on make_scconv_state_dict(name,
0) and 8 make_crops crops (seed 41, slots 0..7):

  scconv_keys.json          the reference state_dict's keys and shapes, in order
  scconv_block_golden.npz   "<kind>/<shape>": the reference's own ScConv(c)
                            module in fp32 on a small signed ("signed") and a
                            post-ReLU ("relu") input per width, with the
                            generator's weights (block_case)
  scconv_golden.npz         "logits", "probs": the class's fp32 outputs on the 8
                            crops; per block its input and output map
                            ("features1.13_in_sum", "_sample", ...): the float64
                            sum and every 997th value
  scconv_envelope.json      per dtype the largest probability difference
                            between the golden and tests/scconv_ref.py's 16-bit
                            emulation over the 8 crops; "fp32": forward_fp32's
                            largest logit distance from the reference class;
                            "blocks": per block the shares asserted below

It asserts, on the fixture crops (weights.SCCONV_OUT_STD / SCCONV_OUT_MEAN and
the gamma / beta ranges are what to adjust; ``--calibrate`` prints the former
two, measured block by block on the reference class):
  * both sides of the gate are taken on 20 .. 80 % of the elements of every block;
  * no softmax entry s exceeds 10 / 2C;
  * every block's ||out|| / ||in|| after its BatchNorm and ReLU lies in 0.25 .. 4;
  * |sum(gamma)| >= C / 4 for every block;
  * no golden probability within 0.05 of 0 or 1;
and that scconv_ref.scconv_block in float64 is the reference module (in
float64) to 1e-12 on the block cases.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

sys.dont_write_bytecode = True
REPO = Path(__file__).resolve().parents[1]
OUT = REPO / "tests" / "golden"
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import scconv_ref as R  # noqa: E402
from fac_fake_amd import weights as W  # noqa: E402
from fac_fake_amd.weights import _scconv_specs, make_crops, make_scconv_state_dict, synthetic_state_dict, uniform  # noqa: E402
from tools.make_golden import ref_normalize  # noqa: E402
from tools.make_golden_bfm import load_reference_class  # noqa: E402
from tools.make_golden_other import _summ  # noqa: E402

NAME = "cvit_GGCA_ADD_ScConv"
CROP_SEED = 41
N_CROPS = 8
MARGIN = 0.05
N_KEYS = 226
BLOCK_SHAPES = [(2, 64, 10, 14), (2, 128, 6, 6), (1, 256, 4, 18)]
BLOCK_KINDS = ("signed", "relu")
SITES = (("features1.13", "features1.14", 64), ("features1.23", "features1.24", 128), ("features1.33", "features1.34", 256),
         ("features1.39", "features1.40", 256))


def block_case(shape, kind):
    """(state_dict of a ScConv(c) under prefix "sc", x NCHW fp32) of one recorded block case."""
    n, c, h, w = shape
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_state_dict(_scconv_specs("sc", c), 0).items()}
    x = torch.from_numpy(uniform(f"scconv_block_x/{kind}/{c}x{h}x{w}", n * c * h * w, 0).reshape(n, c, h, w).copy()) * 2.5
    return sd, (torch.relu(x + 0.5) if kind == "relu" else x)


def block_key(shape, kind):
    return kind + "/" + "x".join(map(str, shape))


def _load_block(ScConv, sd, c, dtype):
    mod = ScConv(c).to(dtype).eval()
    mod.load_state_dict({k[len("sc."):]: v.to(dtype) for k, v in sd.items()})
    return mod


def _run(cls, sd, x):
    m = cls(image_size=224, patch_size=7, num_classes=2, channels=512, dim=1024, depth=6, heads=8, mlp_dim=2048).eval()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    got = {}
    for p, _bn, _c in SITES:
        mod = m.features1[int(p.split(".")[1])]
        mod.register_forward_hook(lambda _m, i, o, p=p: got.update({p + "_in": i[0].detach().clone(), p + "_raw": o.detach().clone()}))
    with torch.no_grad():
        logits = m(x)
    return m, logits, got


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("FAC_REFERENCE_DIR"), required="FAC_REFERENCE_DIR" not in os.environ,
                    help="the directory that holds the reference's CViT-main/")
    ap.add_argument("--dry-run", action="store_true", help="print the figures, write nothing")
    ap.add_argument("--calibrate", action="store_true",
                    help="measure SCCONV_OUT_STD / SCCONV_OUT_MEAN block by block, print them, write nothing")
    args = ap.parse_args(argv)
    torch.manual_seed(0)
    torch.set_num_threads(16)
    x = ref_normalize(make_crops(N_CROPS, seed=CROP_SEED))
    cls = load_reference_class(Path(args.reference), NAME)
    ScConv = cls.__init__.__globals__["ScConv"]

    if args.calibrate:
        for p, bn, _c in SITES:            # each block's statistics with the earlier ones already fixed
            _m, _lg, got = _run(cls, make_scconv_state_dict(NAME, 0), x)
            raw = got[p + "_raw"].double()
            W.SCCONV_OUT_STD[bn], W.SCCONV_OUT_MEAN[bn] = float(f"{float(raw.std()):.4g}"), float(f"{float(raw.mean()):.4g}")
            print(bn, "std", W.SCCONV_OUT_STD[bn], "mean", W.SCCONV_OUT_MEAN[bn], flush=True)
        print("SCCONV_OUT_STD =", W.SCCONV_OUT_STD)
        print("SCCONV_OUT_MEAN =", W.SCCONV_OUT_MEAN)
        return

    gold_b = {}
    for shape in BLOCK_SHAPES:
        for kind in BLOCK_KINDS:
            sd, xb = block_case(shape, kind)
            c = shape[1]
            with torch.no_grad():
                want32 = _load_block(ScConv, sd, c, torch.float32)(xb)
                want64 = _load_block(ScConv, sd, c, torch.float64)(xb.double())
                ops = R.scconv_fold(sd, "sc", None, torch.float64)
                got64, parts = R.scconv_block(xb, ops, torch.float64, parts=True, raw=True)
            d64 = float((got64 - want64).abs().max())
            tau, t64 = R.tau_of(xb, R.scconv_fold(sd, "sc", None), how="module")
            share = float((parts["t"] * ops["kc"].view(1, -1, 1, 1) > 0).double().mean())
            print(f"ScConv {shape} {kind}: float64 restatement vs module {d64:.3e}; fp32 module vs float64 module "
                  f"{float((want32.double() - want64).abs().max()):.3e} at values up to {float(want64.abs().max()):.3e}; tau "
                  f"{tau:.3e}, gate open on {share:.3f}", flush=True)
            assert d64 <= 1e-12 * max(1.0, float(want64.abs().max())), (shape, kind, d64)
            gold_b[block_key(shape, kind)] = want32.numpy()

    sd = make_scconv_state_dict(NAME, 0)
    m, logits, got = _run(cls, sd, x)
    keys = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert len(keys) == N_KEYS, len(keys)
    p_ref = torch.sigmoid(logits)
    print("logits", logits.numpy().tolist(), "probs", p_ref.numpy().tolist(), flush=True)
    gold = {"crop_seed": np.int64(CROP_SEED), "logits": logits.numpy(), "probs": p_ref.numpy()}
    out32, maps = R.forward_fp32(sd, x, return_features=True)
    env = {"fp32": float((out32 - logits).abs().max()), "blocks": {}}
    sdt = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    for p, bn, c in SITES:
        f = got[p + "_in"]
        after = maps[p]                                      # after the BatchNorm, ReLU (and pool)
        _summ(gold, p + "_in", f)
        _summ(gold, p, after)
        ops = R.scconv_fold(sdt, p, bn)
        _, parts = R.scconv_block(f, ops, torch.float64, parts=True)
        share = float((parts["t"] * ops["kc"].double().view(1, -1, 1, 1) > 0).double().mean())
        smax = float(parts["s"].max()) * 2 * c
        unpooled = R.scconv_block(f, ops, torch.float32)
        ratio = float(unpooled.norm() / f.norm())
        gsum = float(ops["gamma"].sum())
        d_mod = float((R.scconv_block(f, ops, torch.float32, raw=True) - got[p + "_raw"]).abs().max())
        print(f"{p}: gate open on {share:.3f}; max s x 2C {smax:.2f}; ||out||/||in|| {ratio:.3f}; sum(gamma) {gsum:.2f}; raw "
              f"output std {float(got[p + '_raw'].std()):.4g} mean {float(got[p + '_raw'].mean()):.4g}; fp32 restatement vs "
              f"module {d_mod:.3e}", flush=True)
        assert 0.2 <= share <= 0.8, (p, share)
        assert smax <= 10, (p, smax)
        assert 0.25 <= ratio <= 4, (p, ratio)
        assert abs(gsum) >= c / 4, (p, gsum)
        env["blocks"][p] = {"gate_share": share, "s_max_x2c": smax, "ratio": ratio}
    assert float(p_ref.min()) >= MARGIN and float(p_ref.max()) <= 1 - MARGIN, "a golden probability is saturated"
    for dt in ("fp16", "bf16"):
        env[dt] = float((torch.sigmoid(R.forward_emulated(sd, x, dtype=dt)) - p_ref).abs().max())
    print("envelope", env, flush=True)
    if args.dry_run:
        return
    (OUT / "scconv_keys.json").write_text(json.dumps(keys))
    np.savez_compressed(OUT / "scconv_block_golden.npz", **gold_b)
    np.savez_compressed(OUT / "scconv_golden.npz", **gold)
    (OUT / "scconv_envelope.json").write_text(json.dumps(env, indent=1))


if __name__ == "__main__":
    main()
