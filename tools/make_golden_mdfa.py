"""Generate the fixtures of the three MDFA CViT classes (fac_fake_amd/mdfa.py)
under tests/golden/ from the REFERENCE's own class code.

Needs the reference checkout (``--reference DIR`` or $FAC_REFERENCE_DIR: the
directory that holds ``CViT-main/``), so it runs only where that exists.  Like
tools/make_golden_bfm.py it parses ``CViT-main/model/other/<name>.py`` with
``ast`` and executes its imports, assignments, functions and class definitions
unchanged, on the CPU, with a stub for the absent ``torchsummary``.

The fixtures are data only (no reference source), on make_mdfa_state_dict(name,
0) and 4 make_crops crops (seed 41, slots 0..3):

  mdfa_keys.json      per class the reference state_dict's keys and shapes, in order
  mdfa_golden.npz     "<name>/logits": the fp32 logits; the maps before and
                      after MDFA ("<name>/mdfa_in_sum", "_sample", "<name>/mdfa_..."):
                      the float64 sum and every 997th value; "module/<shape>":
                      the reference's own MDFA module (eval) on a small map, with
                      the generator's weights (module_case)
  mdfa_envelope.json  per class: per dtype the largest probability difference
                      between those logits and tests/mdfa_ref.py's 16-bit
                      emulation; "fp32": forward_fp32's largest logit distance
                      from the reference class; "mdfa_block": per dtype the
                      relative L2 and max |d| of mdfa_block's emulation against
                      its float64 form on the golden map; "t_share", "ratio",
                      "max_cat": the shares asserted below

It asserts, on the 4 golden crops of every class (weights.MDFA_GAIN,
MDFA_S_GAIN and MDFA_T_MEAN are what to adjust):
  * each side of max(t_b, s_p) wins on at least 20 % of the pixels;
  * ||MDFA(f)|| / ||f|| within 0.25 .. 4, max cat <= 64;
  * no golden probability within 0.05 of 0 or 1;
and, on the reference's own MDFA module at three shapes with randomised
BatchNorm statistics, that mdfa_block (dropped taps, one scalar gate per pixel,
branch 5 as a per-crop vector) is the module: within 1e-5 relative in fp32 and
1e-12 in float64.
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

import mdfa_ref as R  # noqa: E402
from fac_fake_amd.weights import _mdfa_specs, make_crops, make_mdfa_state_dict, synthetic_state_dict, uniform  # noqa: E402
from tools.make_golden import ref_normalize  # noqa: E402
from tools.make_golden_bfm import load_reference_class  # noqa: E402
from tools.make_golden_other import _summ  # noqa: E402

CROP_SEED = 41
MARGIN = 0.05
MODULE_SHAPES = [(2, 64, 7, 7), (1, 128, 9, 13)]       # recorded; (1, 256, 14, 14) is checked here only
N_KEYS = {"cvit_GGCA4_MDFA5": 246, "cvit_MDFA_BFM": 260, "cvit_BFM_MDFA": 260}


def module_case(shape):
    """(state_dict of an MDFA(c, c) under prefix "mdfa", x NCHW fp32) of one recorded module case."""
    n, c, h, w = shape
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_state_dict(_mdfa_specs("mdfa", c), 0).items()}
    x = torch.from_numpy(uniform(f"mdfa_module_x/{c}x{h}x{w}", n * c * h * w, 0).reshape(n, c, h, w).copy()) * 1.5
    return sd, x


def module_key(shape):
    return "module/" + "x".join(map(str, shape))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("FAC_REFERENCE_DIR"), required="FAC_REFERENCE_DIR" not in os.environ,
                    help="the directory that holds the reference's CViT-main/")
    ap.add_argument("--dry-run", action="store_true", help="print the figures, write nothing")
    args = ap.parse_args(argv)
    torch.manual_seed(0)
    torch.set_num_threads(16)
    x = ref_normalize(make_crops(4, seed=CROP_SEED))
    keys, gold, env = {}, {"crop_seed": np.int64(CROP_SEED)}, {}

    MDFA = load_reference_class(Path(args.reference), "cvit_GGCA4_MDFA5").__init__.__globals__["MDFA"]
    for shape in MODULE_SHAPES + [(1, 256, 14, 14)]:
        sd, xm = module_case(shape)
        c = shape[1]
        for dtype, bound in ((torch.float32, 1e-5), (torch.float64, 1e-12)):
            ops = R.mdfa_fold(sd, dtype=dtype)
            mod = MDFA(c, c).to(dtype).eval()
            mod.load_state_dict({k[len("mdfa."):]: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()})
            with torch.no_grad():
                want = mod(xm.to(dtype))
                got = R.mdfa_block(xm, ops, dtype)
                lit = R.mdfa_module(xm, ops, dtype)
            d, dl = float((got - want).abs().max()), float((lit - want).abs().max())
            print(f"MDFA module {shape} {dtype}: max|mdfa_block - module| {d:.3e}, max|mdfa_module - module| {dl:.3e} at "
                  f"values up to {float(want.abs().max()):.3f}; t share {R.t_share(xm, ops):.3f}", flush=True)
            assert d <= bound * max(1.0, float(want.abs().max())), (shape, dtype, d)
            if dtype == torch.float32 and shape in MODULE_SHAPES:
                gold[module_key(shape)] = want.numpy()

    for name in R.NAMES:
        m = load_reference_class(Path(args.reference), name)(image_size=224, patch_size=7, num_classes=2, channels=512,
                                                             dim=1024, depth=6, heads=8, mlp_dim=2048).eval()
        keys[name] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        assert len(keys[name]) == N_KEYS[name], (name, len(keys[name]))
        sd = make_mdfa_state_dict(name, 0)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
        got = {}
        m.mdfa.register_forward_hook(lambda _m, i, o: got.update(mdfa_in=i[0].detach().clone(), mdfa=o.detach().clone()))
        with torch.no_grad():
            logits = m(x)
        gold[f"{name}/logits"] = logits.numpy()
        p_ref = torch.sigmoid(logits)
        print(name, "logits", logits.numpy().tolist(), "probs", p_ref.numpy().tolist(), flush=True)
        for k in ("mdfa_in", "mdfa"):
            _summ(gold, f"{name}/{k}", got[k])
        f, blk = got["mdfa_in"], got["mdfa"]
        ops = R.mdfa_fold(sd)
        _, parts = R.mdfa_block(f, ops, parts=True)
        share = float((parts["t"].view(-1, 1, 1) > parts["s"]).double().mean())
        ratio = float(blk.norm() / f.norm())
        max_cat = float(max(parts["cat4"].max(), parts["g"].max()))
        d_blk = float((R.mdfa_block(f, ops, torch.float32) - blk).abs().max())
        print(f"MDFA: t wins on {share:.3f} of the pixels (t_b {parts['t'].tolist()}, s_p {float(parts['s'].min()):.3f} .. "
              f"{float(parts['s'].max()):.3f}); ||MDFA(f)||/||f|| {ratio:.3f}; max cat {max_cat:.2f}; mdfa_block fp32 vs the "
              f"reference module: max|d| {d_blk:.3e} at output scale {float(blk.abs().mean()):.3e}", flush=True)
        assert 0.2 <= share <= 0.8, share
        assert 0.25 <= ratio <= 4, ratio
        assert max_cat <= 64, max_cat
        assert float(p_ref.min()) >= MARGIN and float(p_ref.max()) <= 1 - MARGIN, f"{name}: a golden probability is saturated"
        env[name] = {"t_share": share, "ratio": ratio, "max_cat": max_cat}
        env[name]["fp32"] = float((R.forward_fp32(name, sd, x) - logits).abs().max())
        for dt in ("fp16", "bf16"):
            env[name][dt] = float((torch.sigmoid(R.forward_emulated(name, sd, x, dtype=dt)) - p_ref).abs().max())
        env[name]["mdfa_block"] = {}
        for dt in ("fp16", "bf16"):
            f16, ops16 = R.round_to(f, dt), R.round_ops(ops, dt)
            ref16 = R.mdfa_block(f16, ops16)
            e = R.mdfa_block(f16, ops16, torch.float32, round=dt).double() - ref16
            env[name]["mdfa_block"][dt] = {"rel_l2": float(e.norm() / ref16.norm()), "max_abs": float(e.abs().max())}
        print(name, "envelope", env[name], flush=True)
    if args.dry_run:
        return
    (OUT / "mdfa_keys.json").write_text(json.dumps(keys))
    np.savez_compressed(OUT / "mdfa_golden.npz", **gold)
    (OUT / "mdfa_envelope.json").write_text(json.dumps(env, indent=1))


if __name__ == "__main__":
    main()
