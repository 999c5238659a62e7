"""Generate the fixtures of cvit_GGCA4_BFM5 (fac_fake_amd/bfm.py) under
tests/golden/ from the REFERENCE's own class code.

Needs the reference checkout (``--reference DIR`` or $FAC_REFERENCE_DIR: the
directory that holds ``CViT-main/``), so it runs only where that exists.  Like
tools/make_golden_other.py it parses ``CViT-main/model/other/<name>.py`` with
``ast`` and executes its imports, module-level assignments, functions and class
definitions unchanged, on the CPU.

The fixtures are data only (no reference source), on make_bfm_state_dict(name,
0) and 4 make_crops crops (seed 41, slots 0..3):

  bfm_keys.json      the reference state_dict's keys and shapes, in order
  bfm_golden.npz     "<name>/logits": the fp32 logits; the maps before and
                     after BFM ("<name>/pool5_sum", "_sample", "<name>/bfm_..."):
                     the float64 sum and every 997th value
  bfm_envelope.json  per dtype, the largest probability difference between
                     those logits and tests/bfm_ref.py's 16-bit emulation;
                     "fp32": forward_fp32's largest logit distance from the
                     reference class; "tfam_sensitivity": the largest logit
                     change of the REFERENCE class when its eight TFAM tensors
                     are redrawn with another seed; "model_route": the route
                     the emulated forward takes for the block; "bfm_block":
                     per route and dtype the relative L2 and max |d| of
                     bfm_block's emulation against its float64 form on the
                     golden pool5 map

It asserts, on the 4 golden crops (weights.BFM_GAIN and BFM_BIAS are what to
adjust):
  * ||BFM(f)|| / ||f|| within 0.25 .. 4;
  * at least 25 % of BFM's output elements have pre-activations of mixed sign
    across the three convs;
  * no golden probability within 0.05 of 0 or 1;
  * tfam_sensitivity <= forward_fp32's own distance from the reference class:
    BFM(x, x) = 4 MSFE(x) whatever the TFAM weights, on the real module.
"""
from __future__ import annotations

import argparse
import ast
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

import bfm_ref as R  # noqa: E402
from fac_fake_amd.weights import make_bfm_state_dict, make_crops, uniform  # noqa: E402
from tools.make_golden import ref_normalize  # noqa: E402
from tools.make_golden_other import _summ  # noqa: E402

CROP_SEED = 41
MARGIN = 0.05
TFAM_REDRAW_SEED = 7


def load_reference_class(ref_dir: Path, name: str):
    """make_golden_other's loader, which also keeps the module's functions (BFM's kernel_size)."""
    ref = ref_dir / "CViT-main" / "model" / "other" / f"{name}.py"
    tree = ast.parse(ref.read_text(), filename=str(ref))
    keep = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom, ast.ClassDef, ast.Assign, ast.FunctionDef))]
    if "torchsummary" not in sys.modules:
        try:
            import torchsummary  # noqa: F401
        except ImportError:
            stub = types.ModuleType("torchsummary")
            stub.summary = None
            sys.modules["torchsummary"] = stub
    ns = {"__name__": f"{name}_reference"}
    exec(compile(ast.Module(body=keep, type_ignores=[]), str(ref), "exec"), ns)
    return ns["CViT"]


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
    for name in R.NAMES:
        m = load_reference_class(Path(args.reference), name)(image_size=224, patch_size=7, num_classes=2, channels=512,
                                                             dim=1024, depth=6, heads=8, mlp_dim=2048).eval()
        keys[name] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        assert len(keys[name]) == R.N_KEYS[name], (name, len(keys[name]))
        sd = make_bfm_state_dict(name, 0)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
        got = {}
        m.features2.register_forward_hook(lambda _m, _i, o: got.update(pool5=o.detach().clone()))
        m.bfm.register_forward_hook(lambda _m, _i, o: got.update(bfm=o.detach().clone()))
        with torch.no_grad():
            logits = m(x)
        gold[f"{name}/logits"] = logits.numpy()
        p_ref = torch.sigmoid(logits)
        print(name, "logits", logits.numpy().tolist(), "probs", p_ref.numpy().tolist(), flush=True)
        assert float(p_ref.min()) >= MARGIN and float(p_ref.max()) <= 1 - MARGIN, f"{name}: a golden probability is saturated"
        for k in R.BFM_MAPS:
            _summ(gold, f"{name}/{k}", got[k])
        f, blk = got["pool5"], got["bfm"]
        ops = R.bfm_fold(sd)
        ratio, mixed = float(blk.norm() / f.norm()), R.bfm_mixed_sign(f, ops)
        d_blk = float((R.bfm_block(f, ops, dtype=torch.float32) - blk).abs().max())
        print(f"BFM: ||BFM(f)||/||f|| {ratio:.3f}; mixed-sign share {mixed:.3f}; bfm_block fp32 vs the reference module: "
              f"max|d| {d_blk:.3e} at output scale {float(blk.abs().mean()):.3e}", flush=True)
        assert 0.25 <= ratio <= 4, ratio
        assert mixed >= 0.25, mixed
        env[name] = {}
        out32 = R.forward_fp32(name, sd, x)
        env[name]["fp32"] = float((out32 - logits).abs().max())
        # fact 1 on the real module: other TFAM weights, the same logits
        sd2 = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
        for k, v in sd2.items():
            if ".tfam." in k:
                sd2[k] = torch.from_numpy(uniform(k, v.numel(), TFAM_REDRAW_SEED).reshape(tuple(v.shape)).copy())
                assert not torch.equal(sd2[k], v)
        m.load_state_dict(sd2)
        with torch.no_grad():
            env[name]["tfam_sensitivity"] = float((m(x) - logits).abs().max())
        print(name, "forward_fp32 vs the reference class: max |dlogit|", env[name]["fp32"],
              "; TFAM redrawn: max |dlogit|", env[name]["tfam_sensitivity"], flush=True)
        assert env[name]["tfam_sensitivity"] <= env[name]["fp32"], env[name]
        for dt in ("fp16", "bf16"):
            env[name][dt] = float((torch.sigmoid(R.forward_emulated(name, sd, x, dtype=dt)) - p_ref).abs().max())
        env[name]["model_route"] = R.MODEL_ROUTE
        env[name]["bfm_block"] = {"fused": {}, "composed": {}}
        for dt in ("fp16", "bf16"):
            rnd = lambda t, dt=dt: R.round_to(t, dt)  # noqa: E731
            ops16 = {k: (v if k == "bias3" else rnd(v)) for k, v in ops.items()}
            ref16 = R.bfm_block(rnd(f), ops16)
            for route in ("fused", "composed"):
                e = R.bfm_block(rnd(f), ops16, dtype=torch.float32, round=dt, route=route).double() - ref16
                env[name]["bfm_block"][route][dt] = {"rel_l2": float(e.norm() / ref16.norm()),
                                                     "max_abs": float(e.abs().max())}
        print(name, "envelope", env[name], flush=True)
    if args.dry_run:
        return
    (OUT / "bfm_keys.json").write_text(json.dumps(keys))
    np.savez_compressed(OUT / "bfm_golden.npz", **gold)
    (OUT / "bfm_envelope.json").write_text(json.dumps(env, indent=1))


if __name__ == "__main__":
    main()
