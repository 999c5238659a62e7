"""Generate the fixtures of the four model/other/ CViTs (fac_fake_amd/other.py)
under tests/golden/ from the REFERENCE's own class code.

Needs the reference checkout (``--reference DIR`` or $FAC_REFERENCE_DIR: the
directory that holds ``CViT-main/``), so it runs only where that exists.  Like
tools/make_golden_dconv.py it parses ``CViT-main/model/other/<name>.py`` with
``ast`` and executes its imports, module-level assignments and class
definitions unchanged, on the CPU.  ``cvit_GGCA_SMFA.py`` imports
``torchsummary`` (for a ``summary`` it never calls at import); an empty stand-in
module is registered before the exec where the package is not installed.

The fixtures are data only (no reference source), on make_other_state_dict(name,
0) and 4 make_crops crops (seed 41, slots 0..3):

  other_keys.json      per class, the reference state_dict's keys and shapes, in order
  other_golden.npz     per class "<name>/logits": the fp32 logits; for
                       cvit_GGCA_SMFA also the maps after pool4, after x +
                       SMFA(x), after pool5 and after x + GGCA(x)
                       ("cvit_GGCA_SMFA/<map>_sum", "_sample"): the float64
                       sum and every 997th value
  other_envelope.json  per class and dtype, the largest probability difference
                       between those logits and tests/smfa_ref.py's 16-bit
                       emulation; under "smfa_block", per dtype, the relative
                       L2 and max |d| of smfa_block's emulation against its
                       float64 form on the golden pool4 map

It asserts the conditions on the synthetic SMFA weights (weights.SMFA_GAINS and
its neighbours are what to adjust), on the 4 golden crops:
  * ||SMFA(f)|| / ||f|| within 0.25 .. 4;
  * mean |belt var| >= 0.1 mean |alpha (w max + b)|;
  * the gate g takes both signs;
  * no golden probability within 0.05 of 0 or 1 (every class).
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
import torch.nn.functional as F  # noqa: E402

import smfa_ref as R  # noqa: E402
from fac_fake_amd.weights import make_crops, make_other_state_dict  # noqa: E402
from tools.make_golden import ref_normalize  # noqa: E402

CROP_SEED = 41
STRIDE = 997
MARGIN = 0.05


def load_reference_class(ref_dir: Path, name: str):
    ref = ref_dir / "CViT-main" / "model" / "other" / f"{name}.py"
    tree = ast.parse(ref.read_text(), filename=str(ref))
    keep = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom, ast.ClassDef, ast.Assign))]
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


def _summ(gold, key, t):
    a = t.numpy()
    gold[f"{key}_sum"] = np.float64(a.astype(np.float64).sum())
    gold[f"{key}_sample"] = a.reshape(-1)[::STRIDE].copy()
    print(key, tuple(a.shape), "mean|x|", float(np.abs(a).mean()), "max|x|", float(np.abs(a).max()), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("FAC_REFERENCE_DIR"), required="FAC_REFERENCE_DIR" not in os.environ,
                    help="the directory that holds the reference's CViT-main/")
    ap.add_argument("--dry-run", action="store_true", help="print the figures, write nothing")
    ap.add_argument("--only", default=None, help="one class (with --dry-run: tuning the gains)")
    args = ap.parse_args(argv)
    torch.manual_seed(0)
    torch.set_num_threads(16)
    x = ref_normalize(make_crops(4, seed=CROP_SEED))
    keys, gold, env = {}, {"crop_seed": np.int64(CROP_SEED)}, {}
    for name in ([args.only] if args.only else R.NAMES):
        m = load_reference_class(Path(args.reference), name)(image_size=224, patch_size=7, num_classes=2, channels=512,
                                                             dim=1024, depth=6, heads=8, mlp_dim=2048).eval()
        keys[name] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        assert len(keys[name]) == R.N_KEYS[name], (name, len(keys[name]))
        sd = make_other_state_dict(name, 0)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
        got = {}
        if name == "cvit_GGCA_SMFA":
            m.features1.register_forward_hook(lambda _m, _i, o: got.update(pool4=o.detach().clone()))
            m.features2.register_forward_hook(lambda _m, _i, o: got.update(pool5=o.detach().clone()))
            m.smfa.register_forward_hook(lambda _m, i, o: got.update(smfa=(i[0] + o).detach().clone(), block=o.detach().clone()))
            m.ggca.register_forward_hook(lambda _m, i, o: got.update(ggca=(i[0] + o).detach().clone()))
            m.smfa.linear_0.register_forward_hook(lambda _m, _i, o: got.update(t=o.detach().clone()))
            m.smfa.linear_1.register_forward_hook(lambda _m, _i, o: got.update(gate=F.gelu(o.detach().clone())))
        with torch.no_grad():
            logits = m(x)
        gold[f"{name}/logits"] = logits.numpy()
        p_ref = torch.sigmoid(logits)
        print(name, "logits", logits.numpy().tolist(), "probs", p_ref.numpy().tolist(), flush=True)
        assert float(p_ref.min()) >= MARGIN and float(p_ref.max()) <= 1 - MARGIN, f"{name}: a golden probability is saturated"
        if name == "cvit_GGCA_SMFA":
            for k in R.SMFA_MAPS:
                _summ(gold, f"{name}/{k}", got[k])
            f, blk = got["pool4"], got["block"]
            ratio = float(blk.norm() / f.norm())
            xx = got["t"][:, 256:]
            s = m.smfa
            t_max = (s.alpha * (s.dw_conv.weight[:, 0, 1, 1].view(1, -1, 1, 1) * xx.amax(dim=(2, 3), keepdim=True) +
                                s.dw_conv.bias.view(1, -1, 1, 1))).detach().abs().mean()
            t_var = (s.belt * xx.var(dim=(2, 3), keepdim=True)).detach().abs().mean()
            g = got["gate"]
            print(f"SMFA: ||SMFA(f)||/||f|| {ratio:.3f}; mean|belt var| {float(t_var):.4f} vs mean|alpha(w max + b)| "
                  f"{float(t_max):.4f}; gate min {float(g.min()):.4f} max {float(g.max()):.4f} "
                  f"negative share {float((g < 0).float().mean()):.3f}", flush=True)
            assert 0.25 <= ratio <= 4, ratio
            assert float(t_var) >= 0.1 * float(t_max), (float(t_var), float(t_max))
            assert float(g.min()) < 0 < float(g.max())
            ops = R.smfa_fold(sd)
            d = float((R.smfa_block(f, ops, False, dtype=torch.float32) - blk).abs().max())
            print(f"smfa_block fp32 vs the reference module: max|d| {d:.3e} at output scale {float(blk.abs().mean()):.3e}", flush=True)
            env["smfa_block"] = {}
            for dt in ("fp16", "bf16"):
                rnd = lambda t, dt=dt: R.round_to(t, dt)  # noqa: E731
                ops16 = {k: (rnd(v) if k in ("w0", "wpw", "wcat") else v) for k, v in ops.items()}
                ref16 = R.smfa_block(rnd(f), ops16, True)
                e = R.smfa_block(rnd(f), ops16, True, dtype=torch.float32, round=dt).double() - ref16
                env["smfa_block"][dt] = {"rel_l2": float(e.norm() / ref16.norm()), "max_abs": float(e.abs().max())}
        out32, _ = R.forward_fp32(name, sd, x, return_features=True)
        print(name, "smfa_ref fp32 vs the reference class: max |dlogit|", float((out32 - logits).abs().max()), flush=True)
        env[name] = {}
        for dt in ("fp16", "bf16"):
            env[name][dt] = float((torch.sigmoid(R.forward_emulated(name, sd, x, dtype=dt)) - p_ref).abs().max())
        print(name, "envelope", env[name], flush=True)
    print("envelope", env, flush=True)
    if args.dry_run or args.only:
        return
    (OUT / "other_keys.json").write_text(json.dumps(keys))
    np.savez_compressed(OUT / "other_golden.npz", **gold)
    (OUT / "other_envelope.json").write_text(json.dumps(env, indent=1))


if __name__ == "__main__":
    main()
