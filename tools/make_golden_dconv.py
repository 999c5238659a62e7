"""Generate the fixtures of cvit_GGCA_ADD_DConv (fac_fake_amd/dconv.py) under
tests/golden/ from the REFERENCE's own class code.

Needs the reference checkout (``--reference DIR`` or $FAC_REFERENCE_DIR: the
directory that holds ``CViT-main/``), so it runs only where that exists.  Like
tools/make_golden_variants.py it parses ``CViT-main/model/cvit_GGCA_ADD_DConv.py``
with ``ast`` and executes its imports, module-level assignments and class
definitions unchanged, on the CPU.

The fixtures are data only (no reference source), on make_dconv_state_dict(0)
and 4 make_crops crops (seed 31, slots 0..3):

  dconv_keys.json      the reference state_dict's 238 keys and shapes, in order
  dconv_golden.npz     the fp32 logits; for the map after each of the five
                       MaxPool2d ("pool1".."pool5") and after x + GGCA(x)
                       ("combined"): its float64 sum and every 997th value
  dconv_envelope.json  per dtype, the largest probability difference between
                       those logits and tests/dconv_ref.py's 16-bit emulation

It asserts the condition on the synthetic weights: no golden probability
within 0.05 of 0 or 1 (weights.DCONV_DW_GAIN is what to adjust).
"""
from __future__ import annotations

import argparse
import ast
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
from torch import nn  # noqa: E402

import dconv_ref as R  # noqa: E402
from fac_fake_amd.weights import make_crops, make_dconv_state_dict  # noqa: E402
from tools.make_golden import ref_normalize  # noqa: E402

CROP_SEED = 31
STRIDE = 997
MARGIN = 0.05


def load_reference_class(ref_dir: Path):
    ref = ref_dir / "CViT-main" / "model" / f"{R.NAME}.py"
    tree = ast.parse(ref.read_text(), filename=str(ref))
    keep = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom, ast.ClassDef, ast.Assign))]
    ns = {"__name__": f"{R.NAME}_reference"}
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
    m = load_reference_class(Path(args.reference))(image_size=224, patch_size=7, num_classes=2, channels=512, dim=1024,
                                                   depth=6, heads=8, mlp_dim=2048).eval()
    keys = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    sd = make_dconv_state_dict(0)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    maps, got = [], {}
    for mod in m.features:
        if isinstance(mod, nn.MaxPool2d):
            mod.register_forward_hook(lambda _m, _i, o: maps.append(o.detach().clone()))
    m.ggca.register_forward_hook(lambda _m, i, o: got.update(combined=(i[0] + o).detach().clone()))
    with torch.no_grad():
        logits = m(x)
    assert len(maps) == 5
    gold = {"crop_seed": np.int64(CROP_SEED), "logits": logits.numpy()}
    for name, t in [(f"pool{i + 1}", t) for i, t in enumerate(maps)] + [("combined", got["combined"])]:
        a = t.numpy()
        gold[f"{name}_sum"] = np.float64(a.astype(np.float64).sum())
        gold[f"{name}_sample"] = a.reshape(-1)[::STRIDE].copy()
        print(name, tuple(a.shape), "mean|x|", float(np.abs(a).mean()), "max|x|", float(np.abs(a).max()), flush=True)
    p_ref = torch.sigmoid(logits)
    print("logits", logits.numpy().tolist(), "probs", p_ref.numpy().tolist(), flush=True)
    assert float(p_ref.min()) >= MARGIN and float(p_ref.max()) <= 1 - MARGIN, "a golden probability is saturated"
    d = float((R.forward_fp32(sd, x) - logits).abs().max())
    print("dconv_ref fp32 vs the reference class: max |dlogit|", d, flush=True)
    env = {}
    for dt in ("fp16", "bf16"):
        env[dt] = float((torch.sigmoid(R.forward_emulated(sd, x, dtype=dt)) - p_ref).abs().max())
    print("envelope", env, flush=True)
    if args.dry_run:
        return
    (OUT / "dconv_keys.json").write_text(json.dumps(keys))
    np.savez_compressed(OUT / "dconv_golden.npz", **gold)
    (OUT / "dconv_envelope.json").write_text(json.dumps(env, indent=1))


if __name__ == "__main__":
    main()
