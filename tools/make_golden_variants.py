"""Generate the fixtures of the eight CViT variants (fac_fake_amd/variants.py)
under tests/golden/ from the REFERENCE's own class code.

Runs only in the build container (it reads /root/reference, which does not
exist on the GPU box).  Like tools/make_golden_repbn8.py, whose header gives
the reasons, it parses each ``CViT-main/model/<name>.py`` with ``ast``, keeps
its imports except ``torchsummary``, its module-level assignments and every
class definition, unchanged, and executes them with two substitutions that do
not touch the arithmetic:

  * ``torch.cuda.FloatTensor(*shape)`` -> a CPU fp32 tensor of that shape
  * ``nn.Conv1d.cuda()`` -> returns the module unchanged (stays on the CPU)

The fixtures are data only (no reference source):

  variants_keys.json      per variant, the reference state_dict's keys and
                          shapes, in order
  variants_golden.npz     per variant (keys "<name>.<what>"), on
                          make_variant_state_dict(name, 0) and 4 make_crops
                          crops (seed 31, slots 0..3): the fp32 logits; sum and
                          every 997th value of the GGCA's input map (the stem
                          output; RepBn3: features1's 56x56 map) and of that map
                          after the variant's x * GGCA(x) / x + GGCA(x)
  variants_envelope.json  per variant and dtype, the largest probability
                          difference between those fp32 logits and
                          tests/variants_ref.py's 16-bit emulation on the crops
"""
from __future__ import annotations

import ast
import json
import sys
from pathlib import Path

sys.dont_write_bytecode = True
REPO = Path(__file__).resolve().parents[1]
REF_DIR = Path("/root/reference/CViT-main/model")
OUT = REPO / "tests" / "golden"
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch import nn  # noqa: E402

from fac_fake_amd.weights import VARIANT_NAMES, VARIANTS, make_crops, make_variant_state_dict  # noqa: E402
import variants_ref as R  # noqa: E402
from tools.make_golden import ref_normalize  # noqa: E402

CROP_SEED = 31
STRIDE = 997


def load_reference_namespace(name: str):
    ref = REF_DIR / f"{name}.py"
    tree = ast.parse(ref.read_text(), filename=str(ref))
    keep = []
    for node in tree.body:
        if isinstance(node, (ast.Import, ast.ImportFrom)):
            mods = [a.name for a in node.names] + ([node.module] if isinstance(node, ast.ImportFrom) else [])
            if any(m and m.startswith("torchsummary") for m in mods):
                continue
            keep.append(node)
        elif isinstance(node, (ast.ClassDef, ast.Assign)):
            keep.append(node)
    ns = {"__name__": f"{name}_reference"}
    exec(compile(ast.Module(body=keep, type_ignores=[]), str(ref), "exec"), ns)
    return ns


def main():
    torch.manual_seed(0)
    torch.set_num_threads(16)
    torch.cuda.FloatTensor = lambda *shape: torch.empty(*shape, dtype=torch.float32)  # CPU scratch
    nn.Conv1d.cuda = lambda self, *a, **k: self
    crops = make_crops(4, seed=CROP_SEED)
    x = ref_normalize(crops)
    keys, gold, env = {}, {"crop_seed": np.int64(CROP_SEED)}, {}
    for name in VARIANT_NAMES:
        m = load_reference_namespace(name)["CViT"](image_size=224, patch_size=7, num_classes=2, channels=512,
                                                   dim=1024, depth=6, heads=8, mlp_dim=2048).eval()
        keys[name] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        sd = make_variant_state_dict(name, 0)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
        got = {}
        site = VARIANTS[name]["ggca"]
        if site is not None:
            # the map GGCA sees, and the caller's combine recomputed from GGCA's own output
            m.ggca.register_forward_hook(lambda mod, i, o: got.update(pre=i[0].detach().clone(), g=o.detach().clone()))
        else:
            m.features2.register_forward_hook(lambda mod, i, o: got.update(pre=o.detach().clone()))
        with torch.no_grad():
            logits = m(x)
        pre = got["pre"].numpy()
        gold[f"{name}.logits"] = logits.numpy()
        gold[f"{name}.pre_sum"] = np.float64(pre.astype(np.float64).sum())
        gold[f"{name}.pre_sample"] = pre.reshape(-1)[::STRIDE].copy()
        if site is not None:
            comb = (got["pre"] * got["g"] if site[2] == "mul" else got["pre"] + got["g"]).numpy()
            gold[f"{name}.combined_sum"] = np.float64(comb.astype(np.float64).sum())
            gold[f"{name}.combined_sample"] = comb.reshape(-1)[::STRIDE].copy()
        p_ref = torch.sigmoid(logits)
        env[name] = {}
        for dt in ("fp16", "bf16"):
            p = torch.sigmoid(R.forward_emulated(name, sd, x, dtype=dt))
            env[name][dt] = float((p - p_ref).abs().max())
        print(name, "logits", logits.numpy().tolist(), "mean|pre|", float(np.abs(pre).mean()), "max|pre|",
              float(np.abs(pre).max()), "envelope", env[name], flush=True)
    (OUT / "variants_keys.json").write_text(json.dumps(keys))
    np.savez_compressed(OUT / "variants_golden.npz", **gold)
    (OUT / "variants_envelope.json").write_text(json.dumps(env, indent=1))


if __name__ == "__main__":
    main()
