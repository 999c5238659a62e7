"""Generate the ResKan fixtures under tests/golden/ from the REFERENCE itself.

Runs only where the reference checkout is present (it does not exist on the
GPU box).  It imports ``CViT-main/ResKan/kan_resnet.py`` (and its ``kan.py``)
with empty stand-ins for ``torchvision`` / ``torchvision.transforms``, which
the file imports at its top and never uses in the model, loads the repo's
deterministic synthetic weights (fac_fake_amd.weights.make_reskan_state_dict,
seed 0) and records the reference's outputs.  Data only, no reference source:

  reskan_keys.json          the reference state_dict's keys and shapes, in order
  reskan_golden_stages.npz  8 content-varied crops (reskan_crops_varied seed
                            47): logits; for the max-pool, each of the 16
                            BasicBlocks and the pooled features, the
                            per-channel mean over (H, W) of its output; the
                            16-bit rounding envelope of each (tests/
                            reskan_ref.py's emulation of the HIP path's
                            rounding points vs the reference), of the
                            probabilities and of the logits; the seeds; the
                            fixture statistics asserted below.

A fixture on which the KAN head is saturated, sees only its inner interval, or
scores every crop alike proves nothing about the head, so this asserts: every
|logit| <= 4; each logit's range over the crops >= 20x its fp16 logit
envelope; >= 50 % of the pooled features in [0, 1), >= 90 % below 2.2, >= 1 %
above 1; the emulated fp16 probability envelope <= 5e-4.
"""
from __future__ import annotations

import json
import sys
import types
from pathlib import Path

sys.dont_write_bytecode = True
REPO = Path(__file__).resolve().parents[1]
REF = Path("/root/reference/CViT-main/ResKan")
OUT = REPO / "tests" / "golden"
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fac_fake_amd.weights import make_reskan_state_dict, reskan_crops_varied  # noqa: E402
from tools.make_golden import ref_normalize  # noqa: E402

WEIGHT_SEED, CROP_SEED, N_CROPS = 0, 47, 8


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.sqrt((b.astype(np.float64) ** 2).mean()) + 1e-30))


def reference_module():
    for name in ("torchvision", "torchvision.transforms"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    sys.path.insert(0, str(REF))
    import kan_resnet as K  # the reference module (imports kan.py from the same directory)
    return K.resnet34(set_device="cpu", num_classes=2, include_top=False, include_top_kan=True).eval()


def main(write: bool = True):
    import reskan_ref as R
    torch.manual_seed(0)
    m = reference_module()
    keys = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    sd = make_reskan_state_dict(WEIGHT_SEED)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})

    x = ref_normalize(reskan_crops_varied(N_CROPS, seed=CROP_SEED))
    taps = []
    mods = [m.maxpool] + [blk for layer in (m.layer1, m.layer2, m.layer3, m.layer4) for blk in layer] + [m.avgpool]
    hooks = [md.register_forward_hook(lambda mod, i, o: taps.append(o.detach().clone())) for md in mods]
    with torch.no_grad():
        logits = m(x).numpy()
    for hk in hooks:
        hk.remove()
    assert len(taps) == 18
    taps[-1] = torch.flatten(taps[-1], 1)
    means = R.tap_means(taps)
    pooled = means[-1]
    out = {"weight_seed": np.int64(WEIGHT_SEED), "crop_seed": np.int64(CROP_SEED), "n_crops": np.int64(N_CROPS),
           "logits": logits}
    for i, mu in enumerate(means):
        out[f"mean_{i}"] = mu.astype(np.float32)
    p_ref = 1 / (1 + np.exp(-logits.astype(np.float64)))
    for dt in ("fp16", "bf16"):
        et = []
        R.features_emulated(sd, x, dt, et)
        out[f"env_{dt}"] = np.array([_rel(a, mu) for a, mu in zip(R.tap_means(et), means)])
        le = R.forward_emulated(sd, x, dt).double().numpy()
        out[f"env_logit_{dt}"] = np.abs(le - logits.astype(np.float64)).max(axis=0)
        out[f"env_prob_{dt}"] = np.float64(np.abs(1 / (1 + np.exp(-le)) - p_ref).max())
        print(dt, "env", np.round(out[f"env_{dt}"], 5), "logit", out[f"env_logit_{dt}"], "prob", out[f"env_prob_{dt}"])

    stats = {"logit_abs_max": float(np.abs(logits).max()),
             "logit_range": (logits.max(axis=0) - logits.min(axis=0)).astype(np.float64),
             "pooled_in_0_1": float(((pooled >= 0) & (pooled < 1)).mean()),
             "pooled_below_2p2": float((pooled < 2.2).mean()),
             "pooled_above_1": float((pooled > 1).mean())}
    print("logits", np.round(logits, 4).tolist())
    print("probs", np.round(p_ref, 4).tolist())
    print("stats", stats, "pooled mean", float(pooled.mean()), "max", float(pooled.max()))
    assert stats["logit_abs_max"] <= 4, stats
    assert (stats["logit_range"] >= 20 * out["env_logit_fp16"]).all(), (stats, out["env_logit_fp16"])
    assert stats["pooled_in_0_1"] >= 0.5 and stats["pooled_below_2p2"] >= 0.9 and stats["pooled_above_1"] >= 0.01, stats
    assert out["env_prob_fp16"] <= 5e-4, out["env_prob_fp16"]
    for k, v in stats.items():
        out[f"stat_{k}"] = np.asarray(v, np.float64)
    if write:
        (OUT / "reskan_keys.json").write_text(json.dumps(keys))
        np.savez_compressed(OUT / "reskan_golden_stages.npz", **out)
        print("wrote", OUT / "reskan_keys.json", OUT / "reskan_golden_stages.npz")


if __name__ == "__main__":
    main(write="--dry" not in sys.argv)
