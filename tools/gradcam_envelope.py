"""Write tests/golden/gradcam_envelope.json: how far 16-bit rounding alone moves
the Grad-CAM heatmap of each fixture, and the order term of the GPU gate.

envelope[model][dtype][category]: max|delta heatmap| (over the four fixture
crops, at the fixture's sampled pixels) between the fp32 golden
(tests/golden/gradcam_<model>.npz, made by the reference's GradCAM) and the
CPU restatement (tests/gradcam_ref.py) run with that dtype's roundings from
the input on: premap() emulates the conv stack the way the oracle's
forward_emulated does, gradcam() rounds the tail's GEMM inputs
straight-through.  Runs on the CPU.  A bf16 envelope above 0.1 is reported:
the plan was to replace such a crop, but with the seed-0 synthetic weights
every one of 16 candidate crops exceeds it for RepBn8 (0.18 .. 0.37) and all
but one for the base CViT (0.10 .. 0.34), so the probe crops stay and the
envelope is recorded as measured.

order_term[model][dtype]: what fp32 summation order inside the EXISTING conv
kernels does to the heatmap.  ``--maps FILE.npz`` names a dump of the
pre-ReLU map A taken on an MI355X from the conv kernels of commit
``--commit`` (keys ``<model>_<dtype>`` = A as fp32 [4,512,14,14] for the
fixture's crops; made with entry points that commit already had:
fac_debug_features_u8 / fac_stem224 + fac_conv3x3).  That A and the emulated A
both go through the fp32 restatement without any further rounding; the term
is the max|delta heatmap| between the two over both categories.  Without
``--maps`` the stored order terms are kept.

The GPU heatmap gate (tests/test_gradcam_gpu.py) is 1.25 x envelope + order term.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gradcam_ref as G  # noqa: E402
from fac_fake_amd.weights import make_repbn8_state_dict, make_state_dict  # noqa: E402
from oracle.cvit_torch import normalize_u8  # noqa: E402

OUT = REPO / "tests" / "golden" / "gradcam_envelope.json"
MODELS = ("cvit", "repbn8")
DTYPES = ("fp16", "bf16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=Path, default=None)
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    old = json.loads(OUT.read_text()) if OUT.exists() else {}
    res = {"envelope": {}, "order_term": old.get("order_term", {}), "order_term_commit": old.get("order_term_commit"),
           "order_term_box": old.get("order_term_box")}
    maps = dict(np.load(args.maps)) if args.maps else None
    if maps is not None:
        assert args.commit, "--maps needs --commit (the commit whose conv kernels made the maps)"
        res["order_term"], res["order_term_commit"], res["order_term_box"] = {}, args.commit, "MI355X (gfx950)"
    for model in MODELS:
        g = dict(np.load(G.GOLDEN / f"gradcam_{model}.npz"))
        s = int(g["heat_stride"])
        sd = make_state_dict(0) if model == "cvit" else make_repbn8_state_dict(0)
        x = normalize_u8(G.crops_of(g["crop_src"]))
        res["envelope"][model] = {}
        for dt in DTYPES:
            a16 = G.premap(sd, x, model, dtype=dt)
            env = {}
            for cat in (0, 1):
                r = G.gradcam(sd, a16, model, target_category=cat, dtype=dt)
                env[str(cat)] = float(np.abs(r["heatmap"][:, ::s, ::s].numpy() - g[f"heat_{cat}"]).max())
            print(f"{model} {dt}: envelope {env}")
            if dt == "bf16" and max(env.values()) > 0.1:
                # With the synthetic weights no crop tried stays below 0.1 in bf16: the
                # gradient's ReLU / max-pool routing flips under bf16 rounding.  Recorded as measured.
                print(f"  note: {model} bf16 envelope {max(env.values()):.3f} > 0.1")
            res["envelope"][model][dt] = env
            if maps is not None:
                a_gpu = torch.from_numpy(maps[f"{model}_{dt}"]).float()
                flips = float((a_gpu != a16).float().mean())
                term = 0.0
                for cat in (0, 1):
                    h0 = G.gradcam(sd, a16, model, target_category=cat)["heatmap"]
                    h1 = G.gradcam(sd, a_gpu, model, target_category=cat)["heatmap"]
                    term = max(term, float((h0 - h1).abs().max()))
                print(f"{model} {dt}: order term {term:.3e} ({flips:.2%} of the map's 16-bit values differ)")
                res["order_term"].setdefault(model, {})[dt] = term
    OUT.write_text(json.dumps(res, indent=1, sort_keys=True) + "\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
