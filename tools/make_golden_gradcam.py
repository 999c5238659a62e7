"""Generate the Grad-CAM fixtures tests/golden/gradcam_{cvit,repbn8}.npz from the
REFERENCE's own code.

Runs only where the reference tree exists.  The models are the reference
classes (``CViT-main/model/cvit.py``; ``cvit_GGCA_ADD_DEConv_RepBn8.py`` loaded
the way tools/make_golden_repbn8.py loads it) with the seed-0 synthetic
weights; ``ActivationsAndGradients`` and ``GradCAM`` are taken from
``CViT-main/figure/utils.py`` by ``ast``, unchanged.  cv2 is not installed
here, so the name ``cv2`` in that code is bound to a shim whose ``resize`` is
the bilinear restatement of tests/gradcam_ref.py (cv2's INTER_LINEAR formula;
parity with cv2 itself stays unpinned, as it is for the crops).

Inputs: the two real crops of golden_real.npz and the first two of
make_crops(8, seed=5), one call of four crops (slots 0..3) per target category
0 and 1, target layer ``features[-3]`` / ``features2[-3]`` as in
figure/gradcam_cnn.py.  A crop whose CAM is degenerate for a model (below) is
replaced, for that model, by the next unused crop of make_crops(8, seed=5);
``crop_src`` records the choice (-1, -2: the real crops; n >= 0: crop n of
make_crops(8, seed=5)).  Recorded per model and category (data only, fp32):

  logits [4,2]; w [4,512], the channel weights (get_cam_weights); cam14
  [4,14,14], the scaled 14x14 map (scale_cam_image without a target size);
  heat [4,75,75], the returned 224x224 heatmap at rows and columns 0, 3, ..,
  222 (a ninth of its pixels keeps the file small: the heatmap is a fixed fp32
  function of cam14, which is recorded whole)

A CAM is degenerate when fewer than 10 % or more than 95 % of cam14's
positions are above 0 (it would test nothing); the script fails if the pool
runs out.
"""
from __future__ import annotations

import ast
import sys
import types
from pathlib import Path

sys.dont_write_bytecode = True
REPO = Path(__file__).resolve().parents[1]
REF = Path("/root/reference/CViT-main")
OUT = REPO / "tests" / "golden"
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch import nn  # noqa: E402

from fac_fake_amd.weights import make_repbn8_state_dict, make_state_dict  # noqa: E402
from gradcam_ref import CROP_SEED, bilinear_resize, crops_of  # noqa: E402
from tools.make_golden import ref_model, ref_normalize  # noqa: E402
from tools.make_golden_repbn8 import load_reference_namespace  # noqa: E402

HEAT_STRIDE = 3


def cv2_shim():
    def resize(img, target_size):
        assert tuple(target_size) == (224, 224) and img.shape == (14, 14)
        return bilinear_resize(torch.from_numpy(np.float32(img))[None], 224)[0].numpy()
    return types.SimpleNamespace(resize=resize, COLORMAP_JET=2)


def ref_gradcam_classes():
    tree = ast.parse((REF / "figure" / "utils.py").read_text(encoding="utf-8"))
    keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in ("ActivationsAndGradients", "GradCAM")]
    ns = {"np": np, "cv2": cv2_shim()}
    exec(compile(ast.Module(body=keep, type_ignores=[]), "figure_utils_classes", "exec"), ns)
    return ns["GradCAM"]


def record(GradCAM, model, layer, x):
    out = {}
    for cat in (0, 1):
        with GradCAM(model=model, target_layers=[layer], use_cuda=False) as cam:
            heat = cam(input_tensor=x, target_category=cat)
            acts = cam.activations_and_grads.activations[0].numpy()
            grads = cam.activations_and_grads.gradients[0].numpy()
            w = cam.get_cam_weights(grads)
            raw = cam.get_cam_image(acts, grads)
            raw[raw < 0] = 0
            cam14 = cam.scale_cam_image(raw)
        with torch.no_grad():
            logits = model(x).numpy()
        pos = (cam14 > 0).reshape(len(cam14), -1).mean(1)
        print(f"  category {cat}: logits {logits.tolist()} positive share {pos.tolist()} max|grad| "
              f"{np.abs(grads).reshape(len(grads), -1).max(1).tolist()}")
        bad = np.nonzero((pos < 0.10) | (pos > 0.95))[0]
        if len(bad):
            return int(bad[0])
        out[f"logits_{cat}"] = logits.astype(np.float32)
        out[f"w_{cat}"] = np.float32(w.reshape(len(w), -1))
        out[f"cam14_{cat}"] = np.float32(cam14)
        out[f"heat_{cat}"] = np.float32(heat[:, ::HEAT_STRIDE, ::HEAT_STRIDE])
    return out


def record_swapping(GradCAM, model, layer):
    """record() on the default crops, replacing a crop whose CAM is degenerate for this model."""
    src, nxt = [-1, -2, 0, 1], 2
    while True:
        fix = record(GradCAM, model, layer, ref_normalize(crops_of(src)))
        if isinstance(fix, dict):
            fix["crop_src"] = np.int64(src)
            return fix
        assert nxt < 8, "no crop of the pool gives a non-degenerate CAM"
        print(f"  crop {fix} (source {src[fix]}) is degenerate here: replaced by pool crop {nxt}")
        src[fix], nxt = nxt, nxt + 1


def main():
    torch.manual_seed(0)
    GradCAM = ref_gradcam_classes()
    to_t = lambda sd: {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}  # noqa: E731

    print("cvit")
    m = ref_model(make_state_dict(0))
    fix = record_swapping(GradCAM, m, m.features[-3])
    np.savez_compressed(OUT / "gradcam_cvit.npz", crop_seed=np.int64(CROP_SEED), heat_stride=np.int64(HEAT_STRIDE),
                        **fix)

    print("repbn8")
    torch.cuda.FloatTensor = lambda *shape: torch.empty(*shape, dtype=torch.float32)  # see make_golden_repbn8.py
    nn.Conv1d.cuda = lambda self, *a, **k: self
    ns = load_reference_namespace()
    m = ns["CViT"](image_size=224, patch_size=7, num_classes=2, channels=512, dim=1024, depth=6, heads=8,
                   mlp_dim=2048).eval()
    m.load_state_dict(to_t(make_repbn8_state_dict(0)))
    fix = record_swapping(GradCAM, m, m.features2[-3])
    np.savez_compressed(OUT / "gradcam_repbn8.npz", crop_seed=np.int64(CROP_SEED), heat_stride=np.int64(HEAT_STRIDE),
                        **fix)
    for f in ("gradcam_cvit.npz", "gradcam_repbn8.npz"):
        print(f, (OUT / f).stat().st_size, "bytes")


if __name__ == "__main__":
    main()
