"""Grad-CAM on the CPU: the torch restatement (tests/gradcam_ref.py) against the
fixtures made from the reference's own GradCAM code (tests/golden/gradcam_*.npz,
tools/make_golden_gradcam.py).  No GPU, no library.

Metric: max|delta| on cam14 and on the (sampled) heatmap, both in [0, 1].
Yardstick: the same metric between the restatement run in float64 and in
float32 from the same fp32 map A; the gate is 4x the yardstick, because two
valid fp32 summation orders differ by a small factor.

Measured on the CPU (the four fixture crops; category 0 / category 1):
  cvit    yardstick cam14 1.94e-06 / 1.11e-06, heatmap 1.90e-06 / 1.22e-06;
          fp32 restatement vs golden cam14 1.03e-06 / 1.37e-06, heatmap 9.69e-07 / 1.43e-06
  repbn8  yardstick cam14 1.44e-06 / 1.19e-06, heatmap 1.43e-06 / 1.16e-06;
          fp32 restatement vs golden cam14 6.56e-07 / 9.54e-07, heatmap 7.15e-07 / 8.64e-07
The channel weights w agree with the golden to 2.5e-07 of max|w|, the logits bit for bit.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gradcam_ref as G
from fac_fake_amd.weights import make_repbn8_state_dict, make_state_dict
from oracle.cvit_torch import normalize_u8

MODELS = ("cvit", "repbn8")
GATE = 4.0


@pytest.fixture(scope="module")
def runs(golden, torch_threads):
    """Per model: the golden, and the restatement in fp32 and float64 per category (computed once)."""
    out = {}
    for model in MODELS:
        g = golden(f"gradcam_{model}.npz")
        sd = make_state_dict(0) if model == "cvit" else make_repbn8_state_dict(0)
        a = G.premap(sd, normalize_u8(G.crops_of(g["crop_src"])), model)
        res = {cat: {p: G.gradcam(sd, a, model, target_category=cat, prec=p) for p in (torch.float32, torch.float64)}
               for cat in (0, 1)}
        out[model] = (g, res)
    return out


@pytest.mark.parametrize("model", MODELS)
def test_fixture_cams_are_not_degenerate(golden, model):
    g = golden(f"gradcam_{model}.npz")
    for cat in (0, 1):
        share = (g[f"cam14_{cat}"] > 0).reshape(4, -1).mean(1)
        assert ((share >= 0.10) & (share <= 0.95)).all(), (model, cat, share)
        assert g[f"heat_{cat}"].shape == (4, 75, 75) and int(g["heat_stride"]) == 3


@pytest.mark.parametrize("model", MODELS)
def test_restatement_matches_reference_gradcam(runs, model):
    g, res = runs[model]
    s = int(g["heat_stride"])
    for cat in (0, 1):
        r32, r64 = res[cat][torch.float32], res[cat][torch.float64]
        y_cam = float((r32["cam14"].double() - r64["cam14"]).abs().max())
        y_heat = float((r32["heatmap"].double() - r64["heatmap"]).abs().max())
        d_cam = float(np.abs(r32["cam14"].numpy() - g[f"cam14_{cat}"]).max())
        d_heat = float(np.abs(r32["heatmap"][:, ::s, ::s].numpy() - g[f"heat_{cat}"]).max())
        d_w = float(np.abs(r32["w"].numpy() - g[f"w_{cat}"]).max() / np.abs(g[f"w_{cat}"]).max())
        d_logit = float(np.abs(r32["logits"].numpy() - g[f"logits_{cat}"]).max())
        print(f"{model} category {cat}: yardstick cam14 {y_cam:.2e} heat {y_heat:.2e}; vs golden cam14 {d_cam:.2e} "
              f"heat {d_heat:.2e} w {d_w:.2e} logits {d_logit:.2e}")
        assert y_cam > 0 and y_heat > 0
        assert d_cam <= GATE * y_cam, (model, cat, d_cam, y_cam)
        assert d_heat <= GATE * y_heat, (model, cat, d_heat, y_heat)
        assert d_logit <= 1e-5


def test_bilinear_resize_is_interpolate():
    """The cv2.resize restatement the goldens were made with against torch's bilinear upsampling
    (align_corners=False): the same formula when upscaling, up to fp32 rounding of the two lerps."""
    g = torch.Generator().manual_seed(11)
    m = torch.rand(3, 14, 14, generator=g)
    m[1] = 0.0
    m[1, 13, 13] = 1.0          # a corner peak: the clamped edges
    ours = G.bilinear_resize(m, 224)
    ref = F.interpolate(m[:, None], size=(224, 224), mode="bilinear", align_corners=False)[:, 0]
    assert ours.shape == ref.shape == (3, 224, 224)
    assert float((ours - ref).abs().max()) <= 4 * 2.0 ** -24
    assert float(ours[1, 223, 223]) == 1.0 and float(ours[1, 0, 0]) == 0.0


def test_straight_through_rounding_passes_the_gradient():
    x = torch.tensor([0.1, 1.0 + 2.0 ** -12, -3.3], requires_grad=True)
    y = G.ste(x, "bf16")
    assert torch.equal(y.detach(), x.detach().to(torch.bfloat16).float())
    (y * torch.tensor([1.0, 2.0, 3.0])).sum().backward()
    assert torch.equal(x.grad, torch.tensor([1.0, 2.0, 3.0]))


def test_kernel_references_agree_with_closed_forms():
    """The per-kernel autograd references against formulas written out by hand (float64)."""
    g = torch.Generator().manual_seed(3)
    pre = torch.randn(64, generator=g, dtype=torch.float64)
    dh = torch.randn(64, generator=g, dtype=torch.float64)
    want = dh * (0.5 * (1 + torch.erf(pre / 2 ** 0.5)) + pre * torch.exp(-pre * pre / 2) / (2 * torch.pi) ** 0.5)
    assert float((G.gelu_bwd(pre, dh) - want).abs().max()) < 1e-14
    a = torch.tensor([[[[1.0, 1.0], [1.0, 1.0]]], [[[-1.0, -2.0], [-3.0, -0.5]]]])   # equal positives; all negative
    da = G.relu_pool_bwd(a, torch.ones(2, 1, 1, 1))
    assert da[0].flatten().tolist() == [1.0, 0.0, 0.0, 0.0] and float(da[1].abs().sum()) == 0.0
