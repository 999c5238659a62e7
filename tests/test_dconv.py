"""cvit_GGCA_ADD_DConv (fac_fake_amd/dconv.py), CPU side.

``dconv_param_specs`` and the drop-in's ``state_dict`` against the reference
class's own keys (tests/golden/dconv_keys.json, tools/make_golden_dconv.py); the
CPU reference (tests/dconv_ref.py) pinned to the reference's fp32 logits and
feature maps; its 16-bit emulation of the HIP path's rounding points inside the
recorded envelope; its folded single layer against torch's grouped convs; the
``model/`` import shim and ``cvit_prediction``'s loader; the inference-only /
no-CPU-fallback contract.
"""
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))

import dconv_ref as R  # noqa: E402
from fac_fake_amd.weights import DCONV_LAYERS, dconv_param_specs, make_crops, make_dconv_state_dict  # noqa: E402
from oracle.cvit_torch import normalize_u8  # noqa: E402

REPO = Path(__file__).resolve().parents[1]
ENVELOPE_MARGIN = 1.25            # drift of the CPU BLAS between hosts (conftest.ENVELOPE_MARGIN)
N_KEYS = 238
MAPS = ["pool1", "pool2", "pool3", "pool4", "pool5", "combined"]


def _sd_t():
    return {k: torch.from_numpy(np.asarray(v)) for k, v in make_dconv_state_dict(0).items()}


def test_param_specs_are_the_reference_layout(golden):
    want = golden("dconv_keys.json")
    got = [[n, list(s)] for n, s, _ in dconv_param_specs()]
    assert got == want and len(got) == N_KEYS
    assert [(i, k[0], ci, co, b, p) for i, k, ci, co, b, p in DCONV_LAYERS] == R.LAYERS
    assert sum(k == "idw" for _, k, *_ in DCONV_LAYERS) == 9


def test_synthetic_weights_are_deterministic_and_non_degenerate():
    a, b = make_dconv_state_dict(0), make_dconv_state_dict(0)
    assert list(a) == [n for n, _, _ in dconv_param_specs()]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert not np.array_equal(a["features.3.dwconv_w.weight"], make_dconv_state_dict(1)["features.3.dwconv_w.weight"])
    for k, v in a.items():
        if k.endswith("running_var"):
            assert v.min() >= 0.8 and v.std() > 0.05, k
        if k.endswith("running_mean") or ".dwconv_" in k:
            assert np.abs(v).max() > 0.01, k


def test_dropin_state_dict_layout_and_contract(golden):
    from fac_fake_amd import dconv
    m = dconv.CViT(image_size=224, patch_size=7, num_classes=2, channels=512, dim=1024, depth=6, heads=8,
                   mlp_dim=2048)
    sd = m.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == golden("dconv_keys.json")
    m.load_state_dict(_sd_t())
    assert not m.training and m.variant == "cvit_GGCA_ADD_DConv"
    with pytest.raises(RuntimeError):
        m.train()
    with pytest.raises(RuntimeError):          # no CPU fallback
        m(torch.zeros(1, 3, 224, 224))
    with pytest.raises(RuntimeError):
        m.forward_u8(torch.zeros(1, 224, 224, 3, dtype=torch.uint8))
    with pytest.raises(NotImplementedError):   # only the reference's default configuration
        dconv.CViT(depth=4)
    with pytest.raises(ValueError):
        dconv.CViT(dtype="fp32")
    assert hasattr(m, "reserve") and hasattr(m, "_release")


def test_gradcam_is_refused():
    from fac_fake_amd import dconv
    from fac_fake_amd.gradcam import GradCAM
    with pytest.raises(NotImplementedError):
        GradCAM(dconv.CViT())


def test_model_shim_and_prediction_loader():
    """`sys.path.insert(1, 'model'); from cvit_GGCA_ADD_DConv import CViT` as the reference's scripts do."""
    import cvit_prediction as P
    from fac_fake_amd import dconv
    sys.path.insert(1, str(REPO / "model"))
    try:
        mod = importlib.import_module("cvit_GGCA_ADD_DConv")
    finally:
        sys.path.remove(str(REPO / "model"))
    assert mod.CViT is dconv.CViT
    assert len(mod.CViT().state_dict()) == N_KEYS
    assert P.model_class("cvit_GGCA_ADD_DConv") is dconv.CViT
    before = P.model
    try:
        m = P.load_model(name="cvit_GGCA_ADD_DConv", dev="cpu")
    finally:
        P.model = before
    assert type(m) is dconv.CViT and not m.training
    want = make_dconv_state_dict(0)
    assert all(np.array_equal(v.numpy(), want[k]) for k, v in m.state_dict().items())


def test_folded_operands_match_the_cpu_reference():
    """dconv.idw_fold (what the kernel is given) is dconv_ref.idw_fold, layer by layer."""
    from fac_fake_amd import dconv
    m = dconv.CViT()
    m.load_state_dict(_sd_t())
    sd = _sd_t()
    layers = m.folded_layers()
    assert [l[0] for l in layers] == [k for _, k, *_ in DCONV_LAYERS]
    for (idx, kind, _ci, _co, bn, pool), got in zip(DCONV_LAYERS, layers):
        assert got[-1] == pool
        if kind == "idw":
            want = R.idw_fold(*R._idw_params(sd, f"features.{idx}", f"features.{bn}"))
            for a, b in zip(got[1:-1], want):
                assert torch.equal(a, b), idx


@pytest.fixture(scope="module")
def fp32_run(torch_threads):
    return R.forward_fp32(make_dconv_state_dict(0), normalize_u8(make_crops(4, seed=31)), return_features=True)


def test_cpu_reference_matches_reference_goldens(golden, fp32_run):
    g = golden("dconv_golden.npz")
    assert int(g["crop_seed"]) == 31
    out, maps = fp32_run
    assert np.abs(out.numpy() - g["logits"]).max() <= 1e-5   # CPU BLAS differs across hosts
    p = 1 / (1 + np.exp(-g["logits"]))
    assert p.min() >= 0.05 and p.max() <= 0.95               # the fixture condition on the synthetic weights
    assert [tuple(t.shape[1:]) for t in maps] == [(32, 112, 112), (64, 56, 56), (128, 28, 28), (256, 14, 14),
                                                  (512, 7, 7), (512, 7, 7)]
    for name, t in zip(MAPS, maps):
        assert np.isclose(t.double().sum().item(), float(g[f"{name}_sum"]), rtol=1e-6), name
        assert np.allclose(t.numpy().reshape(-1)[::997], g[f"{name}_sample"], rtol=1e-5, atol=1e-6), name


def test_emulation_stays_inside_the_recorded_envelope(golden, torch_threads):
    """The HIP path's rounding points (emulated) against the fp32 reference's
    probabilities: the recorded envelope, which the GPU test doubles."""
    env = golden("dconv_envelope.json")
    x = normalize_u8(make_crops(4, seed=31))
    p_ref = torch.sigmoid(torch.from_numpy(golden("dconv_golden.npz")["logits"]))
    sd = make_dconv_state_dict(0)
    for dt in ("fp16", "bf16"):
        d = float((torch.sigmoid(R.forward_emulated(sd, x, dtype=dt)) - p_ref).abs().max())
        print(f"{dt}: emulated max|dp| {d:.3e}, recorded {env[dt]:.3e}")
        assert 0 < env[dt] and d <= ENVELOPE_MARGIN * env[dt], dt


@pytest.mark.parametrize("c,h,w", [(32, 9, 13), (64, 12, 6), (256, 4, 16)])
def test_single_idw_layer_matches_torch_grouped_convs(c, h, w):
    """dconv_ref.idw_layer on idw_fold's operands (the kernel's formulation:
    taps over zero-padded shifts, then scale and shift) against
    torch.nn.functional.conv2d(groups=gc) + batch_norm + relu, written out here."""
    g = torch.Generator().manual_seed(c + h)
    u = lambda *s, lo=-1.0, hi=1.0: torch.rand(*s, generator=g) * (hi - lo) + lo  # noqa: E731
    gc = c // 8
    x = torch.randn(2, c, h, w, generator=g) * 1.5
    w_hw, w_w, w_h = u(gc, 1, 3, 3), u(gc, 1, 1, 11), u(gc, 1, 11, 1)
    b_hw, b_w, b_h = u(gc), u(gc), u(gc)
    bn = (u(c, lo=-0.5, hi=0.5), u(c, lo=0.5, hi=1.5), u(c, lo=-1.5, hi=1.5), u(c, lo=-0.5, hi=0.5))
    cid = c - 3 * gc
    y = torch.cat((x[:, :cid], F.conv2d(x[:, cid:cid + gc], w_hw, b_hw, padding=1, groups=gc),
                   F.conv2d(x[:, cid + gc:cid + 2 * gc], w_w, b_w, padding=(0, 5), groups=gc),
                   F.conv2d(x[:, cid + 2 * gc:], w_h, b_h, padding=(5, 0), groups=gc)), 1)
    want = F.relu(F.batch_norm(y, bn[0], bn[1], bn[2], bn[3], False, 0.1, 1e-5))
    assert torch.equal(R.idw_reference(x, w_hw, b_hw, w_w, b_w, w_h, b_h, bn), want)
    ops = R.idw_fold(w_hw, b_hw, w_w, b_w, w_h, b_h, bn)
    got = R.idw_layer(x, *ops, False)
    assert torch.allclose(got, want, rtol=1e-5, atol=2e-5)
    if h % 2 == 0 and w % 2 == 0:
        assert torch.allclose(R.idw_layer(x, *ops, True), F.max_pool2d(want, 2, 2), rtol=1e-5, atol=2e-5)
    # a negative BatchNorm gain makes scale negative: the affine must come before ReLU and the pool
    assert (ops[3] < 0).any()
