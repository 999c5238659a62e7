"""The eight CViT variants of fac_fake_amd/variants.py, CPU side.

The variant table, ``variant_param_specs`` and the drop-ins' ``state_dict``
against the reference classes' own keys (tests/golden/variants_keys.json,
tools/make_golden_variants.py); the CPU reference (tests/variants_ref.py)
pinned to the reference's fp32 logits and feature maps; its 16-bit emulation of
the HIP path's rounding points inside the recorded envelope; the ``model/``
import shims; the inference-only / no-CPU-fallback contract.
"""
import importlib
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import variants_ref as R  # noqa: E402
from fac_fake_amd.weights import (REPBN8_LAYERS, VARIANT_NAMES, VARIANTS, make_crops,  # noqa: E402
                                  make_variant_state_dict, repbn8_param_specs, variant_param_specs)
from oracle.cvit_torch import normalize_u8  # noqa: E402

REPO = Path(__file__).resolve().parents[1]
ENVELOPE_MARGIN = 1.25            # drift of the CPU BLAS between hosts (conftest.ENVELOPE_MARGIN)
N_KEYS = {"cvit_DEConv": 350, "cvit_GGCA_ADD": 202, "cvit_GGCA_ADD_DEConv": 305, "cvit_GGCA_ADD_RepBn": 256,
          "cvit_GGCA_ADD_DEConv_RepBn": 306, "cvit_GGCA_ADD_DEConv_RepBn3": 306, "cvit_GGCA_ADD_DEConv_RepBn4": 335,
          "cvit_GGCA_ADD_DEConv_RepBn5": 359}


def _sd_t(name):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in make_variant_state_dict(name, 0).items()}


def test_the_eight_variants_are_listed(golden):
    assert set(VARIANT_NAMES) == set(N_KEYS) == set(golden("variants_keys.json")) == set(R.NAMES)
    assert "cvit_GGCA_ADD_DConv" not in VARIANTS and "cvit_GGCA_ADD_DEConv_RepBn8" not in VARIANTS


def test_table_matches_the_cpu_reference_and_repbn8():
    """The library's table and the reference's independent restatement agree;
    RepBn5's stem is RepBn8's, key for key."""
    for name in VARIANT_NAMES:
        v, (layers, g, ff) = VARIANTS[name], R.TABLE[name]
        assert v["layers"] == layers, name
        assert v["ggca"] == g, name
        assert (v["ff_norm"] == "linearnorm") == (ff[1] == 1e-6), name
    assert VARIANTS["cvit_GGCA_ADD_DEConv_RepBn5"]["layers"] == REPBN8_LAYERS
    assert variant_param_specs("cvit_GGCA_ADD_DEConv_RepBn5") == repbn8_param_specs()
    assert VARIANTS["cvit_GGCA_ADD_DEConv_RepBn3"]["ggca"] == ("features1", (64, 56, 56), "add")


@pytest.mark.parametrize("name", VARIANT_NAMES)
def test_param_specs_are_the_reference_layout(golden, name):
    want = golden("variants_keys.json")[name]
    got = [[n, list(s)] for n, s, _ in variant_param_specs(name)]
    assert got == want and len(got) == N_KEYS[name]


@pytest.mark.parametrize("name", VARIANT_NAMES)
def test_dropin_state_dict_layout_and_contract(golden, name):
    from fac_fake_amd import variants
    m = variants.CViT(name, image_size=224, patch_size=7, num_classes=2, channels=512, dim=1024, depth=6, heads=8,
                      mlp_dim=2048)
    sd = m.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == golden("variants_keys.json")[name]
    if VARIANTS[name]["ff_norm"] == "linearnorm":
        assert int(sd["transformer.layers.0.1.fn.norm.total_step"]) == 300000
    m.load_state_dict(_sd_t(name))
    assert not m.training and type(m) is variants.variant_class(name)
    with pytest.raises(RuntimeError):
        m.train()
    with pytest.raises(RuntimeError):          # no CPU fallback
        m(torch.zeros(1, 3, 224, 224))
    with pytest.raises(RuntimeError):
        m.forward_u8(torch.zeros(1, 224, 224, 3, dtype=torch.uint8))
    with pytest.raises(NotImplementedError):   # only the reference's default configuration
        variants.CViT(name, depth=4)


def test_unknown_variant_and_gradcam_are_refused():
    from fac_fake_amd import variants
    from fac_fake_amd.gradcam import GradCAM
    with pytest.raises(KeyError):
        variants.CViT("cvit_GGCA_ADD_DConv")
    with pytest.raises(NotImplementedError):
        GradCAM(variants.CViT("cvit_GGCA_ADD"))


@pytest.mark.parametrize("name", VARIANT_NAMES)
def test_model_shim_imports_and_constructs(name):
    """`sys.path.insert(1, 'model'); from <name> import CViT` as the reference's scripts do."""
    from fac_fake_amd import variants
    sys.path.insert(1, str(REPO / "model"))
    try:
        mod = importlib.import_module(name)
    finally:
        sys.path.remove(str(REPO / "model"))
    assert mod.CViT is variants.variant_class(name)
    m = mod.CViT(image_size=224, patch_size=7, num_classes=2, channels=512, dim=1024, depth=6, heads=8, mlp_dim=2048)
    assert len(m.state_dict()) == N_KEYS[name] and m.variant == name


def test_prediction_script_takes_a_model_name():
    import cvit_prediction as P
    assert P.model_class(None).__module__ == "fac_fake_amd.cvit"
    assert P.model_class("cvit").__module__ == "fac_fake_amd.cvit"
    assert P.model_class("cvit_GGCA_ADD_DEConv_RepBn8").__module__ == "fac_fake_amd.repbn8"
    for name in VARIANT_NAMES:
        from fac_fake_amd import variants
        assert P.model_class(name) is variants.variant_class(name)
    with pytest.raises(SystemExit):
        P.main(["--model", "cvit_GGCA_ADD_DConv"])


@pytest.fixture(scope="module")
def fp32_runs(torch_threads):
    """(logits, GGCA input map, combined map) of the fp32 reference, per variant, computed once."""
    x = normalize_u8(make_crops(4, seed=31))
    return {name: R.forward_fp32(name, make_variant_state_dict(name, 0), x, return_features=True)
            for name in VARIANT_NAMES}


@pytest.mark.parametrize("name", VARIANT_NAMES)
def test_cpu_reference_matches_reference_goldens(golden, fp32_runs, name):
    g = golden("variants_golden.npz")
    assert int(g["crop_seed"]) == 31
    out, pre, comb = fp32_runs[name]
    assert np.abs(out.numpy() - g[f"{name}.logits"]).max() <= 1e-5   # CPU BLAS differs across hosts
    assert np.isclose(pre.double().sum().item(), float(g[f"{name}.pre_sum"]), rtol=1e-6)
    assert np.allclose(pre.numpy().reshape(-1)[::997], g[f"{name}.pre_sample"], rtol=1e-5, atol=1e-6)
    if VARIANTS[name]["ggca"] is None:
        assert comb is None and f"{name}.combined_sum" not in g
        return
    assert tuple(pre.shape[1:]) == VARIANTS[name]["ggca"][1]
    assert np.isclose(comb.double().sum().item(), float(g[f"{name}.combined_sum"]), rtol=1e-6)
    assert np.allclose(comb.numpy().reshape(-1)[::997], g[f"{name}.combined_sample"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", VARIANT_NAMES)
def test_emulation_stays_inside_the_recorded_envelope(golden, torch_threads, name):
    """The HIP path's rounding points (emulated) against the fp32 reference's
    probabilities: the recorded envelope, which the GPU test doubles."""
    env = golden("variants_envelope.json")[name]
    x = normalize_u8(make_crops(4, seed=31))
    p_ref = torch.sigmoid(torch.from_numpy(golden("variants_golden.npz")[f"{name}.logits"]))
    sd = make_variant_state_dict(name, 0)
    for dt in ("fp16", "bf16"):
        d = float((torch.sigmoid(R.forward_emulated(name, sd, x, dtype=dt)) - p_ref).abs().max())
        print(f"{name} {dt}: emulated max|dp| {d:.3e}, recorded {env[dt]:.3e}")
        assert 0 < env[dt] and d <= ENVELOPE_MARGIN * env[dt], (name, dt)


def test_ggca_reference_is_the_oracles_on_7x7(torch_threads):
    """variants_ref.ggca generalises oracle.repbn8_torch.ggca: same bits on the 7x7x512 site."""
    from oracle import repbn8_torch as O
    from oracle.cvit_torch import to_torch_sd
    sd = to_torch_sd(make_variant_state_dict("cvit_GGCA_ADD_DEConv_RepBn5", 0))
    x = torch.randn(2, 512, 7, 7, generator=torch.Generator().manual_seed(3))
    assert torch.equal(R.ggca(R.ggca_weights(sd), x), O.ggca(sd, x))


def test_envelope_file_is_complete(golden):
    env = json.loads((REPO / "tests" / "golden" / "variants_envelope.json").read_text())
    assert set(env) == set(VARIANT_NAMES) and all(set(v) == {"fp16", "bf16"} for v in env.values())
