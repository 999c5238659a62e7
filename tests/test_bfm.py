"""cvit_GGCA4_BFM5 (fac_fake_amd/bfm.py), CPU side.

``bfm_param_specs`` and the drop-in's ``state_dict`` against the reference
class's own keys (tests/golden/bfm_keys.json, tools/make_golden_bfm.py); the
CPU restatement of the block (tests/bfm_ref.py) against the reference's own
``BFM`` module where the reference checkout is present; the CPU reference of
the class pinned to the reference's fp32 logits and maps; its 16-bit emulation
of the HIP path's rounding points inside the recorded envelope; the stem plan
with its ``bfm`` step; the ``model/other/`` shim and ``cvit_prediction``'s
loader; the inference-only / no-CPU-fallback contract.
"""
import importlib
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import bfm_ref as R  # noqa: E402
from fac_fake_amd.weights import (BFM_NAMES, BFM_VARIANTS, CVIT_FAMILY, FAMILY_NAMES, OTHER_VARIANTS,  # noqa: E402
                                  bfm_param_specs, make_bfm_state_dict, make_crops, make_other_state_dict)
from oracle.cvit_torch import normalize_u8  # noqa: E402

REPO = Path(__file__).resolve().parents[1]
REFERENCE = Path(os.environ.get("FAC_REFERENCE_DIR", "/root/reference"))
ENVELOPE_MARGIN = 1.25            # drift of the CPU BLAS between hosts (conftest.ENVELOPE_MARGIN)
CROP_SEED = 41
NAME = "cvit_GGCA4_BFM5"
TFAM_KEYS = [f"bfm.tfam.{a}.{b}{i}.{p}" for a, b in (("channel_attention", "channel_conv"), ("spatial_attention", "spatial_conv"))
             for i in (1, 2) for p in ("weight", "bias")]


def _sd_t(name=NAME):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in make_bfm_state_dict(name, 0).items()}


def test_the_tables_agree_and_the_registry_is_untouched():
    assert BFM_NAMES == R.NAMES == (NAME,)
    v, (layers, g, bfm) = BFM_VARIANTS[NAME], R.TABLE[NAME]
    assert [tuple(l) for l in v["layers"]] == layers and v["ggca"] == g and v["bfm"] == bfm == ("stem", 512)
    base = OTHER_VARIANTS["cvit_GGCA4"]
    assert set(v) == set(base) | {"bfm"} and all(v[k] == base[k] for k in base)
    assert NAME not in CVIT_FAMILY and NAME not in FAMILY_NAMES and "bfm" not in base


def test_param_specs_are_the_reference_layout(golden):
    want = golden("bfm_keys.json")[NAME]
    got = [[n, list(s)] for n, s, _ in bfm_param_specs(NAME)]
    assert got == want and len(got) == R.N_KEYS[NAME] == 216
    names = [n for n, _ in got]
    first_bfm = names.index("bfm.multi_scale_extractor.conv1.weight")
    assert all(n.startswith("bfm.") for n in names[first_bfm:]) and len(names) - first_bfm == 14
    assert names[first_bfm - 1].startswith("ggca.") and names[-8:] == TFAM_KEYS


def test_synthetic_weights_are_deterministic_and_non_degenerate():
    a, b = make_bfm_state_dict(NAME, 0), make_bfm_state_dict(NAME, 0)
    assert list(a) == [n for n, _, _ in bfm_param_specs(NAME)]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    other = make_bfm_state_dict(NAME, 1)
    base = make_other_state_dict("cvit_GGCA4", 0)
    assert all(np.array_equal(a[k], base[k]) for k in base)          # the shared keys are cvit_GGCA4's draws
    for conv, k in (("conv1", 3), ("conv2", 5), ("conv3", 7)):
        w, bias = a[f"bfm.multi_scale_extractor.{conv}.weight"], a[f"bfm.multi_scale_extractor.{conv}.bias"]
        assert w.shape == (512, 512, k, k) and (w < 0).any() and (w > 0).any() and abs(float(w.mean())) < 0.01 * float(np.abs(w).mean())
        assert (bias < 0).any() and (bias > 0).any() and np.abs(bias).max() > 0.05
        assert not np.array_equal(w, other[f"bfm.multi_scale_extractor.{conv}.weight"])   # the seed matters
    for k in TFAM_KEYS:
        assert np.abs(a[k]).min() >= 0.1, k
    tf = np.concatenate([a[k].reshape(-1) for k in TFAM_KEYS])
    assert (tf < 0).any() and (tf > 0).any()


def _reference_bfm():
    """The reference file's own BFM class (the namespace its CViT was defined in)."""
    from tools.make_golden_bfm import load_reference_class
    return load_reference_class(REFERENCE, NAME).__init__.__globals__["BFM"]


def _have_reference() -> bool:
    try:
        return os.access(REFERENCE / "CViT-main" / "model" / "other" / f"{NAME}.py", os.R_OK)
    except OSError:
        return False


@pytest.mark.skipif(not _have_reference(), reason="needs the reference checkout")
@pytest.mark.parametrize("shape", [(2, 64, 7, 7), (2, 128, 9, 13), (1, 256, 14, 14), (1, 512, 7, 7)],
                         ids=lambda s: "x".join(map(str, s)))
def test_bfm_block_matches_the_reference_module_in_fp32(torch_threads, shape):
    """bfm_ref.bfm_block in fp32 against the reference's own BFM(C)(x, x) with
    the module's own (default-initialised) weights, TFAM included.  The bound
    is the module's own fp32-vs-float64 error at that shape, times 2."""
    BFM = _reference_bfm()
    n, c, h, w = shape
    torch.manual_seed(100 + c + h)
    mod = BFM(c).eval()
    x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(c * h + w)) * 1.5
    with torch.no_grad():
        want = mod(x, x)
        mod64 = BFM(c).double().eval()
        mod64.load_state_dict({k: v.double() for k, v in mod.state_dict().items()})
        want64 = mod64(x.double(), x.double())
        got = R.bfm_block(x, R.bfm_fold({f"bfm.{k}": v for k, v in mod.state_dict().items()}), 4.0, dtype=torch.float32)
    own = float((want.double() - want64).abs().max())
    d = float((got.double() - want.double()).abs().max())
    print(f"{shape}: max|bfm_block - BFM(x,x)| {d:.3e}; the module's own fp32 error {own:.3e} at values up to "
          f"{float(want.abs().max()):.2f}")
    assert own > 0 and d <= 2 * own, (shape, d, own)


@pytest.fixture(scope="module")
def crops_x():
    return normalize_u8(make_crops(4, seed=CROP_SEED))


def test_cpu_reference_matches_reference_goldens(golden, torch_threads, crops_x):
    g, env = golden("bfm_golden.npz"), golden("bfm_envelope.json")[NAME]
    assert int(g["crop_seed"]) == CROP_SEED
    sd = make_bfm_state_dict(NAME, 0)
    out, maps = R.forward_fp32(NAME, sd, crops_x, return_features=True)
    d = float(np.abs(out.numpy() - g[f"{NAME}/logits"]).max())
    print(f"forward_fp32 vs the golden logits: max|d| {d:.3e} (recorded {env['fp32']:.3e})")
    assert 0 < env["fp32"] and d <= 2 * env["fp32"]
    assert 0 <= env["tfam_sensitivity"] <= env["fp32"]               # fact 1, as the tool pinned it on the real module
    p = 1 / (1 + np.exp(-g[f"{NAME}/logits"]))
    assert p.min() >= 0.05 and p.max() <= 0.95                       # the fixture condition on the synthetic weights
    assert [tuple(maps[k].shape[1:]) for k in R.BFM_MAPS] == [(512, 7, 7), (512, 7, 7)]
    for k in R.BFM_MAPS:
        assert np.isclose(maps[k].double().sum().item(), float(g[f"{NAME}/{k}_sum"]), rtol=1e-6), k
        assert np.allclose(maps[k].numpy().reshape(-1)[::997], g[f"{NAME}/{k}_sample"], rtol=1e-5, atol=1e-5), k
    # the fixture conditions on the BFM weights, from the restatement
    f, ops = maps["pool5"], R.bfm_fold(sd)
    assert 0.25 <= float(maps["bfm"].norm() / f.norm()) <= 4
    assert R.bfm_mixed_sign(f, ops) >= 0.25


def test_emulation_stays_inside_the_recorded_envelope(golden, torch_threads, crops_x):
    """The HIP path's rounding points (emulated) against the fp32 reference's
    probabilities: the recorded envelope, which the GPU test doubles."""
    env = golden("bfm_envelope.json")[NAME]
    p_ref = torch.sigmoid(torch.from_numpy(golden("bfm_golden.npz")[f"{NAME}/logits"]))
    sd = make_bfm_state_dict(NAME, 0)
    _, maps = R.forward_fp32(NAME, sd, crops_x, return_features=True)
    ops = R.bfm_fold(sd)
    for dt in ("fp16", "bf16"):
        d = float((torch.sigmoid(R.forward_emulated(NAME, sd, crops_x, dtype=dt)) - p_ref).abs().max())
        print(f"{NAME} {dt}: emulated max|dp| {d:.3e}, recorded {env[dt]:.3e}")
        assert 0 < env[dt] and d <= ENVELOPE_MARGIN * env[dt], dt
        rnd = lambda t: R.round_to(t, dt)  # noqa: E731
        ops16 = {k: (v if k == "bias3" else rnd(v)) for k, v in ops.items()}
        f = rnd(maps["pool5"])
        ref = R.bfm_block(f, ops16)
        for route in ("fused", "composed"):
            e = R.bfm_block(f, ops16, dtype=torch.float32, round=dt, route=route).double() - ref
            rel, mx = float(e.norm() / ref.norm()), float(e.abs().max())
            rec = env["bfm_block"][route][dt]
            print(f"bfm_block {route} {dt}: rel L2 {rel:.3e} (recorded {rec['rel_l2']:.3e}), max|d| {mx:.3e} "
                  f"({rec['max_abs']:.3e})")
            assert 0 < rel <= ENVELOPE_MARGIN * rec["rel_l2"] and 0 < mx <= ENVELOPE_MARGIN * rec["max_abs"]
    from fac_fake_amd import bfm
    assert env["model_route"] == R.MODEL_ROUTE == bfm.MODEL_ROUTE      # the emulated forward rounds where the model does


def test_relu_before_the_sum_is_not_relu_of_the_sum():
    """The three convs do not merge into one 7x7 conv: on signed inputs the two forms differ by tens of percent."""
    g = torch.Generator().manual_seed(3)
    c = 64
    ops = {f"w{k}": (torch.rand(c, c, k, k, generator=g) * 2 - 1) * (3.0 / (c * k * k)) ** 0.5 for k in R.KS}
    ops["bias3"] = (torch.rand(3, c, generator=g) * 2 - 1) * 0.1
    x = torch.randn(2, c, 9, 13, generator=g)
    sep = R.bfm_block(x, ops, 1.0)
    merged = torch.relu(sum(R._pre(x, ops, torch.float64)))
    assert float((sep - merged).norm() / sep.norm()) > 0.2 and R.bfm_mixed_sign(x, ops) >= 0.5


def test_stem_plan_has_one_bfm_step_after_the_stem():
    from fac_fake_amd.variants import Step, stem_plan, steps_upto
    plan = stem_plan(BFM_VARIANTS[NAME])
    base = stem_plan(OTHER_VARIANTS["cvit_GGCA4"])
    S = Step
    want = [S("stem224", (3,), 224, 3, 32, True, True),
            S("conv", (4,), 112, 32, 64, False, True), S("conv", (5,), 112, 64, 64, False, True),
            S("conv", (6,), 112, 64, 64, True, True),
            S("conv", (7,), 56, 64, 128, False, True), S("conv", (8,), 56, 128, 128, False, True),
            S("conv", (9,), 56, 128, 128, True, True),
            S("conv", (10,), 28, 128, 256, False, True), S("conv", (11,), 28, 256, 256, False, True),
            S("conv", (12,), 28, 256, 256, False, True), S("conv", (13, "features1"), 28, 256, 256, True, True),
            S("ggca", ("ggca",), 14, 256, 256, op="att"),
            S("conv", (14,), 14, 256, 512, False, True), S("conv", (15,), 14, 512, 512, False, True),
            S("conv", (16,), 14, 512, 512, False, True), S("conv", (17,), 14, 512, 512, True, True),
            S("bfm", ("bfm",), 7, 512, 512)]
    assert plan == want and plan[:-1] == base
    assert steps_upto(plan, "bfm") == len(plan) == steps_upto(plan, None) and steps_upto(plan, 17) == len(plan) - 1
    assert steps_upto(plan, "ggca") == 12
    with pytest.raises(ValueError):
        steps_upto(base, "bfm")
    with pytest.raises(ValueError):
        steps_upto(plan, "smfa")
    # the cvit_BFM_MDFA spelling: the block after features1, on the 256-wide 14x14 map
    early = stem_plan(dict(BFM_VARIANTS[NAME], ggca=None, bfm=("features1", 256)))
    assert early[11] == S("bfm", ("bfm",), 14, 256, 256) and [s.kind for s in early].count("bfm") == 1


def test_bfm_fold_matches_the_cpu_reference_bitwise():
    from fac_fake_amd import bfm
    sd = _sd_t()
    got, want = bfm.bfm_fold(sd, "bfm"), R.bfm_fold(sd, "bfm")
    assert list(got) == list(want) == ["w3", "w5", "w7", "bias3"]
    for k in want:
        assert got[k].dtype == torch.float32 and torch.equal(got[k], want[k]), k
    assert got["bias3"].shape == (3, 512) and got["w7"].shape == (512, 512, 7, 7)
    assert bfm.BFM_SCALE == R.BFM_SCALE == 4.0


def test_dropin_state_dict_layout_and_contract(golden):
    from fac_fake_amd import bfm
    cls = bfm.bfm_class(NAME)
    m = cls(image_size=224, patch_size=7, num_classes=2, channels=512, dim=1024, depth=6, heads=8, mlp_dim=2048)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == golden("bfm_keys.json")[NAME]
    sd = _sd_t()
    m.load_state_dict(sd)
    back = m.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)       # the TFAM tensors included
    assert all(k in back and float(back[k].abs().min()) > 0 for k in TFAM_KEYS)
    assert not m.training and m.variant == NAME and m.table is BFM_VARIANTS[NAME]
    with pytest.raises(RuntimeError):
        m.train()
    with pytest.raises(RuntimeError):          # no CPU fallback
        m(torch.zeros(1, 3, 224, 224))
    with pytest.raises(RuntimeError):
        m.forward_u8(torch.zeros(1, 224, 224, 3, dtype=torch.uint8))
    with pytest.raises(NotImplementedError):   # only the reference's default configuration
        cls(depth=4)
    with pytest.raises(ValueError):
        cls(dtype="fp32")
    assert hasattr(m, "reserve") and hasattr(m, "_release")
    with pytest.raises(KeyError):
        bfm.bfm_class("cvit_GGCA4_MDFA5")
    with pytest.raises(KeyError):
        bfm.bfm_class("cvit_GGCA4")            # the other tables' classes are not BFM classes
    assert bfm.CViT(NAME).variant == NAME


def test_existing_tables_and_choices_are_untouched():
    import cvit_prediction as P
    from fac_fake_amd.weights import OTHER_NAMES, VARIANT_NAMES
    assert not set(BFM_NAMES) & (set(VARIANT_NAMES) | set(OTHER_NAMES) | set(P.MODEL_NAMES) | set(FAMILY_NAMES))
    assert len(FAMILY_NAMES) == 14


def test_gradcam_is_refused():
    from fac_fake_amd import bfm
    from fac_fake_amd.gradcam import GradCAM
    with pytest.raises(NotImplementedError):
        GradCAM(bfm.CViT(NAME))


def test_model_shim_and_prediction_loader():
    """`sys.path.insert(1, 'model/other'); from cvit_GGCA4_BFM5 import CViT`, and cvit_prediction's loader."""
    import cvit_prediction as P
    from fac_fake_amd import bfm
    sys.path.insert(1, str(REPO / "model" / "other"))
    try:
        mod = importlib.import_module(NAME)
    finally:
        sys.path.remove(str(REPO / "model" / "other"))
    assert mod.CViT is bfm.bfm_class(NAME)
    assert len(mod.CViT().state_dict()) == R.N_KEYS[NAME]
    assert P.model_class(NAME) is bfm.bfm_class(NAME)
    before = P.model
    try:
        m = P.load_model(name=NAME, dev="cpu")
    finally:
        P.model = before
    assert type(m) is bfm.bfm_class(NAME) and not m.training
    want = make_bfm_state_dict(NAME, 0)
    assert all(np.array_equal(v.numpy(), want[k]) for k, v in m.state_dict().items())
