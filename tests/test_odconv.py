"""The ODConv2d block and the two ODConv CViT classes (fac_fake_amd/odconv.py), CPU side.

The CPU restatement of the block (tests/odconv_ref.py) against the reference's
own ``ODConv2d`` module's recorded outputs and attentions; the table and
``state_dict`` layout against the reference classes' own keys
(tests/golden/odconv_keys.json, tools/make_golden_odconv.py); the stem plans; the
host fold; the CPU references of the classes pinned to the reference's fp32
logits; their 16-bit emulation of the HIP path's rounding points inside the
recorded envelope; the ``model/other/`` shims and ``cvit_prediction``'s loader.
"""
import functools
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import odconv_ref as R  # noqa: E402
from fac_fake_amd.weights import (BFM_NAMES, BFM_VARIANTS, CVIT_FAMILY, FAMILY_NAMES, MDFA_NAMES, MDFA_VARIANTS,  # noqa: E402
                                  ODCONV_NAMES, ODCONV_VARIANTS, OTHER_VARIANTS, SCCONV_NAMES, SCCONV_VARIANTS, family_entry,
                                  make_crops, make_odconv_state_dict, make_other_state_dict, odconv_param_specs)
from oracle.cvit_torch import BN_EPS, normalize_u8  # noqa: E402
from tools.make_golden_odconv import BLOCK_KINDS, BLOCK_SHAPES, N_CROPS, N_KEYS, block_case, block_key  # noqa: E402

REPO = Path(__file__).resolve().parents[1]
ENVELOPE_MARGIN = 1.25            # drift of the CPU BLAS between hosts (conftest.ENVELOPE_MARGIN)
CROP_SEED = 41
ADD, BARE = R.NAMES
OD_KEYS = ("weight", "attention.fc.weight", "attention.bn.weight", "attention.bn.bias", "attention.bn.running_mean",
           "attention.bn.running_var", "attention.bn.num_batches_tracked", "attention.channel_fc.weight",
           "attention.channel_fc.bias", "attention.filter_fc.weight", "attention.filter_fc.bias", "attention.spatial_fc.weight",
           "attention.spatial_fc.bias", "attention.kernel_fc.weight", "attention.kernel_fc.bias")


@functools.lru_cache(maxsize=None)
def _sd_t(name):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in make_odconv_state_dict(name, 0).items()}


# ---------------------------------------------------------------- the block
@pytest.mark.parametrize("kind", BLOCK_KINDS)
@pytest.mark.parametrize("shape", BLOCK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_block_matches_the_recorded_reference_module(golden, torch_threads, shape, kind):
    """odconv_block in float64 against the reference's own ODConv2d(c, c, 3,
    padding=1).eval() output and its attention(x), both recorded in fp32.  The
    bounds are fp32 accuracy: 1e-5 of the largest output (the tool measured 2.5e-6
    .. 4.2e-6 at values up to 11.7 between the module in fp32 and in float64)
    and 2e-6 for the attentions, which lie in (0, 1)."""
    g = golden("odconv_block_golden.npz")
    want, want_att = torch.from_numpy(g[block_key(shape, kind)]), torch.from_numpy(g[block_key(shape, kind) + "/att"])
    sd, x = block_case(shape, kind)
    n, c = shape[:2]
    ops = R.odconv_fold(sd, "od", None)
    assert tuple(want.shape) == shape and tuple(want_att.shape) == (n, 2 * c + 13) and float(want.abs().max()) > 1e-1
    with torch.no_grad():
        got, att = R.odconv_block(x, ops, torch.float64, parts=True, raw=True)
    d, da = float((got - want.double()).abs().max()), float((R.att_row(att) - want_att.double()).abs().max())
    print(f"{shape} {kind}: max|d| {d:.3e} (bound {1e-5 * float(want.abs().max()):.3e}), attentions {da:.3e}")
    assert d <= 1e-5 * float(want.abs().max()) and da <= 2e-6
    # the attentions are not trivial: ca spreads, ka is neither uniform nor one-hot
    assert float(att["ca"].max() - att["ca"].min()) > 0.3 and 0.3 < float(att["ka"].max()) < 0.95
    if n > 1:                      # and they differ per crop
        assert float((att["ca"][0] - att["ca"][1]).abs().max()) > 0.05


def test_the_aggregated_weight_is_the_formula():
    """aggregate() against four nested loops on a tiny case, and the block as a per-crop plain conv."""
    g = torch.Generator().manual_seed(3)
    B, C = 2, 4
    ops = dict(weight=torch.randn(4, C, C, 3, 3, generator=g, dtype=torch.float64))
    ca, sa = torch.rand(B, C, generator=g, dtype=torch.float64), torch.rand(B, 9, generator=g, dtype=torch.float64)
    ka = torch.softmax(torch.randn(B, 4, generator=g, dtype=torch.float64), 1)
    w = R.aggregate(ops, ca, sa, ka)
    for b in range(B):
        for o in range(C):
            for i in range(C):
                for t in range(9):
                    want = sum(ka[b, k] * ops["weight"][k, o, i, t // 3, t % 3] for k in range(4)) * sa[b, t] * ca[b, i]
                    assert abs(float(w[b, o, i, t // 3, t % 3] - want)) < 1e-14


# ---------------------------------------------------------------- the table
def test_the_tables_and_the_other_registries_are_untouched():
    import cvit_prediction as P
    assert ODCONV_NAMES == R.NAMES == ("cvit_GGCA_ADD_ODConv", "cvit_GGCA_ODConv")
    a, b = ODCONV_VARIANTS[ADD], ODCONV_VARIANTS[BARE]
    for name in R.NAMES:
        assert [tuple(l) for l in ODCONV_VARIANTS[name]["layers"]] == [tuple(l) for l in R.LAYERS[name]]
        assert ODCONV_VARIANTS[name]["ggca"] == R.GGCA[name] and family_entry(name) is ODCONV_VARIANTS[name]
        assert ODCONV_VARIANTS[name]["ff_norm"] == "layernorm" and not ODCONV_VARIANTS[name]["deconv"]
    base = OTHER_VARIANTS["cvit_GGCA4"]["layers"]
    assert [l[:2] + l[5:] for l in a["layers"]] == [l[:2] + l[5:] for l in base]          # the plain (4, 1) stem's indices
    assert [tuple(l) for l in b["layers"]] == [tuple(l) for l in base]
    assert [i for i, l in enumerate(a["layers"]) if l[2] == "od"] == list(R.OD_AT)
    assert [(l[0], l[1], l[3], l[4], l[5], l[6], l[7]) for l in a["layers"] if l[2] == "od"] == [
        ("features1", 13, 64, 64, 14, True, False), ("features1", 23, 128, 128, 24, True, False),
        ("features1", 33, 256, 256, 34, True, False), ("features1", 39, 256, 256, 40, True, True)]
    assert a["odconv_unused"] == 256 and a.get("odconv") is None
    assert b["odconv"] == ("features1", 256) and b.get("odconv_unused") is None
    others = (set(FAMILY_NAMES) | set(BFM_NAMES) | set(MDFA_NAMES) | set(SCCONV_NAMES) | set(CVIT_FAMILY) | set(BFM_VARIANTS) |
              set(MDFA_VARIANTS) | set(SCCONV_VARIANTS) | set(P.MODEL_NAMES))
    assert not set(ODCONV_NAMES) & others
    assert len(FAMILY_NAMES) == 14 and BFM_NAMES == ("cvit_GGCA4_BFM5",) and SCCONV_NAMES == ("cvit_GGCA_ADD_ScConv",)
    assert MDFA_NAMES == ("cvit_GGCA4_MDFA5", "cvit_MDFA_BFM", "cvit_BFM_MDFA")
    with pytest.raises(KeyError):
        family_entry("cvit_ODConv")


@pytest.mark.parametrize("name", R.NAMES)
def test_param_specs_are_the_reference_layout(golden, name):
    want = golden("odconv_keys.json")[name]
    got = [[n, list(s)] for n, s, _ in odconv_param_specs(name)]
    assert got == want and len(got) == N_KEYS[name] == {ADD: 269, BARE: 217}[name]
    shapes = dict((n, s) for n, s in got)
    blocks = [(p, c) for p, _bn, c, _h, _pool in R.SITES[name]] + ([("odconv", 256)] if name == ADD else [])
    for p, c in blocks:
        assert [n for n, _ in got if n.startswith(p + ".")] == [f"{p}.{k}" for k in OD_KEYS]
        assert shapes[f"{p}.weight"] == [4, c, c, 3, 3] and shapes[f"{p}.attention.fc.weight"] == [16, c, 1, 1]
        assert shapes[f"{p}.attention.spatial_fc.weight"] == [9, 16, 1, 1] and shapes[f"{p}.attention.kernel_fc.bias"] == [4]
    assert [n for n, _ in got][-15] == "odconv.weight" and [n for n, _ in got][-24] == "ggca.shared_conv.0.weight"


def test_synthetic_draws():
    """The shared keys are the other tables' draws; the four W_k differ; the head
    biases take both signs; the attention's BatchNorm is on the scale of fc p."""
    from fac_fake_amd import weights as W
    sd, bare = make_odconv_state_dict(ADD, 0), make_odconv_state_dict(BARE, 0)
    base = make_other_state_dict("cvit_GGCA4", 0)
    own = [q + "." for p, bn, *_ in R.SITES[ADD] for q in (p, bn)]          # the blocks and the BatchNorms after them
    shared = [k for k in base if k in sd and not k.startswith("ggca.") and not any(k.startswith(q) for q in own)]
    assert len(shared) > 130 and all(np.array_equal(sd[k], base[k]) for k in shared)
    assert all(np.array_equal(bare[k], base[k]) for k in base if not k.startswith("ggca."))
    assert all(np.array_equal(sd[k], bare[k]) for k in bare if k.startswith("odconv."))      # same key, same draw
    for p in [s[0] for s in R.SITES[ADD]] + ["odconv"]:
        w = sd[p + ".weight"]
        assert all(not np.array_equal(w[0], w[k]) for k in (1, 2, 3))
        for head in ("channel", "filter", "spatial", "kernel"):
            b = sd[f"{p}.attention.{head}_fc.bias"]
            assert (b < 0).any() and (b > 0).any()
        assert abs(float(sd[p + ".attention.bn.running_var"].mean()) / W.ODCONV_FC_STD[p] ** 2 - 1) < 0.2
    assert not np.array_equal(sd["features1.13.weight"], make_odconv_state_dict(ADD, 1)["features1.13.weight"])


def test_stem_plans():
    from fac_fake_amd.variants import Step as S, stem_plan, steps_upto
    plan = stem_plan(ODCONV_VARIANTS[ADD])
    assert plan[0] == S("stem224", (3,), 224, 3, 32, True, True)
    assert [s for s in plan if s.kind == "odconv"] == [
        S("odconv", (5,), 112, 64, 64, False, True), S("odconv", (8,), 56, 128, 128, False, True),
        S("odconv", (11,), 28, 256, 256, False, True), S("odconv", (13, "features1"), 28, 256, 256, True, True)]
    assert plan[-1] == S("ggca", ("ggca",), 7, 512, 512, op="add")
    assert [s.kind for s in plan] == ["stem224", "conv", "odconv", "conv", "conv", "odconv", "conv", "conv", "odconv", "conv",
                                      "odconv"] + ["conv"] * 4 + ["ggca"]
    k = steps_upto(plan, "features1")
    assert plan[k - 1].kind == "odconv" and plan[k - 1].pool and steps_upto(plan, 13) == k
    with pytest.raises(ValueError):
        steps_upto(plan, "odconv")                  # the class never calls its top-level odconv
    plan = stem_plan(ODCONV_VARIANTS[BARE])
    assert [s.kind for s in plan] == ["stem224"] + ["conv"] * 10 + ["odconv"] + ["conv"] * 4 + ["ggca"]
    k = steps_upto(plan, "odconv")
    assert plan[k - 1] == S("odconv", ("odconv",), 14, 256, 256, False, False) and k == steps_upto(plan, "features1") + 1
    assert plan[k - 2].pool and plan[k - 2].relu and plan[k] == S("conv", (14,), 14, 256, 512, False, True)
    assert plan[-1] == S("ggca", ("ggca",), 7, 512, 512, op="att")
    # the other tables' plans have no odconv step
    others = list(CVIT_FAMILY.values()) + list(MDFA_VARIANTS.values()) + list(SCCONV_VARIANTS.values()) + list(BFM_VARIANTS.values())
    assert not any(s.kind == "odconv" for e in others for s in stem_plan(e))


# ---------------------------------------------------------------- the fold
def test_odconv_fold_matches_a_hand_fold_bitwise():
    from fac_fake_amd import odconv
    sd = _sd_t(ADD)
    for p, bn, c, _h, _pool in R.SITES[ADD]:
        got, want = odconv.odconv_fold(sd, p, bn), R.odconv_fold(sd, p, bn)
        assert list(got) == list(want) and tuple(got) == odconv.PACK_ORDER == R.PACK_ORDER
        for k in want:
            assert got[k].dtype == torch.float32 and got[k].is_contiguous() and torch.equal(got[k], want[k]), k
        a = p + ".attention.bn."
        s = sd[a + "weight"] / torch.sqrt(sd[a + "running_var"] + torch.tensor(BN_EPS, dtype=torch.float32))
        assert torch.equal(got["bn_scale"], s) and torch.equal(got["bn_shift"], sd[a + "bias"] - sd[a + "running_mean"] * s)
        q = bn + "."
        s = sd[q + "weight"] / torch.sqrt(sd[q + "running_var"] + torch.tensor(BN_EPS, dtype=torch.float32))
        assert torch.equal(got["scale"], s) and torch.equal(got["shift"], sd[q + "bias"] - sd[q + "running_mean"] * s)
        assert torch.equal(got["weight"], sd[p + ".weight"]) and got["fc"].shape == (16, c) and got["channel_fc"].shape == (c, 16)
        assert torch.equal(got["kernel_fc"], sd[p + ".attention.kernel_fc.weight"].reshape(4, 16))
    bare = odconv.odconv_fold(_sd_t(BARE), "odconv")
    assert torch.equal(bare["scale"], torch.ones(256)) and torch.equal(bare["shift"], torch.zeros(256))


def test_odconv_fold_refuses_bad_shapes():
    from fac_fake_amd import odconv
    sd = _sd_t(ADD)
    p = "features1.13"
    for key, bad in ((p + ".weight", sd[p + ".weight"][:3]),                                    # kernel_num 3
                     (p + ".weight", sd[p + ".weight"][:, :, :, :, :2]),                         # 3x2 taps
                     (p + ".attention.fc.weight", sd[p + ".attention.fc.weight"][:8]),           # attention width 8
                     (p + ".attention.channel_fc.weight", sd[p + ".attention.channel_fc.weight"][:32]),
                     (p + ".attention.spatial_fc.bias", sd[p + ".attention.spatial_fc.bias"][:4]),
                     ("features1.14.weight", sd["features1.14.weight"][:32])):
        with pytest.raises(ValueError):
            odconv.odconv_fold({**sd, key: bad}, p, "features1.14")
    with pytest.raises(ValueError):
        R.odconv_fold({**sd, p + ".weight": sd[p + ".weight"][:1]}, p, "features1.14")


# ---------------------------------------------------------------- the classes
@functools.lru_cache(maxsize=None)
def _fp32(name):
    torch.set_num_threads(16)
    return R.forward_fp32(name, make_odconv_state_dict(name, 0), normalize_u8(make_crops(N_CROPS, seed=CROP_SEED)),
                          return_features=True)


@pytest.mark.parametrize("name", R.NAMES)
def test_cpu_reference_matches_reference_goldens(golden, torch_threads, name):
    """forward_fp32 against the reference class's recorded fp32 logits, and each
    ODConv site's input and output map against their recorded sums; the
    fixture conditions on the synthetic weights hold on the restatement too."""
    g, env = golden("odconv_golden.npz"), golden("odconv_envelope.json")[name]
    assert int(g["crop_seed"]) == CROP_SEED and g[name + "/logits"].shape == (N_CROPS, 2)
    out, maps = _fp32(name)
    d = float(np.abs(out.numpy() - g[name + "/logits"]).max())
    print(f"{name}: forward_fp32 vs the golden logits: max|d| {d:.3e} (recorded {env['fp32']:.3e})")
    assert d <= max(2 * env["fp32"], 2e-5)
    assert g[name + "/probs"].min() >= 0.05 and g[name + "/probs"].max() <= 0.95
    sd = _sd_t(name)
    for p, bn, c, H, pool in R.SITES[name]:
        f, after = maps[p + "_in"], maps[p]
        assert tuple(f.shape[1:]) == (c, H, H) and tuple(after.shape[1:]) == ((c, H // 2, H // 2) if pool else (c, H, H))
        assert np.isclose(f.double().sum().item(), float(g[f"{name}/{p}_in_sum"]), rtol=1e-4), p
        assert np.isclose(after.double().sum().item(), float(g[f"{name}/{p}_sum"]), rtol=1e-3, atol=1.0), p
        assert np.allclose(after.numpy().reshape(-1)[::997], g[f"{name}/{p}_sample"], rtol=1e-3, atol=1e-4), p
        _, att = R.odconv_block(f, R.odconv_fold(sd, p, bn), torch.float64, parts=True, raw=True)
        rec = env["blocks"][p]
        assert float(att["ka"].max()) <= 0.9 and float(att["ka"].max(0).values.min()) >= 0.05
        assert abs(float(att["ka"].max()) - rec["ka_max"]) < 1e-3
        for a in (att["ca"], att["fa"]):
            assert float(torch.quantile(a.flatten(), 0.05)) <= 0.25 and float(torch.quantile(a.flatten(), 0.95)) >= 0.75
        assert float(att["sa"].min()) < 0.4 and float(att["sa"].max()) > 0.6 and 0.25 <= rec["ratio"] <= 4
    if name == BARE:               # the bare block's output is signed and feeds features2.0 as it is
        assert float((maps["odconv"] < 0).float().mean()) > 0.2


@pytest.mark.parametrize("name", R.NAMES)
def test_emulation_stays_inside_the_recorded_envelope(golden, torch_threads, name):
    """The HIP path's rounding points (emulated) against the reference class's
    fp32 probabilities over the 8 crops: the recorded envelope, which the GPU
    test doubles."""
    env = golden("odconv_envelope.json")[name]
    p_ref = torch.from_numpy(golden("odconv_golden.npz")[name + "/probs"])
    sd = make_odconv_state_dict(name, 0)
    x = normalize_u8(make_crops(N_CROPS, seed=CROP_SEED))
    for dt in ("fp16", "bf16"):
        d = float((torch.sigmoid(R.forward_emulated(name, sd, x, dtype=dt)) - p_ref).abs().max())
        print(f"{name} {dt}: emulated max|dp| {d:.3e}, recorded {env[dt]:.3e}")
        assert 0 < env[dt] and d <= ENVELOPE_MARGIN * env[dt], dt


@pytest.mark.parametrize("name", R.NAMES)
def test_dropin_state_dict_layout_and_contract(golden, name):
    from fac_fake_amd import odconv, scconv
    cls = odconv.odconv_class(name)
    m = cls(image_size=224, patch_size=7, num_classes=2, channels=512, dim=1024, depth=6, heads=8, mlp_dim=2048)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == golden("odconv_keys.json")[name]
    sd = _sd_t(name)
    m.load_state_dict(sd)
    back = m.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    assert sum(k.startswith("odconv.") for k in back) == 15          # kept, called (cvit_GGCA_ODConv) or not
    assert not m.training and m.variant == name and m.table is ODCONV_VARIANTS[name]
    folded = m.folded_layers()
    assert len(folded) == 17
    if name == ADD:
        kinds = [l[0] for l in folded]
        assert kinds.count("od") == 4 and kinds.count("conv") == 13
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
    assert hasattr(m, "reserve") and m._odconv_scratch is None
    with pytest.raises(KeyError):
        odconv.odconv_class("cvit_GGCA_ADD_ScConv")     # the other tables' classes are not ODConv classes
    with pytest.raises(KeyError):
        scconv.scconv_class(name)
    assert odconv.CViT(name).variant == name and odconv.CViT().variant == ADD


def test_gradcam_is_refused():
    from fac_fake_amd import odconv
    from fac_fake_amd.gradcam import GradCAM
    for name in R.NAMES:
        with pytest.raises(NotImplementedError):
            GradCAM(odconv.CViT(name))


@pytest.mark.parametrize("name", R.NAMES)
def test_model_shim_and_prediction_loader(name):
    """`sys.path.insert(1, 'model/other'); from <name> import CViT`, and cvit_prediction's loader."""
    import cvit_prediction as P
    from fac_fake_amd import odconv
    sys.path.insert(1, str(REPO / "model" / "other"))
    try:
        mod = importlib.import_module(name)
    finally:
        sys.path.remove(str(REPO / "model" / "other"))
    assert mod.CViT is odconv.odconv_class(name)
    assert P.model_class(name) is odconv.odconv_class(name) and name not in P.MODEL_NAMES
    before = P.model
    try:
        m = P.load_model(name=name, dev="cpu")
    finally:
        P.model = before
    assert type(m) is odconv.odconv_class(name) and not m.training and len(m.state_dict()) == N_KEYS[name]
    want = make_odconv_state_dict(name, 0)
    assert all(np.array_equal(v.numpy(), want[k]) for k, v in m.state_dict().items())
