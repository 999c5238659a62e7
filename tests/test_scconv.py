"""The ScConv block and cvit_GGCA_ADD_ScConv (fac_fake_amd/scconv.py), CPU side.

The CPU restatement of the block (tests/scconv_ref.py) against the reference's
own ``ScConv`` module's recorded outputs; the identity the kernel's softmax
rests on (the 2C channel means are linear in sums of the squeezed map); the
table and ``state_dict`` layout against the reference class's own keys
(tests/golden/scconv_keys.json, tools/make_golden_scconv.py); the stem plan; the
CPU reference of the class pinned to the reference's fp32 logits; its 16-bit
emulation of the HIP path's rounding points inside the recorded envelope; the
``model/other/`` shim and ``cvit_prediction``'s loader.
"""
import functools
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import scconv_ref as R  # noqa: E402
from fac_fake_amd.weights import (BFM_NAMES, BFM_VARIANTS, CVIT_FAMILY, FAMILY_NAMES, MDFA_NAMES, MDFA_VARIANTS,  # noqa: E402
                                  OTHER_VARIANTS, SCCONV_NAMES, SCCONV_VARIANTS, family_entry, make_crops,
                                  make_other_state_dict, make_scconv_state_dict, scconv_param_specs)
from oracle.cvit_torch import normalize_u8  # noqa: E402
from tools.make_golden_scconv import BLOCK_KINDS, BLOCK_SHAPES, N_CROPS, N_KEYS, SITES, block_case, block_key  # noqa: E402

REPO = Path(__file__).resolve().parents[1]
ENVELOPE_MARGIN = 1.25            # drift of the CPU BLAS between hosts (conftest.ENVELOPE_MARGIN)
CROP_SEED = 41
NAME = "cvit_GGCA_ADD_ScConv"
SIGMOID_HALF = 2.0 ** -22         # fp32 sigmoid(z) is exactly 0.5 for |z| below about 2^-23: the module's r > 0.5 is then false


def _sd_t():
    return {k: torch.from_numpy(np.asarray(v)) for k, v in make_scconv_state_dict(NAME, 0).items()}


# ---------------------------------------------------------------- the block
@pytest.mark.parametrize("kind", BLOCK_KINDS)
@pytest.mark.parametrize("shape", BLOCK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_block_matches_the_recorded_reference_module(golden, torch_threads, shape, kind):
    """scconv_block in float64 against the reference's own ScConv(c).eval()
    output, recorded in fp32, on every output outside the near-threshold band:
    |t| <= tau (8 x the error of fp32 F.group_norm, which the module runs) or |z| <= 2^-22, where the
    fp32 module's sigmoid is exactly 0.5 and its gate r > 0.5 stays shut for a
    positive z.  The bound is 1e-5 of the largest value: the tool measured 2e-8
    .. 2.2e-6 at values up to 9.6 between the module in fp32 and in float64."""
    want = torch.from_numpy(golden("scconv_block_golden.npz")[block_key(shape, kind)])
    sd, x = block_case(shape, kind)
    ops = R.scconv_fold(sd, "sc", None)
    assert tuple(want.shape) == shape and float(want.abs().max()) > 1e-3
    with torch.no_grad():
        tau, t64 = R.tau_of(x, ops, how="module")      # the module runs nn.GroupNorm
        got, parts = R.scconv_block(x, ops, torch.float64, parts=True, raw=True)
    z = t64 * ops["kc"].double().view(1, -1, 1, 1)
    near = R.near_mask(t64, tau) | (z.abs() <= SIGMOID_HALF)
    keep = ~R.excluded(near).unsqueeze(1).expand_as(got)
    share = float((z > 0).double().mean())
    d = float((got - want.double())[keep].abs().max())
    bound = 1e-5 * float(want.abs().max())
    print(f"{shape} {kind}: tau {tau:.3e}, {int(near.sum())} near elements, {1 - float(keep.double().mean()):.4f} excluded; gate "
          f"open on {share:.3f}; max|d| {d:.3e} (bound {bound:.3e})")
    assert 0.2 <= share <= 0.8 and float(keep.double().mean()) >= 0.95
    assert d <= bound, (shape, kind, d)


@pytest.mark.parametrize("shape", [(2, 64, 10, 14), (1, 128, 2, 2), (1, 64, 2, 7), (1, 256, 4, 18)], ids=lambda s: "x".join(map(str, s)))
def test_the_channel_means_are_linear_in_sums_of_u_and_l(shape):
    """mean(Y2) = [PWC2; I] mean(l), and mean(Y1) from the sum of u over the map,
    its first and last rows and columns and its four corners: what lets
    scconv.hip know s before any Y is formed.  Down to a 2x2 map, where every
    pixel is a corner."""
    n, c, h, w = shape
    sd, _ = block_case((1, c, 4, 4), "signed")
    ops = R.scconv_fold(sd, "sc", None, torch.float64)
    g = torch.Generator().manual_seed(9 + h * w)
    u, l = torch.randn(n, c // 4, h, w, generator=g, dtype=torch.float64), torch.randn(n, c // 4, h, w, generator=g, dtype=torch.float64)
    y1, y2 = R.transform(u, l, ops)
    direct = torch.cat([y1, y2], 1).mean((2, 3))
    lin = R.linear_means(u, l, ops)
    assert lin.shape == (n, 2 * c) and float((lin - direct).abs().max()) <= 1e-13 * max(1.0, float(direct.abs().max()))
    # and the borders matter: the means of a conv without padding effects (9 taps everywhere) differ
    assert float((direct[:, :c] - (ops["gwc_b"] + 0 * direct[:, :c])).abs().max()) > 1e-3


def test_the_gate_moves_half_of_x_between_the_halves():
    """At t -> 0+ the element keeps x[c] in channel c; at t -> 0- half of it stays
    and half arrives in the partner channel: the discontinuity the band is for."""
    c = 64
    ops = dict(gamma=torch.ones(c), beta=torch.zeros(c), kc=torch.full((c,), 1.0 / c))
    x = torch.zeros(1, c, 1, 1, dtype=torch.float64)
    x[0, 3] = 1.0
    for eps, own, partner in ((1e-9, 1.0, 0.0), (-1e-9, 0.5, 0.5)):
        t = torch.zeros(1, c, 1, 1, dtype=torch.float64)
        t[0, 3] = eps
        t[0, 35] = 1.0                           # the partner's own gate is open: it sends nothing back
        y = R.gate(x, t, ops)
        assert abs(float(y[0, 3]) - own) < 1e-8 and abs(float(y[0, 35]) - partner) < 1e-8


# ---------------------------------------------------------------- the table
def test_the_table_and_the_other_registries_are_untouched():
    import cvit_prediction as P
    assert SCCONV_NAMES == R.NAMES == (NAME,)
    v = SCCONV_VARIANTS[NAME]
    assert [tuple(l) for l in v["layers"]] == [tuple(l) for l in R.LAYERS]
    base = OTHER_VARIANTS["cvit_GGCA4"]["layers"]
    assert [l[:2] + l[5:] for l in v["layers"]] == [l[:2] + l[5:] for l in base]          # the plain (4, 1) stem's indices
    assert [i for i, l in enumerate(v["layers"]) if l[2] == "sc"] == list(R.SC_AT)
    assert [(l[0], l[1], l[3], l[4], l[5], l[7]) for l in v["layers"] if l[2] == "sc"] == [
        ("features1", 13, 64, 64, 14, False), ("features1", 23, 128, 128, 24, False), ("features1", 33, 256, 256, 34, False),
        ("features1", 39, 256, 256, 40, True)]
    assert v["ggca"] == R.GGCA and v["ff_norm"] == "layernorm" and not v["deconv"] and v["smfa"] is None
    assert family_entry(NAME) is v
    assert not set(SCCONV_NAMES) & (set(FAMILY_NAMES) | set(BFM_NAMES) | set(MDFA_NAMES) | set(CVIT_FAMILY) |
                                    set(BFM_VARIANTS) | set(MDFA_VARIANTS) | set(P.MODEL_NAMES))
    assert len(FAMILY_NAMES) == 14 and BFM_NAMES == ("cvit_GGCA4_BFM5",)
    assert MDFA_NAMES == ("cvit_GGCA4_MDFA5", "cvit_MDFA_BFM", "cvit_BFM_MDFA")
    with pytest.raises(KeyError):
        family_entry("cvit_ScConv")


def test_param_specs_are_the_reference_layout(golden):
    want = golden("scconv_keys.json")
    got = [[n, list(s)] for n, s, _ in scconv_param_specs(NAME)]
    assert got == want and len(got) == N_KEYS == 226
    shapes = dict((n, s) for n, s in got)
    for p, bn, c in SITES:
        names = [n for n, _ in got if n.startswith(p + ".")]
        assert names == [f"{p}.{k}" for k in ("SRU.gn.weight", "SRU.gn.bias", "CRU.squeeze1.weight", "CRU.squeeze2.weight",
                                               "CRU.GWC.weight", "CRU.GWC.bias", "CRU.PWC1.weight", "CRU.PWC2.weight")]
        assert shapes[f"{p}.CRU.GWC.weight"] == [c, c // 8, 3, 3] and shapes[f"{p}.CRU.PWC2.weight"] == [3 * c // 4, c // 4, 1, 1]
        assert shapes[f"{bn}.running_var"] == [c]
    assert [n for n, _ in got][-9:][0] == "ggca.shared_conv.0.weight"


def test_synthetic_draws():
    """The shared keys are the other tables' draws; gamma has both signs with
    |sum| >= C / 4, beta is non-zero, and the BatchNorms after the blocks are on
    the blocks' own output scale."""
    sd = make_scconv_state_dict(NAME, 0)
    base = make_other_state_dict("cvit_GGCA4", 0)
    shared = [k for k in base if k in sd and not k.startswith("ggca.") and not any(k.startswith(bn + ".") for _p, bn, _c in SITES)]
    assert len(shared) > 130 and all(np.array_equal(sd[k], base[k]) for k in shared)
    for p, bn, c in SITES:
        g, b = sd[p + ".SRU.gn.weight"], sd[p + ".SRU.gn.bias"]
        assert (g < 0).any() and (g > 0).any() and abs(float(g.sum())) >= c / 4 and float(np.abs(b).min()) >= 0.2
        assert float(sd[bn + ".running_var"].max()) < 1e-3
    assert not np.array_equal(sd["features1.13.CRU.GWC.weight"], make_scconv_state_dict(NAME, 1)["features1.13.CRU.GWC.weight"])


def test_stem_plan():
    from fac_fake_amd.variants import Step as S, stem_plan, steps_upto
    plan = stem_plan(SCCONV_VARIANTS[NAME])
    assert plan[0] == S("stem224", (3,), 224, 3, 32, True, True)
    sc = [s for s in plan if s.kind == "scconv"]
    assert sc == [S("scconv", (5,), 112, 64, 64, False, True), S("scconv", (8,), 56, 128, 128, False, True),
                  S("scconv", (11,), 28, 256, 256, False, True), S("scconv", (13, "features1"), 28, 256, 256, True, True)]
    assert plan[-1] == S("ggca", ("ggca",), 7, 512, 512, op="add")
    assert [s.kind for s in plan] == ["stem224", "conv", "scconv", "conv", "conv", "scconv", "conv", "conv", "scconv", "conv",
                                      "scconv"] + ["conv"] * 4 + ["ggca"]
    k = steps_upto(plan, "features1")
    assert plan[k - 1].kind == "scconv" and plan[k - 1].pool and steps_upto(plan, 13) == k and steps_upto(plan, None) == len(plan)
    with pytest.raises(ValueError):
        steps_upto(plan, "mdfa")
    # the other tables' plans have no scconv step
    assert not any(s.kind == "scconv" for e in list(CVIT_FAMILY.values()) + list(MDFA_VARIANTS.values()) for s in stem_plan(e))


# ---------------------------------------------------------------- the class
@functools.lru_cache(maxsize=None)
def _fp32():
    torch.set_num_threads(16)
    return R.forward_fp32(make_scconv_state_dict(NAME, 0), normalize_u8(make_crops(N_CROPS, seed=CROP_SEED)), return_features=True)


def test_cpu_reference_matches_reference_goldens(golden, torch_threads):
    """forward_fp32 against the reference class's logits: the restatement takes
    the gate as z > 0, the fp32 module as sigmoid(z) > 0.5, so a few elements
    within rounding of the threshold take the other side; the recorded distance
    holds that."""
    g, env = golden("scconv_golden.npz"), golden("scconv_envelope.json")
    assert int(g["crop_seed"]) == CROP_SEED and g["logits"].shape == (N_CROPS, 2)
    out, maps = _fp32()
    d = float(np.abs(out.numpy() - g["logits"]).max())
    print(f"forward_fp32 vs the golden logits: max|d| {d:.3e} (recorded {env['fp32']:.3e})")
    assert 0 < env["fp32"] < 1e-2 and d <= 2 * env["fp32"]
    assert g["probs"].min() >= 0.05 and g["probs"].max() <= 0.95          # the fixture condition on the synthetic weights
    sd = _sd_t()
    for p, bn, c in SITES:
        f, after = maps[p + "_in"], maps[p]
        assert np.isclose(f.double().sum().item(), float(g[f"{p}_in_sum"]), rtol=1e-4), p
        assert np.isclose(after.double().sum().item(), float(g[f"{p}_sum"]), rtol=1e-3), p
        ops = R.scconv_fold(sd, p, bn)
        _, parts = R.scconv_block(f, ops, torch.float64, parts=True)
        share = float((parts["t"] * ops["kc"].double().view(1, -1, 1, 1) > 0).double().mean())
        smax = float(parts["s"].max()) * 2 * c
        ratio = float(R.scconv_block(f, ops, torch.float32).norm() / f.norm())
        rec = env["blocks"][p]
        print(f"{p}: gate open on {share:.3f} (recorded {rec['gate_share']:.3f}), max s x 2C {smax:.2f}, ratio {ratio:.3f}")
        assert 0.2 <= share <= 0.8 and smax <= 10 and 0.25 <= ratio <= 4


def test_emulation_stays_inside_the_recorded_envelope(golden, torch_threads):
    """The HIP path's rounding points (emulated) against the reference class's
    fp32 probabilities over the 8 crops: the recorded envelope, which the GPU
    test doubles."""
    env = golden("scconv_envelope.json")
    p_ref = torch.from_numpy(golden("scconv_golden.npz")["probs"])
    sd = make_scconv_state_dict(NAME, 0)
    x = normalize_u8(make_crops(N_CROPS, seed=CROP_SEED))
    for dt in ("fp16", "bf16"):
        d = float((torch.sigmoid(R.forward_emulated(sd, x, dtype=dt)) - p_ref).abs().max())
        print(f"{dt}: emulated max|dp| {d:.3e}, recorded {env[dt]:.3e}")
        assert 0 < env[dt] and d <= ENVELOPE_MARGIN * env[dt], dt


def test_scconv_fold_matches_the_cpu_reference_bitwise():
    from fac_fake_amd import scconv
    sd = _sd_t()
    for p, bn, c in SITES:
        got, want = scconv.scconv_fold(sd, p, bn), R.scconv_fold(sd, p, bn)
        assert list(got) == list(want) and tuple(got) == scconv.PACK_ORDER == R.PACK_ORDER
        for k in want:
            assert got[k].dtype == torch.float32 and torch.equal(got[k], want[k]), k
        assert got["gwc_w"].shape == (c, c // 8, 3, 3) and got["pwc2"].shape == (3 * c // 4, c // 4)
        assert abs(float(got["kc"].sum()) - 1) < 1e-5
    bare = scconv.scconv_fold(sd, "features1.13")
    assert torch.equal(bare["scale"], torch.ones(64)) and torch.equal(bare["shift"], torch.zeros(64))
    bad = dict(sd)
    bad["features1.13.CRU.PWC1.weight"] = bad["features1.13.CRU.PWC1.weight"][:, :8]
    with pytest.raises(ValueError):
        scconv.scconv_fold(bad, "features1.13", "features1.14")


def test_dropin_state_dict_layout_and_contract(golden):
    from fac_fake_amd import mdfa, scconv
    cls = scconv.scconv_class(NAME)
    m = cls(image_size=224, patch_size=7, num_classes=2, channels=512, dim=1024, depth=6, heads=8, mlp_dim=2048)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == golden("scconv_keys.json")
    sd = _sd_t()
    m.load_state_dict(sd)
    back = m.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    assert not m.training and m.variant == NAME and m.table is SCCONV_VARIANTS[NAME]
    kinds = [l[0] for l in m.folded_layers()]
    assert kinds.count("sc") == 4 and kinds.count("conv") == 13
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
    assert hasattr(m, "reserve") and m._scconv_scratch is None
    with pytest.raises(KeyError):
        scconv.scconv_class("cvit_GGCA4_MDFA5")     # the other tables' classes are not ScConv classes
    with pytest.raises(KeyError):
        mdfa.mdfa_class(NAME)
    assert scconv.CViT(NAME).variant == NAME


def test_a_zero_or_non_finite_gamma_sum_is_refused():
    """The block divides by sum(gamma): load_state_dict raises and leaves the weights as they were."""
    from fac_fake_amd import scconv
    m = scconv.CViT(NAME)
    sd = _sd_t()
    m.load_state_dict(sd)
    for value in (0.0, float("nan"), float("inf")):
        bad = dict(sd)
        g = torch.ones(128)
        g[::2] = -1.0
        if value != 0.0:
            g[0] = value
        bad["features1.23.SRU.gn.weight"] = g
        with pytest.raises(ValueError):
            m.load_state_dict(bad)
        assert torch.equal(m.state_dict()["features1.23.SRU.gn.weight"], sd["features1.23.SRU.gn.weight"])
    with pytest.raises(ValueError):
        R.scconv_fold({**sd, "features1.23.SRU.gn.weight": torch.zeros(128)}, "features1.23", "features1.24")


def test_gradcam_is_refused():
    from fac_fake_amd import scconv
    from fac_fake_amd.gradcam import GradCAM
    with pytest.raises(NotImplementedError):
        GradCAM(scconv.CViT(NAME))


def test_model_shim_and_prediction_loader():
    """`sys.path.insert(1, 'model/other'); from cvit_GGCA_ADD_ScConv import CViT`, and cvit_prediction's loader."""
    import cvit_prediction as P
    from fac_fake_amd import scconv
    sys.path.insert(1, str(REPO / "model" / "other"))
    try:
        mod = importlib.import_module(NAME)
    finally:
        sys.path.remove(str(REPO / "model" / "other"))
    assert mod.CViT is scconv.scconv_class(NAME)
    assert P.model_class(NAME) is scconv.scconv_class(NAME) and NAME not in P.MODEL_NAMES
    before = P.model
    try:
        m = P.load_model(name=NAME, dev="cpu")
    finally:
        P.model = before
    assert type(m) is scconv.scconv_class(NAME) and not m.training and len(m.state_dict()) == N_KEYS
    want = make_scconv_state_dict(NAME, 0)
    assert all(np.array_equal(v.numpy(), want[k]) for k, v in m.state_dict().items())
