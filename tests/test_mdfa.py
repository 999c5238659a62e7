"""The MDFA block and the three MDFA CViT classes (fac_fake_amd/mdfa.py), CPU side.

The CPU restatement of the block (tests/mdfa_ref.py) against the reference's
own ``MDFA`` module's recorded outputs; the three identities the kernel rests
on (hebing collapses to one scalar per pixel, most dilated taps never touch
the map, branch 5 is a per-crop constant), each on its own; the tables and
``state_dict`` layouts against the reference classes' own keys
(tests/golden/mdfa_keys.json, tools/make_golden_mdfa.py); each class's stem
plan; the CPU reference of each class pinned to the reference's fp32 logits;
its 16-bit emulation of the HIP path's rounding points inside the recorded
envelope; the ``model/other/`` shims and ``cvit_prediction``'s loader.
"""
import functools
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))

import mdfa_ref as R  # noqa: E402
from fac_fake_amd.weights import (BFM_NAMES, BFM_VARIANTS, CVIT_FAMILY, FAMILY_NAMES, MDFA_NAMES, MDFA_VARIANTS,  # noqa: E402
                                  OTHER_VARIANTS, family_entry, make_bfm_state_dict, make_crops, make_mdfa_state_dict,
                                  make_other_state_dict, mdfa_param_specs)
from oracle.cvit_torch import normalize_u8  # noqa: E402
from tools.make_golden_mdfa import MODULE_SHAPES, N_KEYS, module_case, module_key  # noqa: E402

REPO = Path(__file__).resolve().parents[1]
ENVELOPE_MARGIN = 1.25            # drift of the CPU BLAS between hosts (conftest.ENVELOPE_MARGIN)
CROP_SEED = 41
GGCA4, BOTH, SWAPPED = "cvit_GGCA4_MDFA5", "cvit_MDFA_BFM", "cvit_BFM_MDFA"


def _sd_t(name):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in make_mdfa_state_dict(name, 0).items()}


def _random_case(shape, seed=5):
    """Signed input and folded operands with both gates in play, float64-ready."""
    n, c, h, w = shape
    sd, _ = module_case(shape)
    x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(seed + c)) * 1.5
    return x, R.mdfa_fold(sd)


# ---------------------------------------------------------------- the block
@pytest.mark.parametrize("shape", MODULE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mdfa_block_matches_the_recorded_reference_module(golden, torch_threads, shape):
    """mdfa_block (the kernel's form) and mdfa_module (the reference's form)
    against the reference's own MDFA(c, c).eval() output, recorded in fp32 with
    randomised BatchNorm statistics.  The bound is 1e-5 of the largest value:
    the tool measured 9e-7 .. 2.5e-6 at values up to 1.7 for the fp32 forms."""
    want = torch.from_numpy(golden("mdfa_golden.npz")[module_key(shape)])
    sd, x = module_case(shape)
    ops = R.mdfa_fold(sd)
    assert tuple(want.shape) == shape and float(want.abs().max()) > 0.5
    bound = 1e-5 * float(want.abs().max())
    with torch.no_grad():
        for dtype in (torch.float32, torch.float64):
            for fn in (R.mdfa_block, R.mdfa_module):
                d = float((fn(x, ops, dtype).double() - want.double()).abs().max())
                print(f"{shape} {fn.__name__} {dtype}: max|d| {d:.3e} (bound {bound:.3e})")
                assert d <= bound, (fn.__name__, dtype, d)


@pytest.mark.parametrize("shape", [(2, 64, 7, 7), (1, 128, 9, 13), (1, 64, 14, 14)], ids=lambda s: "x".join(map(str, s)))
def test_hebing_collapses_to_one_scalar_per_pixel(shape):
    """cat >= 0, so max(cat t_b, cat s_p) = cat max(t_b, s_p) bit for bit, in
    fp32 and float64, with both sides of the max occurring."""
    x, ops = _random_case(shape)
    for dtype in (torch.float32, torch.float64):
        cat4 = R.branches(x, ops, dtype)
        g = R.branch5(x, ops, dtype)
        cat = torch.cat([cat4, g.view(*g.shape, 1, 1).expand(-1, -1, *cat4.shape[2:])], 1)
        s, t = R.gates(cat4, g, ops, dtype)
        t = torch.full_like(t, float(s.median()))            # a channel gate inside the pixel gate's spread
        assert float(cat.min()) >= 0 and 0.2 <= float((t.view(-1, 1, 1) > s).double().mean()) <= 0.8
        two = torch.max(cat * t.view(-1, 1, 1, 1), cat * s.unsqueeze(1))
        one = cat * torch.maximum(t.view(-1, 1, 1), s).unsqueeze(1)
        assert torch.equal(two, one)
        # larry * cat = m_p cat^2: the same products in another association, a rounding or two apart
        m = torch.maximum(t.view(-1, 1, 1), s).unsqueeze(1)
        assert torch.allclose(two * cat, m * (cat * cat), rtol=4 * torch.finfo(dtype).eps, atol=0)


def test_dropped_tap_table():
    """The taps of the 28 that touch the map at all, and the in-map count per pixel."""
    count = lambda h, w: len(R.kept_taps(h, w))  # noqa: E731
    assert count(14, 14) == 1 + 9 + 9 + 1 == 20
    assert count(7, 7) == 1 + 9 + 1 + 1 == 12
    assert count(9, 13) == 1 + 9 + 3 + 1 == 14
    per_branch = lambda h, w: [sum(1 for b, _, _ in R.kept_taps(h, w) if b == i) for i in (1, 2, 3, 4)]  # noqa: E731
    assert per_branch(14, 14) == [1, 9, 9, 1] and per_branch(7, 7) == [1, 9, 1, 1] and per_branch(9, 13) == [1, 9, 3, 1]
    assert (3, 0, 1) in R.kept_taps(9, 13) and (3, 1, 0) not in R.kept_taps(9, 13)      # d = 12 along w only
    assert count(13, 13) == 20 and count(12, 12) == 12                                   # the threshold is |d| < size
    avg = 1 + sum(float(R.in_map_taps(14, 14, d).mean()) for d in R.DILATIONS)
    assert abs(avg - 8.2) < 0.1, avg                                                      # about 8.2 C x C products per pixel
    v6 = R.in_map_taps(7, 7, 6)
    assert v6[0, 0] == 4 and v6[0, 3] == 2 and v6[3, 3] == 1 and int(v6.sum()) == 4 * 4 + 20 * 2 + 25


@pytest.mark.parametrize("shape", [(2, 64, 14, 14), (2, 64, 7, 7), (1, 128, 9, 13)], ids=lambda s: "x".join(map(str, s)))
def test_dropped_taps_contribute_nothing(shape):
    """The convs with the dropped taps' weights zeroed equal the full dilated convs."""
    x, ops = _random_case(shape)
    full, kept = R.branches(x, ops, torch.float64), R.branches(x, ops, torch.float64, drop=True)
    assert float((full - kept).abs().max()) <= 1e-13 * float(full.abs().max())
    # and a kept tap is not droppable: zeroing one changes the result
    ops2 = dict(ops, w2=ops["w2"].clone())
    ops2["w2"][:, :, 0, 0] = 0
    assert float((R.branches(x, ops2, torch.float64) - full).abs().max()) > 1e-3


def test_branch5_is_a_per_crop_constant():
    """The bilinear upsample of a 1x1 map with align_corners is a constant map,
    so branch 5's share of conv_cat is the vector e_b and its shares of the two
    dots are scalars: mdfa_block equals mdfa_module."""
    x, ops = _random_case((2, 64, 9, 13))
    g = R.branch5(x, ops, torch.float64)
    up = F.interpolate(g.view(2, 64, 1, 1), (9, 13), None, "bilinear", True)
    assert torch.equal(up, g.view(2, 64, 1, 1).expand(2, 64, 9, 13))
    a, b = R.mdfa_block(x, ops), R.mdfa_module(x, ops)
    assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())
    # a second crop does not change the first: the constant is per crop (the CPU's sums may reorder with the batch)
    assert float((R.mdfa_block(x[:1], ops) - a[:1]).abs().max()) <= 1e-12 * float(b.abs().max())


def test_fp16_square_is_clamped():
    """cat above 255.9 would square to inf in fp16: the emulation clamps q to 65504 as the kernel does."""
    x, ops = _random_case((1, 64, 7, 7))
    ops = R.round_ops(ops, "fp16")
    out = R.mdfa_block(R.round_to(x * 400, "fp16"), ops, torch.float32, round="fp16", parts=True)
    assert float(out[1]["cat4"].max()) > 256
    assert not torch.isnan(out[0]).any()


# ---------------------------------------------------------------- the tables
def test_the_tables_agree_and_the_other_registries_are_untouched():
    import cvit_prediction as P
    assert MDFA_NAMES == R.NAMES == (GGCA4, BOTH, SWAPPED)
    base = OTHER_VARIANTS["cvit_GGCA4"]
    for name in MDFA_NAMES:
        v, (layers, g, mdfa, bfm, unused) = MDFA_VARIANTS[name], R.TABLE[name]
        assert [tuple(l) for l in v["layers"]] == layers == [tuple(l) for l in base["layers"]]
        assert v["ggca"] == g and v["mdfa"] == mdfa and v.get("bfm") == bfm and v.get("ggca_unused") == unused
        assert v["ff_norm"] == "layernorm" and not v["deconv"] and v["smfa"] is None
        assert family_entry(name) is v
    assert MDFA_VARIANTS[SWAPPED]["bfm"] == ("features1", 256) and MDFA_VARIANTS[SWAPPED]["mdfa"] == ("stem", 512)
    assert not set(MDFA_NAMES) & (set(FAMILY_NAMES) | set(BFM_NAMES) | set(CVIT_FAMILY) | set(BFM_VARIANTS) | set(P.MODEL_NAMES))
    assert len(FAMILY_NAMES) == 14 and BFM_NAMES == ("cvit_GGCA4_BFM5",)
    with pytest.raises(KeyError):
        family_entry("cvit_MDFA")


@pytest.mark.parametrize("name", R.NAMES)
def test_param_specs_are_the_reference_layout(golden, name):
    want = golden("mdfa_keys.json")[name]
    got = [[n, list(s)] for n, s, _ in mdfa_param_specs(name)]
    assert got == want and len(got) == N_KEYS[name]
    names = [n for n, _ in got]
    first = {p: min(i for i, n in enumerate(names) if n.startswith(p + ".")) for p in ("ggca", "mdfa")}
    assert names[first["ggca"] - 1] == "mlp_head.2.bias" and first["ggca"] < first["mdfa"]      # ggca, mdfa, bfm
    assert sum(n.startswith("mdfa.") for n in names) == 44 and sum(n.startswith("ggca.") for n in names) == 9
    if name != GGCA4:
        fb = names.index("bfm.multi_scale_extractor.conv1.weight")
        assert fb == first["mdfa"] + 44 and all(n.startswith("bfm.") for n in names[fb:]) and len(names) - fb == 14
    c = MDFA_VARIANTS[name]["mdfa"][1]
    shapes = dict((n, s) for n, s in got)
    assert shapes["mdfa.conv_cat.0.weight"] == [c, 5 * c, 1, 1] and shapes["mdfa.branch4.0.weight"] == [c, c, 3, 3]
    assert shapes["mdfa.Hebing.tongdao.fc.weight"] == shapes["mdfa.Hebing.kongjian.Conv1x1.weight"] == [1, 5 * c, 1, 1]


def test_synthetic_draws_are_keyed_per_tensor():
    """The shared keys are the other tables' draws, so no existing checksum moves."""
    a = make_mdfa_state_dict(GGCA4, 0)
    base = make_other_state_dict("cvit_GGCA4", 0)
    shared = [k for k in base if not k.startswith("ggca.")]          # GGCA(512,7,7) here, GGCA(256,14,14) there
    assert len(shared) > 150 and all(np.array_equal(a[k], base[k]) for k in shared)
    b, bfm5 = make_mdfa_state_dict(BOTH, 0), make_bfm_state_dict("cvit_GGCA4_BFM5", 0)
    assert all(np.array_equal(b[k], bfm5[k]) for k in bfm5)          # features, tail, GGCA(256), BFM(512)
    assert all(np.array_equal(a[k], b[k]) for k in a if k.startswith("mdfa."))
    sw = make_mdfa_state_dict(SWAPPED, 0)
    assert sw["mdfa.branch2.0.weight"].shape == (512, 512, 3, 3) and sw["bfm.multi_scale_extractor.conv3.weight"].shape == (256, 256, 7, 7)
    wt, ws = a["mdfa.Hebing.tongdao.fc.weight"], a["mdfa.Hebing.kongjian.Conv1x1.weight"]
    assert wt.min() >= 0 and wt.max() > 0 and (ws < 0).any() and (ws > 0).any()
    assert not np.array_equal(a["mdfa.branch3.0.weight"], make_mdfa_state_dict(GGCA4, 1)["mdfa.branch3.0.weight"])


def test_stem_plans():
    from fac_fake_amd.variants import Step as S, stem_plan, steps_upto
    base = stem_plan(OTHER_VARIANTS["cvit_GGCA4"])
    convs = [s for s in base if s.kind != "ggca"]
    f1 = next(i for i, s in enumerate(convs) if "features1" in s.labels) + 1
    want = {
        GGCA4: convs[:f1] + [S("mdfa", ("mdfa",), 14, 256, 256)] + convs[f1:] + [S("ggca", ("ggca",), 7, 512, 512, op="att")],
        BOTH: convs[:f1] + [S("mdfa", ("mdfa",), 14, 256, 256)] + convs[f1:] + [S("bfm", ("bfm",), 7, 512, 512)],
        SWAPPED: convs[:f1] + [S("bfm", ("bfm",), 14, 256, 256)] + convs[f1:] + [S("mdfa", ("mdfa",), 7, 512, 512)],
    }
    for name in R.NAMES:
        plan = stem_plan(MDFA_VARIANTS[name])
        assert plan == want[name], name
        assert [s.kind for s in plan].count("mdfa") == 1 and len(plan) == len(base) + 1
        k = steps_upto(plan, "mdfa")
        assert plan[k - 1].kind == "mdfa" and k == (f1 + 1 if name != SWAPPED else len(plan))
        assert steps_upto(plan, "features1") == f1 and steps_upto(plan, None) == len(plan)
        with pytest.raises(ValueError):
            steps_upto(plan, "smfa")
    with pytest.raises(ValueError):
        steps_upto(base, "mdfa")
    with pytest.raises(ValueError):
        steps_upto(stem_plan(MDFA_VARIANTS[BOTH]), "ggca")             # its ggca is never called


# ---------------------------------------------------------------- the classes
@pytest.fixture(scope="module")
def crops_x():
    return normalize_u8(make_crops(4, seed=CROP_SEED))


@functools.lru_cache(maxsize=None)
def _fp32(name):
    """forward_fp32 of one class on the golden crops, computed once for the two tests that need it."""
    torch.set_num_threads(16)
    return R.forward_fp32(name, make_mdfa_state_dict(name, 0), normalize_u8(make_crops(4, seed=CROP_SEED)),
                          return_features=True)


@pytest.mark.parametrize("name", R.NAMES)
def test_cpu_reference_matches_reference_goldens(golden, torch_threads, crops_x, name):
    g, env = golden("mdfa_golden.npz"), golden("mdfa_envelope.json")[name]
    assert int(g["crop_seed"]) == CROP_SEED
    sd = make_mdfa_state_dict(name, 0)
    out, maps = _fp32(name)
    d = float(np.abs(out.numpy() - g[f"{name}/logits"]).max())
    print(f"{name}: forward_fp32 vs the golden logits: max|d| {d:.3e} (recorded {env['fp32']:.3e})")
    assert 0 < env["fp32"] and d <= 2 * env["fp32"]
    p = 1 / (1 + np.exp(-g[f"{name}/logits"]))
    assert p.min() >= 0.05 and p.max() <= 0.95                       # the fixture condition on the synthetic weights
    c, hw = MDFA_VARIANTS[name]["mdfa"][1], 14 if MDFA_VARIANTS[name]["mdfa"][0] == "features1" else 7
    for k in ("mdfa_in", "mdfa"):
        assert tuple(maps[k].shape[1:]) == (c, hw, hw)
        assert np.isclose(maps[k].double().sum().item(), float(g[f"{name}/{k}_sum"]), rtol=1e-5), k
        assert np.allclose(maps[k].numpy().reshape(-1)[::997], g[f"{name}/{k}_sample"], rtol=1e-4, atol=1e-4), k
    # the fixture conditions on the MDFA weights, from the restatement
    f, ops = maps["mdfa_in"], R.mdfa_fold(sd)
    _, parts = R.mdfa_block(f, ops, parts=True)
    share = float((parts["t"].view(-1, 1, 1) > parts["s"]).double().mean())
    print(f"{name}: t wins on {share:.3f} (recorded {env['t_share']:.3f}), ratio {float(maps['mdfa'].norm() / f.norm()):.3f}, "
          f"max cat {float(parts['cat4'].max()):.2f}")
    assert 0.2 <= share <= 0.8 and 0.2 <= env["t_share"] <= 0.8
    assert 0.25 <= float(maps["mdfa"].norm() / f.norm()) <= 4
    assert float(max(parts["cat4"].max(), parts["g"].max())) <= 64 and env["max_cat"] <= 64
    assert 0.02 < float(parts["s"].min()) and float(parts["s"].max()) < 0.98          # the pixel gate is not saturated


@pytest.mark.parametrize("name", R.NAMES)
def test_emulation_stays_inside_the_recorded_envelope(golden, torch_threads, crops_x, name):
    """The HIP path's rounding points (emulated) against the fp32 reference's
    probabilities: the recorded envelope, which the GPU test doubles."""
    env = golden("mdfa_envelope.json")[name]
    p_ref = torch.sigmoid(torch.from_numpy(golden("mdfa_golden.npz")[f"{name}/logits"]))
    sd = make_mdfa_state_dict(name, 0)
    _, maps = _fp32(name)
    ops = R.mdfa_fold(sd)
    for dt in ("fp16", "bf16"):
        d = float((torch.sigmoid(R.forward_emulated(name, sd, crops_x, dtype=dt)) - p_ref).abs().max())
        print(f"{name} {dt}: emulated max|dp| {d:.3e}, recorded {env[dt]:.3e}")
        assert 0 < env[dt] and d <= ENVELOPE_MARGIN * env[dt], dt
        f, ops16 = R.round_to(maps["mdfa_in"], dt), R.round_ops(ops, dt)
        e = R.mdfa_block(f, ops16, torch.float32, round=dt).double() - R.mdfa_block(f, ops16)
        rel, mx = float(e.norm() / R.mdfa_block(f, ops16).norm()), float(e.abs().max())
        rec = env["mdfa_block"][dt]
        print(f"mdfa_block {dt}: rel L2 {rel:.3e} (recorded {rec['rel_l2']:.3e}), max|d| {mx:.3e} ({rec['max_abs']:.3e})")
        assert 0 < rel <= ENVELOPE_MARGIN * rec["rel_l2"] and 0 < mx <= ENVELOPE_MARGIN * rec["max_abs"]


def test_mdfa_fold_matches_the_cpu_reference_bitwise():
    from fac_fake_amd import mdfa
    for name in (GGCA4, SWAPPED):
        sd = _sd_t(name)
        got, want = mdfa.mdfa_fold(sd, "mdfa"), R.mdfa_fold(sd, "mdfa")
        assert list(got) == list(want) and set(got) == set(mdfa.PACK_ORDER)
        for k in want:
            assert got[k].dtype == torch.float32 and torch.equal(got[k], want[k]), k
        c = MDFA_VARIANTS[name]["mdfa"][1]
        assert got["wcat"].shape == (c, 5 * c) and got["w3"].shape == (c, c, 3, 3) and got["bias4"].shape == (4, c)
    with pytest.raises(ValueError):
        bad = dict(sd)
        bad["mdfa.branch5_conv.weight"] = bad["mdfa.branch5_conv.weight"][:, :8]
        mdfa.mdfa_fold(bad)


@pytest.mark.parametrize("name", R.NAMES)
def test_dropin_state_dict_layout_and_contract(golden, name):
    from fac_fake_amd import bfm, mdfa
    cls = mdfa.mdfa_class(name)
    m = cls(image_size=224, patch_size=7, num_classes=2, channels=512, dim=1024, depth=6, heads=8, mlp_dim=2048)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == golden("mdfa_keys.json")[name]
    sd = _sd_t(name)
    m.load_state_dict(sd)
    back = m.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)       # the unused ggca included
    assert not m.training and m.variant == name and m.table is MDFA_VARIANTS[name]
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
    assert hasattr(m, "reserve") and m._mdfa_scratch is None
    with pytest.raises(KeyError):
        mdfa.mdfa_class("cvit_GGCA4_BFM5")     # the other tables' classes are not MDFA classes
    with pytest.raises(KeyError):
        bfm.bfm_class(name)
    assert mdfa.CViT(name).variant == name


def test_gradcam_is_refused():
    from fac_fake_amd import mdfa
    from fac_fake_amd.gradcam import GradCAM
    with pytest.raises(NotImplementedError):
        GradCAM(mdfa.CViT(GGCA4))


@pytest.mark.parametrize("name", R.NAMES)
def test_model_shim_and_prediction_loader(name):
    """`sys.path.insert(1, 'model/other'); from <name> import CViT`, and cvit_prediction's loader."""
    import cvit_prediction as P
    from fac_fake_amd import mdfa
    sys.path.insert(1, str(REPO / "model" / "other"))
    try:
        mod = importlib.import_module(name)
    finally:
        sys.path.remove(str(REPO / "model" / "other"))
    assert mod.CViT is mdfa.mdfa_class(name)
    assert P.model_class(name) is mdfa.mdfa_class(name)
    before = P.model
    try:
        m = P.load_model(name=name, dev="cpu")
    finally:
        P.model = before
    assert type(m) is mdfa.mdfa_class(name) and not m.training and len(m.state_dict()) == N_KEYS[name]
    want = make_mdfa_state_dict(name, 0)
    assert all(np.array_equal(v.numpy(), want[k]) for k, v in m.state_dict().items())
