"""The WTConv2d block and cvit_GGCA_ADD_WTConv (fac_fake_amd/wtconv.py), CPU side.

The CPU restatements of the block (tests/wtconv_ref.py) against the reference's
own ``WTConv2d`` module's recorded outputs and against each other; the table
and ``state_dict`` layout against the reference class's own keys
(tests/golden/wtconv_keys.json, tools/make_golden_wtconv.py); the stem plan;
the host fold and packing; the CPU reference of the class pinned to the
reference's fp32 logits; its 16-bit emulation of the HIP path's rounding points
inside the recorded envelope; the ``model/other/`` shim and
``cvit_prediction``'s loader.
"""
import functools
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import wtconv_ref as R  # noqa: E402
from fac_fake_amd import weights as W  # noqa: E402
from fac_fake_amd.weights import (WTCONV_KINDS, WTCONV_NAMES, WTCONV_VARIANTS, db1_filters, family_entry, make_crops,  # noqa: E402
                                  make_family_state_dict, make_wtconv_state_dict, wtconv_param_specs)
from oracle.cvit_torch import BN_EPS, normalize_u8  # noqa: E402
from tools.make_golden_wtconv import BLOCK_KINDS, BLOCK_SHAPES, N_CROPS, N_KEYS, block_case, block_key, pywt_stand_in  # noqa: E402

REPO = Path(__file__).resolve().parents[1]
ENVELOPE_MARGIN = 1.25            # drift of the CPU BLAS between hosts (conftest.ENVELOPE_MARGIN)
CROP_SEED = 41
NAME = R.NAME


@functools.lru_cache(maxsize=None)
def _sd_t():
    return {k: torch.from_numpy(np.asarray(v)) for k, v in make_wtconv_state_dict(NAME, 0).items()}


# ---------------------------------------------------------------- the block
@pytest.mark.parametrize("kind", BLOCK_KINDS)
@pytest.mark.parametrize("shape", BLOCK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wt_reference_matches_the_recorded_reference_module(golden, torch_threads, shape, kind):
    """wt_reference in fp32 against the reference's own WTConv2d(c).eval() output, recorded in fp32: 1e-5 of the
    largest output (the tool measured 3.7e-7 .. 7.9e-7 between the module in fp32 and in float64)."""
    want = torch.from_numpy(golden("wtconv_block_golden.npz")[block_key(shape, kind)])
    sd, x = block_case(shape, kind)
    assert tuple(want.shape) == shape and float(want.abs().max()) > 1.0
    with torch.no_grad():
        got = R.wt_reference(x, sd, "wt", torch.float32)
    d = float((got - want).abs().max())
    print(f"{shape} {kind}: max|d| {d:.3e} (bound {1e-5 * float(want.abs().max()):.3e})")
    assert d <= 1e-5 * float(want.abs().max())


@pytest.mark.parametrize("kind", BLOCK_KINDS)
@pytest.mark.parametrize("shape", BLOCK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wt_layer_is_wt_reference_in_float64(torch_threads, shape, kind):
    """The kernel's arithmetic (folded scales, general 2x2 filters, shifted sums) against the reference's op
    sequence, both in float64: 1e-12 of the largest output; and both paths are there."""
    sd, x = block_case(shape, kind)
    with torch.no_grad():
        want = R.wt_reference(x, sd, "wt", torch.float64)
        ops = R.wt_fold(sd, "wt", None, torch.float64)
        got = R.wt_layer(x, ops, False, torch.float64, relu=False)
        u, b = R.wt_layer(x, ops, dtype=torch.float64, parts=True)
        u_ref, b_ref = R.wt_reference(x, sd, "wt", torch.float64, parts=True)
    top = float(want.abs().max())
    assert float((got - want).abs().max()) <= 1e-12 * top
    assert float((u - u_ref).abs().max()) <= 1e-12 * top
    bias = (ops["shift"]).view(1, -1, 1, 1)                     # q None: shift = base_scale * bias
    assert float((b + bias - b_ref).abs().max()) <= 1e-12 * top
    assert 0.1 < float(u.norm() / b.norm()) < 10
    # pooled and with ReLU: the pool of the unpooled layer
    full = R.wt_layer(x, ops, False, torch.float64)
    assert torch.equal(R.wt_layer(x, ops, True, torch.float64), torch.nn.functional.max_pool2d(full, 2, 2)) and float(full.min()) == 0


def test_general_filters_are_used_not_haar():
    """wt_layer with random 2x2 filters against the op sequence with the same filters."""
    sd, x = block_case((2, 32, 10, 14), "signed")
    g = torch.Generator().manual_seed(5)
    sd = {**sd, "wt.wt_filter": torch.randn(128, 1, 2, 2, generator=g), "wt.iwt_filter": torch.randn(128, 1, 2, 2, generator=g)}
    with torch.no_grad():
        want = R.wt_reference(x, sd, "wt", torch.float64)
        got = R.wt_layer(x, R.wt_fold(sd, "wt", None, torch.float64), False, torch.float64, relu=False)
        haar = R.wt_reference(x, block_case((2, 32, 10, 14), "signed")[0], "wt", torch.float64)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert float((want - haar).abs().max()) > 0.1


def test_db1_filters_and_the_stand_in():
    """The generator's filters are the ones the reference's create_wavelet_filter builds from PyWavelets' db1
    values (restated here with torch as the reference does, through the tool's stand-in), bit for bit; they are
    +-0.5 up to fp32 rounding, and synthesis inverts analysis."""
    mod, _ = pywt_stand_in()
    w = mod.Wavelet("db1")
    r = 2.0 ** -0.5
    assert (w.dec_lo, w.dec_hi, w.rec_lo, w.rec_hi) == ([r, r], [-r, r], [r, r], [r, -r])
    with pytest.raises(ValueError):
        mod.Wavelet("db2")
    dec_hi, dec_lo = torch.tensor(w.dec_hi[::-1], dtype=torch.float), torch.tensor(w.dec_lo[::-1], dtype=torch.float)
    rec_hi, rec_lo = torch.tensor(w.rec_hi[::-1], dtype=torch.float).flip(0), torch.tensor(w.rec_lo[::-1], dtype=torch.float).flip(0)
    outer = lambda a, b: a.unsqueeze(0) * b.unsqueeze(1)  # noqa: E731
    dec = torch.stack([outer(dec_lo, dec_lo), outer(dec_lo, dec_hi), outer(dec_hi, dec_lo), outer(dec_hi, dec_hi)])
    rec = torch.stack([outer(rec_lo, rec_lo), outer(rec_lo, rec_hi), outer(rec_hi, rec_lo), outer(rec_hi, rec_hi)])
    d, i = db1_filters(3)
    assert d.shape == (12, 1, 2, 2) and d.dtype == np.float32
    for ch in range(3):
        assert np.array_equal(d[4 * ch:4 * ch + 4, 0], dec.numpy()) and np.array_equal(i[4 * ch:4 * ch + 4, 0], rec.numpy())
    assert np.abs(np.abs(d) - 0.5).max() < 1e-7 and (d[0] > 0).all() and (d[3, 0] * d[0, 0] < 0).sum() == 2
    x = torch.randn(1, 3, 4, 6, dtype=torch.float64)
    s = torch.nn.functional.conv2d(x, torch.from_numpy(d).double(), stride=2, groups=3)
    back = torch.nn.functional.conv_transpose2d(s, torch.from_numpy(i).double(), stride=2, groups=3)
    assert float((back - x).abs().max()) < 1e-6


# ---------------------------------------------------------------- the table
def test_the_table_and_the_other_registries_are_untouched():
    import cvit_prediction as P
    assert WTCONV_NAMES == (NAME,) == ("cvit_GGCA_ADD_WTConv",) and WTCONV_KINDS == R.WTCONV_KINDS
    e = WTCONV_VARIANTS[NAME]
    assert [tuple(l) for l in e["layers"]] == [tuple(l) for l in R.LAYERS] and family_entry(NAME) is e
    assert e["ggca"] == R.GGCA and e["ff_norm"] == "layernorm" and not e["deconv"] and e["smfa"] is None
    base = W.VARIANTS["cvit_GGCA_ADD"]["layers"]                  # the base CViT's one Sequential
    assert [l[:2] + l[5:] for l in e["layers"]] == [l[:2] + l[5:] for l in base]
    assert [i for i, l in enumerate(e["layers"]) if l[2] == "wt"] == list(R.WT_AT) == [1, 2, 4, 5, 7, 8, 10, 11, 12]
    assert [(p, q, c, h, pool) for p, q, c, h, pool in R.SITES] == [
        ("features.3", "features.4", 32, 224, False), ("features.6", "features.7", 32, 224, True),
        ("features.13", "features.14", 64, 112, False), ("features.16", "features.17", 64, 112, True),
        ("features.23", "features.24", 128, 56, False), ("features.26", "features.27", 128, 56, True),
        ("features.33", "features.34", 256, 28, False), ("features.36", "features.37", 256, 28, False),
        ("features.39", "features.40", 256, 28, True)]
    others = (set(W.FAMILY_NAMES) | set(W.BFM_NAMES) | set(W.MDFA_NAMES) | set(W.SCCONV_NAMES) | set(W.ODCONV_NAMES) |
              set(P.MODEL_NAMES))
    assert NAME not in others and len(W.FAMILY_NAMES) == 14
    with pytest.raises(KeyError):
        family_entry("cvit_WTConv")


def test_param_specs_are_the_reference_layout(golden):
    want = golden("wtconv_keys.json")
    got = [[n, list(s)] for n, s, _ in wtconv_param_specs(NAME)]
    assert got == want and len(got) == N_KEYS == 247
    assert [[k, list(v.shape)] for k, v in make_wtconv_state_dict(NAME, 0).items()] == want
    shapes = dict((n, s) for n, s in got)
    for p, _q, c, _h, _pool in R.SITES:
        assert [n for n, _ in got if n.startswith(p + ".")] == [f"{p}.{k}" for k in R.WT_KEYS]
        assert shapes[f"{p}.wt_filter"] == [4 * c, 1, 2, 2] and shapes[f"{p}.wavelet_convs.0.weight"] == [4 * c, 1, 5, 5]
        assert shapes[f"{p}.wavelet_scale.0.weight"] == [1, 4 * c, 1, 1] and shapes[f"{p}.base_scale.weight"] == [1, c, 1, 1]


def test_synthetic_draws():
    """The shared keys are the base table's draws; the filters are db1's; taps and scales take both signs, the
    scales around the reference's 1 and 0.1; the BatchNorms after WT layers are on the calibrated scale."""
    sd = make_wtconv_state_dict(NAME, 0)
    base = make_family_state_dict("cvit_GGCA_ADD", 0)
    own = [q + "." for p, bn, *_ in R.SITES for q in (p, bn)]
    shared = [k for k in base if k in sd and not k.startswith("ggca.") and not any(k.startswith(q) for q in own)]
    assert len(shared) > 120 and all(np.array_equal(sd[k], base[k]) for k in shared)
    for p, bn, c, _h, _pool in R.SITES:
        d, i = db1_filters(c)
        assert np.array_equal(sd[p + ".wt_filter"], d) and np.array_equal(sd[p + ".iwt_filter"], i)
        for leaf in ("base_conv.weight", "wavelet_convs.0.weight"):
            assert (sd[f"{p}.{leaf}"] < 0).mean() > 0.3 and (sd[f"{p}.{leaf}"] > 0).mean() > 0.3
        bs, ws = sd[p + ".base_scale.weight"], sd[p + ".wavelet_scale.0.weight"]
        assert 0.05 < (bs < 0).mean() < 0.5 and 0.1 < (ws < 0).mean() < 0.4
        assert 0.5 <= np.abs(bs).min() and np.abs(bs).max() <= 1.5 and 0.05 <= np.abs(ws).min() and np.abs(ws).max() <= 0.15
        assert abs(float(sd[bn + ".running_var"].mean()) / W.WTCONV_OUT_STD[bn] ** 2 - 1) < 0.1
    assert not np.array_equal(sd["features.3.base_conv.weight"], make_wtconv_state_dict(NAME, 1)["features.3.base_conv.weight"])


def test_stem_plan():
    from fac_fake_amd.variants import Step as S, stem_plan, steps_upto
    plan = stem_plan(WTCONV_VARIANTS[NAME])
    assert plan[0] == S("pack32", (), 224, 3, 32)
    kinds = {"c": "conv", "w": "wt"}
    assert [s.kind for s in plan[1:-1]] == [kinds[k] for k in WTCONV_KINDS.replace(" ", "")]
    assert plan[1] == S("conv", (1,), 224, 32, 32, False, True) and plan[-1] == S("ggca", ("ggca",), 7, 512, 512, op="add")
    assert [s for s in plan if s.kind == "wt"] == [
        S("wt", (2,), 224, 32, 32, False, True), S("wt", (3,), 224, 32, 32, True, True),
        S("wt", (5,), 112, 64, 64, False, True), S("wt", (6,), 112, 64, 64, True, True),
        S("wt", (8,), 56, 128, 128, False, True), S("wt", (9,), 56, 128, 128, True, True),
        S("wt", (11,), 28, 256, 256, False, True), S("wt", (12,), 28, 256, 256, False, True),
        S("wt", (13,), 28, 256, 256, True, True)]
    assert steps_upto(plan, 3) == 4 and steps_upto(plan, "features1") == len(plan) - 1
    others = (list(W.CVIT_FAMILY.values()) + list(W.MDFA_VARIANTS.values()) + list(W.SCCONV_VARIANTS.values()) +
              list(W.BFM_VARIANTS.values()) + list(W.ODCONV_VARIANTS.values()))
    assert not any(s.kind == "wt" for e in others for s in stem_plan(e))


# ---------------------------------------------------------------- the fold
def test_wt_fold_matches_a_hand_fold_bitwise_and_packs():
    from fac_fake_amd import wtconv
    sd = _sd_t()
    for p, bn, c, _h, _pool in R.SITES[::4]:
        got, want = wtconv.wt_fold(sd, p, bn), R.wt_fold(sd, p, bn)
        assert tuple(got) == wtconv.PACK_ORDER == R.PACK_ORDER
        for k in want:
            assert got[k].dtype == torch.float32 and got[k].is_contiguous() and torch.equal(got[k], want[k]), k
        s = sd[bn + ".weight"] / torch.sqrt(sd[bn + ".running_var"] + torch.tensor(BN_EPS, dtype=torch.float32))
        bs = sd[p + ".base_scale.weight"].reshape(c)
        assert torch.equal(got["scale"], s)
        assert torch.equal(got["shift"], sd[bn + ".bias"] - sd[bn + ".running_mean"] * s + bs * sd[p + ".base_conv.bias"] * s)
        assert torch.equal(got["wtaps"][5, 2], sd[p + ".wavelet_convs.0.weight"][22].reshape(25) * sd[p + ".wavelet_scale.0.weight"][0, 22, 0, 0])
        assert torch.equal(got["btaps"][7], sd[p + ".base_conv.weight"][7].reshape(25) * bs[7])
        assert torch.equal(got["dwt"], sd[p + ".wt_filter"].reshape(c, 4, 2, 2))
        packed = wtconv.wt_pack(got, "cpu")
        assert [tuple(t.shape) for t in packed] == [(c // 4, 4, 4, 4), (c // 4, 4, 25, 4), (c // 4, 4, 4, 4), (c // 4, 25, 4), (c,), (c,)]
        assert all(t.is_contiguous() and t.dtype == torch.float32 for t in packed)
        ch, k, i, j, t = 13, 2, 1, 0, 17
        assert packed[0][ch // 4, k, i * 2 + j, ch % 4] == got["dwt"][ch, k, i, j]
        assert packed[2][ch // 4, k, i * 2 + j, ch % 4] == got["iwt"][ch, k, i, j]
        assert packed[1][ch // 4, k, t, ch % 4] == got["wtaps"][ch, k, t] and packed[3][ch // 4, t, ch % 4] == got["btaps"][ch, t]
    bare = wtconv.wt_fold(sd, "features.3")
    assert torch.equal(bare["scale"], torch.ones(32))
    assert torch.equal(bare["shift"], sd["features.3.base_scale.weight"].reshape(32) * sd["features.3.base_conv.bias"])


def test_wt_fold_refuses_bad_shapes_and_deeper_levels():
    from fac_fake_amd import wtconv
    sd = _sd_t()
    p = "features.13"
    for key, bad in ((p + ".wt_filter", sd[p + ".wt_filter"][:64]), (p + ".base_conv.weight", sd[p + ".base_conv.weight"][:, :, :3, :3]),
                     (p + ".wavelet_convs.0.weight", sd[p + ".wavelet_convs.0.weight"][:64]),
                     (p + ".wavelet_scale.0.weight", sd[p + ".wavelet_scale.0.weight"][:, :64]),
                     ("features.14.weight", sd["features.14.weight"][:32])):
        with pytest.raises(ValueError):
            wtconv.wt_fold({**sd, key: bad}, p, "features.14")
    two = {**sd, p + ".wavelet_convs.1.weight": sd[p + ".wavelet_convs.0.weight"], p + ".wavelet_scale.1.weight": sd[p + ".wavelet_scale.0.weight"]}
    with pytest.raises(ValueError):
        wtconv.wt_fold(two, p, "features.14")
    with pytest.raises(ValueError):
        R.wt_fold(two, p, "features.14")
    with pytest.raises(ValueError):
        wtconv.wtconv16(torch.zeros(1, 7, 8, 32, dtype=torch.float16), wtconv.wt_fold(sd, "features.3"), "fp16")   # an odd side
    with pytest.raises(ValueError):
        wtconv.wtconv16(torch.zeros(1, 8, 8, 48, dtype=torch.float16), wtconv.wt_fold(sd, "features.3"), "fp16")


# ---------------------------------------------------------------- the class
@functools.lru_cache(maxsize=None)
def _fp32():
    torch.set_num_threads(16)
    return R.forward_fp32(make_wtconv_state_dict(NAME, 0), normalize_u8(make_crops(N_CROPS, seed=CROP_SEED)), return_features=True)


def test_cpu_reference_matches_reference_goldens(golden, torch_threads):
    """forward_fp32 against the reference class's recorded fp32 logits within 1.25 x the recorded "fp32" figure,
    and each WT site's input and output map against their recorded sums and samples."""
    g, env = golden("wtconv_golden.npz"), golden("wtconv_envelope.json")
    assert int(g["crop_seed"]) == CROP_SEED and g["logits"].shape == (N_CROPS, 2)
    out, maps = _fp32()
    d = float(np.abs(out.numpy() - g["logits"]).max())
    print(f"forward_fp32 vs the golden logits: max|d| {d:.3e} (recorded {env['fp32']:.3e})")
    assert d <= ENVELOPE_MARGIN * env["fp32"]
    assert g["probs"].min() >= 0.05 and g["probs"].max() <= 0.95
    for p, _bn, c, H, pool in R.SITES:
        f, after = maps[p + "_in"], maps[p]
        assert tuple(f.shape[1:]) == (c, H, H) and tuple(after.shape[1:]) == ((c, H // 2, H // 2) if pool else (c, H, H))
        assert np.isclose(f.double().sum().item(), float(g[f"{p}_in_sum"]), rtol=1e-4), p
        assert np.isclose(after.double().sum().item(), float(g[f"{p}_sum"]), rtol=1e-3, atol=1.0), p
        assert np.allclose(after.numpy().reshape(-1)[::997], g[f"{p}_sample"], rtol=1e-3, atol=1e-4), p
        rec = env["blocks"][p]
        assert 0.25 <= rec["wavelet_over_base"] <= 4 and 0.25 <= rec["ratio"] <= 4


def test_emulation_stays_inside_the_recorded_envelope(golden, torch_threads):
    """The HIP path's rounding points (emulated) against the reference class's fp32 probabilities over the 8
    crops: the recorded envelope, which the GPU test doubles."""
    env = golden("wtconv_envelope.json")
    p_ref = torch.from_numpy(golden("wtconv_golden.npz")["probs"])
    sd = make_wtconv_state_dict(NAME, 0)
    x = normalize_u8(make_crops(N_CROPS, seed=CROP_SEED))
    for dt in ("fp16", "bf16"):
        d = float((torch.sigmoid(R.forward_emulated(sd, x, dtype=dt)) - p_ref).abs().max())
        print(f"{dt}: emulated max|dp| {d:.3e}, recorded {env[dt]:.3e}")
        assert 0 < env[dt] and d <= ENVELOPE_MARGIN * env[dt], dt


def test_dropin_state_dict_layout_and_contract(golden):
    from fac_fake_amd import odconv, wtconv
    cls = wtconv.CViT
    m = cls(image_size=224, patch_size=7, num_classes=2, channels=512, dim=1024, depth=6, heads=8, mlp_dim=2048)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == golden("wtconv_keys.json")
    sd = _sd_t()
    m.load_state_dict(sd)
    back = m.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    assert not m.training and m.variant == NAME == wtconv.NAME and m.table is WTCONV_VARIANTS[NAME]
    folded = m.folded_layers()
    assert [l[0] for l in folded] == [{"c": "conv", "w": "wt"}[k] for k in WTCONV_KINDS.replace(" ", "")]
    assert [l[-1] for l in folded] == [l[7] for l in R.LAYERS] and tuple(folded[1][1]) == wtconv.PACK_ORDER
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
    with pytest.raises(KeyError):
        odconv.odconv_class(NAME)              # the other tables' factories do not know it


def test_load_state_dict_refuses_missing_keys_and_deeper_levels():
    from fac_fake_amd import wtconv
    m = wtconv.CViT()
    sd = dict(_sd_t())
    for k in ("features.16.iwt_filter", "features.3.wavelet_scale.0.weight", "features.39.base_scale.weight"):
        with pytest.raises(RuntimeError, match=k.replace(".", r"\.")):
            m.load_state_dict({a: b for a, b in sd.items() if a != k})
    p = "features.23"
    two = {**sd, p + ".wavelet_convs.1.weight": sd[p + ".wavelet_convs.0.weight"], p + ".wavelet_scale.1.weight": sd[p + ".wavelet_scale.0.weight"]}
    with pytest.raises(ValueError, match="wavelet level"):
        m.load_state_dict(two)
    with pytest.raises(ValueError, match="wavelet level"):
        m.load_state_dict(two, strict=False)   # not ignored either
    m.load_state_dict(sd)


def test_gradcam_is_refused():
    from fac_fake_amd import wtconv
    from fac_fake_amd.gradcam import GradCAM
    with pytest.raises(NotImplementedError):
        GradCAM(wtconv.CViT())


def test_model_shim_and_prediction_loader():
    """`sys.path.insert(1, 'model/other'); from cvit_GGCA_ADD_WTConv import CViT`, and cvit_prediction's loader."""
    import cvit_prediction as P
    from fac_fake_amd import wtconv
    from fac_fake_amd.variants import variant_class
    sys.path.insert(1, str(REPO / "model" / "other"))
    try:
        mod = importlib.import_module(NAME)
    finally:
        sys.path.remove(str(REPO / "model" / "other"))
    assert mod.CViT is wtconv.CViT is variant_class(NAME) and family_entry(NAME) is WTCONV_VARIANTS[NAME]
    assert P.model_class(NAME) is wtconv.CViT and NAME not in P.MODEL_NAMES
    before = P.model
    try:
        m = P.load_model(name=NAME, dev="cpu")
    finally:
        P.model = before
    assert type(m) is wtconv.CViT and not m.training and len(m.state_dict()) == N_KEYS
    want = make_wtconv_state_dict(NAME, 0)
    assert all(np.array_equal(v.numpy(), want[k]) for k, v in m.state_dict().items())
