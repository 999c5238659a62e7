"""ResKan (ResNet-34 + KAN) on the CPU: the drop-in's state_dict layout, the
fp32 restatement pinned against outputs of the reference module itself
(tests/golden/reskan_*, tools/make_golden_reskan.py), the folded BasicBlock's
arithmetic order, and the constructor's contract."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))

import reskan_ref as R  # noqa: E402
from fac_fake_amd.weights import (make_reskan_state_dict, reskan_crops_varied, reskan_param_specs,  # noqa: E402
                                  resnet34_blocks)
from oracle.cvit_torch import normalize_u8, to_torch_sd  # noqa: E402


def test_param_specs_are_the_reference_layout(golden):
    want = golden("reskan_keys.json")
    got = [[n, list(s)] for n, s, _ in reskan_param_specs()]
    assert got == want and len(got) == 224
    blocks = resnet34_blocks()
    assert len(blocks) == 16 and [b[0] for b in blocks if b[4]] == ["layer2.0", "layer3.0", "layer4.0"]


def test_dropin_state_dict_layout(golden):
    from fac_fake_amd.reskan import resnet34
    from fac_fake_amd.weights import kan_grid
    m = resnet34(set_device="cpu", num_classes=2, include_top=False, include_top_kan=True)
    sd = m.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == golden("reskan_keys.json")
    assert sd["bn1.num_batches_tracked"].dtype == torch.long
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in make_reskan_state_dict(0).items()})
    assert torch.equal(m.state_dict()["kan.layers.0.grid"], torch.from_numpy(kan_grid(512)))
    assert not m.training


def test_model_dir_reexports_the_dropin():
    import importlib.util
    p = Path(__file__).resolve().parents[1] / "model" / "kan_resnet.py"
    spec = importlib.util.spec_from_file_location("_kan_resnet_dropin", p)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from fac_fake_amd import reskan
    assert mod.resnet34 is reskan.resnet34 and mod.ResNet is reskan.ResNet


def test_restatement_matches_reference_goldens(golden, torch_threads):
    """fp32 restatement with the synthetic weights vs the reference module on
    the 8 fixture crops: logits to 1e-5 relative, the 18 taps' per-channel
    means to 1e-5 of their rms."""
    g = golden("reskan_golden_stages.npz")
    sd = make_reskan_state_dict(int(g["weight_seed"]))
    x = normalize_u8(reskan_crops_varied(int(g["n_crops"]), seed=int(g["crop_seed"])))
    taps = []
    f = R.features_fp32(sd, x, taps)
    assert len(taps) == 18
    for i, got in enumerate(R.tap_means(taps)):
        ref = g[f"mean_{i}"].astype(np.float64)
        assert got.shape == ref.shape, i
        assert np.abs(got - ref).max() <= 1e-5 * np.sqrt((ref ** 2).mean()) + 1e-7, i
    tsd = to_torch_sd(sd)
    out = R._kan(tsd, f).numpy()
    assert np.abs(out - g["logits"]).max() <= 1e-5 * np.abs(g["logits"]).max()
    assert np.array_equal(out, R.forward_fp32(sd, x).numpy())


def test_fixture_exercises_the_kan_head(golden):
    """What tools/make_golden_reskan.py asserted when it made the fixture."""
    g = golden("reskan_golden_stages.npz")
    lg, pooled = g["logits"], g["mean_17"]
    assert np.abs(lg).max() <= 4
    assert ((lg.max(0) - lg.min(0)) >= 20 * g["env_logit_fp16"]).all()
    assert ((pooled >= 0) & (pooled < 1)).mean() >= 0.5 and (pooled < 2.2).mean() >= 0.9 and (pooled > 1).mean() >= 0.01
    assert float(g["env_prob_fp16"]) <= 5e-4


def test_emulation_within_16bit_envelope(golden, torch_threads):
    """The HIP path's rounding points (emulated) against the reference: the 18
    taps within the gate the GPU path has to meet (2 env + 1e-4), fp16
    probabilities within the 1e-3 bar, bf16 within 2 env_prob."""
    g = golden("reskan_golden_stages.npz")
    sd = make_reskan_state_dict(int(g["weight_seed"]))
    x = normalize_u8(reskan_crops_varied(int(g["n_crops"]), seed=int(g["crop_seed"])))
    p_ref = 1 / (1 + np.exp(-g["logits"].astype(np.float64)))
    for dt in ("fp16", "bf16"):
        taps = []
        f = R.features_emulated(sd, x, dt, taps)
        for i, got in enumerate(R.tap_means(taps)):
            ref = g[f"mean_{i}"].astype(np.float64)
            err = float(np.abs(got - ref).max() / np.sqrt((ref ** 2).mean()))
            assert err <= 2 * g[f"env_{dt}"][i] + 1e-4, (dt, i, err)
        p = torch.sigmoid(R._kan(to_torch_sd(sd), f)).double().numpy()
        assert np.abs(p - p_ref).max() <= (1e-3 if dt == "fp16" else 2 * float(g[f"env_prob_{dt}"])), dt


@pytest.mark.parametrize("p,stride,ds,cin", [("layer1.1", 1, False, 64), ("layer2.0", 2, True, 64)])
def test_folded_block_order_is_bn2_add_relu(p, stride, ds, cin):
    """The folded block (BN folded into the convs; conv2's epilogue + bias, +
    identity, ReLU) equals BasicBlock.forward (kan_resnet.py:38-65), and the
    ReLU-before-add order of ResVitKan's Bottleneck does not: the input has
    both signs, so the identity is negative where it matters."""
    sd = to_torch_sd(make_reskan_state_dict(0))
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, cin, 12, 12, generator=g)
    want = R.basic_block_fp32(sd, p, x, stride, ds)
    got = R.folded_block(sd, p, x, stride, ds)
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= 1e-5 * scale

    def conv(h, ck, bnp, s=1, pad=0):
        w, b = R.fold_bn(sd, ck, bnp)
        return F.conv2d(h, w, b, stride=s, padding=pad)
    identity = conv(x, p + ".downsample.0.weight", p + ".downsample.1", stride) if ds else x
    h = F.relu(conv(x, p + ".conv1.weight", p + ".bn1", stride, 1))
    wrong = F.relu(F.relu(conv(h, p + ".conv2.weight", p + ".bn2", 1, 1)) + identity)
    assert float((wrong - want).abs().max()) > 1e-2 * scale
    assert float(want.min()) == 0.0 and float((want == 0).float().mean()) > 0.05


def test_constructor_contract():
    from fac_fake_amd.reskan import ResNet, resnet34
    for kw in (dict(num_classes=1000), dict(num_classes=2, include_top=True),
               dict(num_classes=2, include_top_kan=False), dict(num_classes=3)):
        with pytest.raises(NotImplementedError):
            resnet34(set_device="cpu", **kw)
    with pytest.raises(NotImplementedError):
        ResNet(None, [3, 4, 23, 3], set_device="cpu", num_classes=2)
    with pytest.raises(ValueError):
        resnet34(set_device="cpu", num_classes=2, dtype="fp32")
    m = resnet34(set_device="cpu", num_classes=2, dtype="bf16")
    with pytest.raises(RuntimeError):
        m.train()
    with pytest.raises(RuntimeError):
        m.train(True)
    assert m.train(False) is m and m.eval() is m
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 224, 224))                      # no CPU fallback
    with pytest.raises(RuntimeError):
        m.forward_u8(torch.zeros(1, 224, 224, 3, dtype=torch.uint8))
