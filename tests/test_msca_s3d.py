"""msca_S3D without a GPU: the state_dict layout and the weight generator, the
restatement (tests/msca_s3d_ref.py) against the reference module's recorded
outputs, and the algebra the host side of fac_fake_amd/msca_s3d.py relies on."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))

import msca_s3d_ref as R  # noqa: E402
from fac_fake_amd.weights import (make_divisible, make_msca_s3d_state_dict, msca_s3d_base, msca_s3d_bn_names,  # noqa: E402
                                  msca_s3d_param_specs, s3d_clips_varied)


@pytest.mark.parametrize("srm", ["no", "yes"])
def test_keys_and_shapes_match_the_reference(golden, srm):
    ref = golden("msca_s3d_keys.json")[srm]
    ours = [[n, list(s)] for n, s, _ in msca_s3d_param_specs(1, srm == "yes")]
    assert len(ref) == 853 and ours == ref
    sd = make_msca_s3d_state_dict(0, 1, srm == "yes")
    assert [[k, list(v.shape)] for k, v in sd.items()] == ref
    assert sum(int(np.prod(s)) for n, s, k in msca_s3d_param_specs(1, srm == "yes") if k not in ("rmean", "rvar", "nbt")) \
        == (8913195 if srm == "yes" else 8828523)
    assert len(msca_s3d_bn_names(srm == "yes")) == 122


def test_make_divisible_table():
    """The channel splits of the four block kinds, as the reference module builds
    them (msca_s3d_keys.json has the shapes).  320 / 3 sits on the round-limit
    branch's edge: 0.9 x 106.666... is exactly 96.0 in float64, `96 < 96.0` is
    false, so the split stays 96 | 224 (not 128 | 192)."""
    want = {(192, 1 / 4): (64, 128, 64), (320, 1 / 3): (96, 224, 112), (320, 1 / 2): (160, 160, 80),
            (320, 2 / 3): (224, 96, 48)}
    for (c, r), (low, high, half) in want.items():
        got = make_divisible(c * r, 32)
        assert (got, c - got, (c - got) // 2) == (low, high, half)
    assert int(320 * (1 / 3) + 16) // 32 * 32 == 96 and 0.9 * (320 * (1 / 3)) == 96.0
    kinds = [L[0] for L in msca_s3d_base(False)]
    assert len(kinds) == 21 and kinds.count("iformer") == 7 and kinds.count("iformer_light") == 4
    assert [L[2] for L in msca_s3d_base(False) if L[0].startswith("iformer")] == [64, 64] + [96] * 3 + [160] * 3 + [224] * 3


def test_weight_generator_is_pinned():
    """A few per-tensor checksums (sum, |.| sum in float64) of the seed-0 weights."""
    sd = make_msca_s3d_state_dict(0, 1, False)
    got = {k: (float(np.asarray(sd[k], np.float64).sum()), float(np.abs(np.asarray(sd[k], np.float64)).sum()))
           for k in PINNED}
    for k, (s, a) in PINNED.items():
        assert got[k] == pytest.approx((s, a), rel=1e-9, abs=1e-9), (k, got[k])
    assert np.array_equal(make_msca_s3d_state_dict(0, 1, False)["fc.0.weight"], sd["fc.0.weight"])
    assert not np.array_equal(make_msca_s3d_state_dict(1, 1, False)["fc.0.weight"], sd["fc.0.weight"])


PINNED = {
    "base.0.bn_s.running_var": (np.float64(948684.4580078125), np.float64(948684.4580078125)),
    "base.5.norm1.running_mean": (np.float64(792.9968416690826), np.float64(792.9968416690826)),
    "base.5.inceptionmixer.attn.spatial_gating_unit.conv1_1.conv_s.weight": (np.float64(391.01527132093906), np.float64(489.73769541084766)),
    "base.9.inceptionmixer.fc_dw.2.bias": (np.float64(-226.91208708286285), np.float64(226.91208708286285)),
    "base.10.mlp.fc1.weight": (np.float64(-49.84262573284076), np.float64(19835.589375126998)),
    "base.17.mlp.dwconv.dwconv.bn_t.weight": (np.float64(3882.533294916153), np.float64(3882.533294916153)),
    "base.19.branch1.1.conv_s.weight": (np.float64(-4.80973454663949), np.float64(1185.5197839337159)),
    "fc.0.weight": (np.float64(0.5679742395877838), np.float64(16.332565642893314)),
}


@pytest.mark.parametrize("srm", ["no", "yes"])
def test_restatement_matches_the_reference(golden, torch_threads, srm):
    """The fp32 restatement on the fixture clips: the channel means of all 21
    base[i] outputs within 2e-5 of the reference module's (relative to the rms
    of its means) and the logits within 2e-5.  (The issue's bounds were 1e-4;
    what the generator measured and recorded as restate_mean / restate_logit
    is below 2e-5, so that is the bound.)"""
    g = R.load_blocks(golden)
    assert float(g[f"restate_logit_{srm}"]) <= 2e-5 and float(g[f"restate_mean_{srm}"].max()) <= 2e-5
    x = torch.from_numpy(s3d_clips_varied(int(g["n_clips"]), 16, 112, int(g["clip_seed"])))
    sd = R.cast_sd(make_msca_s3d_state_dict(0, 1, srm == "yes"), torch.float32)
    taps = []
    lg = R.forward(sd, x, srm == "yes", taps=taps).numpy()
    assert len(taps) == 21 and taps[-1].shape[1:] == (1024, 2, 3, 3) and taps[5].shape[1:] == (192, 8, 14, 14)
    assert np.abs(lg - g[f"logits_{srm}"]).max() <= 2e-5
    for i, t in enumerate(taps):
        ref = g[f"mean_{srm}_{i}"].astype(np.float64)
        err = np.abs(t.double().mean(dim=(2, 3, 4)).numpy() - ref).max() / np.sqrt((ref ** 2).mean())
        assert err <= 2e-5, (i, err)


def test_fixture_margins(golden):
    """What the generator asserted, re-read from the fixtures."""
    g = R.load_blocks(golden)
    for srm in ("no", "yes"):
        hi, lo = g[f"relu6_hi_{srm}"], g[f"relu6_lo_{srm}"]
        assert len(hi) == 93 and hi.min() >= 0.01 and hi.max() <= 0.6 and lo.min() > 0
        assert g[f"relu_shift_over_gate_{srm}"].min() >= 10
        for what in R.ABLATIONS:
            assert g[f"abl_{what}_{srm}"].min() >= 10, what
        neg = g[f"gelu_neg_{srm}"]
        assert len(neg) == 22 and (np.abs(g[f"logits_{srm}"]) <= 4).mean() >= 0.5


def _rand_bn(c, g):
    return {"weight": torch.rand(c, generator=g, dtype=torch.float64) * 2 - 1,       # both signs
            "bias": torch.randn(c, generator=g, dtype=torch.float64),
            "running_mean": torch.randn(c, generator=g, dtype=torch.float64),
            "running_var": torch.rand(c, generator=g, dtype=torch.float64) + 0.5}


def test_folding_identities_fp64():
    g = torch.Generator().manual_seed(1)
    c, lo, ci, co = 40, 16, 16, 24
    x = torch.randn(2, c, 3, 5, 5, generator=g, dtype=torch.float64)
    sd = {f"n.{k}": v for k, v in _rand_bn(c, g).items()}
    s, t = R.bn_affine(sd, "n")
    n = x * s.view(1, -1, 1, 1, 1) + t.view(1, -1, 1, 1, 1)
    assert torch.allclose(n, F.batch_norm(x, sd["n.running_mean"], sd["n.running_var"], sd["n.weight"], sd["n.bias"],
                                          False, 0.0, R.BN_EPS), rtol=1e-12, atol=1e-12)
    # a BatchNorm folds exactly into a 1x1x1 conv on a channel slice (proj_1, fc_dw.0's conv, fc1)
    w, b = torch.randn(co, ci, 1, 1, 1, generator=g, dtype=torch.float64), torch.randn(co, generator=g, dtype=torch.float64)
    wf, bf = R.fold_in(w, b, s, t, lo, c)
    assert torch.allclose(F.conv3d(x, wf, bf), F.conv3d(n[:, lo:lo + ci], w, b), rtol=1e-11, atol=1e-11)
    assert bool((wf[:, :lo] == 0).all()) and bool((wf[:, lo + ci:] == 0).all())
    # ... and a BatchNorm behind a conv folds into it
    sd.update({f"o.{k}": v for k, v in _rand_bn(co, g).items()})
    sd["cw"] = w
    w2, b2 = R.fold_out(sd, "cw", "o")
    s2, t2 = R.bn_affine(sd, "o")
    assert torch.allclose(F.conv3d(x[:, :ci], w2, b2), F.conv3d(x[:, :ci], w) * s2.view(1, -1, 1, 1, 1) + t2.view(1, -1, 1, 1, 1),
                          rtol=1e-11, atol=1e-11)
    # it does not fold through the max-pool where a scale is negative, but: max where s >= 0, min otherwise
    pool = lambda v: F.max_pool3d(v, (3, 3, 3), 1, (1, 1, 1))  # noqa: E731
    want = pool(n)
    naive = pool(x) * s.view(1, -1, 1, 1, 1) + t.view(1, -1, 1, 1, 1)
    assert not torch.allclose(want, naive)
    pick = torch.where(s.view(1, -1, 1, 1, 1) >= 0, pool(x), -pool(-x))
    assert torch.allclose(want, pick * s.view(1, -1, 1, 1, 1) + t.view(1, -1, 1, 1, 1), rtol=1e-12, atol=1e-12)
    assert torch.allclose(R.bn_pool_cl(x.permute(0, 2, 3, 4, 1), s, t, 3).permute(0, 4, 1, 2, 3), want)
    # dw(1,k,k) then dw(kt,1,1), zero padding, no bias = one zero-padded (kt,k,k) depthwise conv, rank-1 window
    for kt, k in ((3, 7), (1, 5), (3, 3)):
        ws = torch.randn(c, 1, 1, k, k, generator=g, dtype=torch.float64)
        wt = torch.randn(c, 1, kt, 1, 1, generator=g, dtype=torch.float64)
        two = F.conv3d(F.conv3d(x, ws, padding=(0, k // 2, k // 2), groups=c), wt, padding=(kt // 2, 0, 0), groups=c)
        one = F.conv3d(x, R.rank1_window(ws, wt), padding=(kt // 2, k // 2, k // 2), groups=c)
        assert R.rank1_window(ws, wt).shape == (c, 1, kt, k, k)
        assert torch.allclose(two, one, rtol=1e-11, atol=1e-11)
    # fc_dw's two BatchNorms are two affines around a ReLU6: they do not merge
    v = torch.randn(1000, generator=g, dtype=torch.float64) * 4
    assert not torch.allclose((v * 2 + 1).clamp(0, 6) * 0.5 - 1, ((v * 2 + 1) * 0.5 - 1).clamp(0, 6))


def test_relu6_is_relu_then_round_then_clamp():
    """round16(min(max(v, 0), 6)) == min(round16(max(v, 0)), 6): the conv's own
    ReLU epilogue followed by ops.clamp6_ gives the bits of one ReLU6 epilogue."""
    g = torch.Generator().manual_seed(2)
    v = torch.cat([torch.randn(200000, generator=g) * 4 + 3, torch.tensor([6.0, 5.9999, 6.0001, 5.998, 6.002, -0.0, 0.0])])
    for dt in (torch.float16, torch.bfloat16):
        one = v.clamp(0, 6).to(dt)
        two = v.clamp(min=0).to(dt).float().clamp(max=6).to(dt)
        assert torch.equal(one.view(torch.int16), two.view(torch.int16))


def test_harness_model():
    from fac_fake_amd.ca_s3d import CA_S3D_v3
    from fac_fake_amd.msca_s3d import harness_model, msca_S3D
    from fac_fake_amd.s3d import S3D
    assert (harness_model(0), harness_model(1), harness_model(3)) == (S3D, msca_S3D, CA_S3D_v3)
    for bad in (2, 4, -1, "1"):
        with pytest.raises(ValueError, match="model_type"):
            harness_model(bad)


def test_dropin_state_dict_and_inference_only(golden):
    from fac_fake_amd.msca_s3d import msca_S3D
    for srm in ("no", "yes"):
        m = msca_S3D(1, srm)
        assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == golden("msca_s3d_keys.json")[srm]
        with pytest.raises(RuntimeError, match="inference-only"):
            m.train(True)
        with pytest.raises(RuntimeError, match="GPU"):
            m(torch.zeros(1, 3, 16, 112, 112))
