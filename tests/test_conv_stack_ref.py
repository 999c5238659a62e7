"""The references and operand sets of tests/conv_stack_ref.py, checked on the CPU:
the yardstick of tests/test_conv_stack_gpu.py has to be right on its own."""
import json
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import conv_stack_ref as R  # noqa: E402


def _conv_by_shifts(x, w, bias):
    """3x3 conv, padding 1, as nine shifted products (float64 NHWC): no conv2d."""
    n, h, _, _ = x.shape
    xp = torch.zeros(n, h + 2, h + 2, x.shape[3], dtype=torch.float64)
    xp[:, 1:-1, 1:-1] = x.double()
    out = bias.double().view(1, 1, 1, -1).expand(n, h, h, w.shape[0]).clone()
    for ky in range(3):
        for kx in range(3):
            out += torch.einsum("nyxc,oc->nyxo", xp[:, ky:ky + h, kx:kx + h], w[:, :, ky, kx].double())
    return out


@pytest.mark.parametrize("pool,relu", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_conv3x3_ref_is_conv_bias_relu_pool_in_that_order(pool, relu):
    x, w, bias = R.random_operands(6, 32, 8, 2, "bf16", 5)
    ref, a = R.conv3x3_ref(x, w.to(torch.bfloat16), bias, pool, relu)
    want = _conv_by_shifts(x, w, bias)
    amax = _conv_by_shifts(x.double().abs(), w.abs(), bias.abs())
    if relu:
        want = want.clamp_min(0)
    if pool:
        want = want.view(2, 3, 2, 3, 2, 8).amax(dim=(2, 4))
        amax = amax.view(2, 3, 2, 3, 2, 8).amax(dim=(2, 4))
    assert ref.dtype == torch.float64 and ref.shape == want.shape
    assert torch.allclose(ref, want, rtol=0, atol=1e-12) and torch.allclose(a, amax, rtol=0, atol=1e-12)
    assert (float(ref.min()) < 0) == (not relu)


def test_exact_operands_are_exact_and_cover_every_tap_and_channel():
    for h, cin, cout, edge in ((14, 96, 64, False), (28, 32, 1280, False), (14, 64, 192, True)):
        x, w, bias = R.exact_operands(h, cin, cout, 2, "bf16", 3, edge=edge)
        assert set(x.float().unique().tolist()) <= {-1.0, 0.0, 1.0} and set(w.unique().tolist()) == {-1.0, 0.0, 1.0}
        assert bool((w.view(cout // 32, 32, cin * 9) != 0).any(1).all())
        assert torch.equal(bias, bias.round()) and float(bias.min()) < 0 < float(bias.max())
        ref, a = R.conv3x3_ref(x, w.to(torch.bfloat16), bias, 0, 0)
        assert float(a.max()) <= R.EXACT_MAX and torch.equal(ref, ref.round())
        assert torch.equal(ref.to(torch.bfloat16).double(), ref) and torch.equal(ref.to(torch.float16).double(), ref)
        if edge:
            assert not bool(x[:, :h - 1, :h - 1].any()) and bool(x[:, h - 1].any()) and bool(x[:, :, h - 1].any())


def test_stem_ref_rounding_points_and_mutants():
    """One crop of the exact-integer chain: float32 and float64 accumulation agree
    exactly, the value is what three plain convs give, and the two mutants of the
    envelope tool change what they should: the dropped tap the whole map, the
    non-zeroed conv1 border only the outermost pooled pixels."""
    ops = R.stem_exact_operands(1, 11)
    inp, w1, b1, w2, b2, w3, b3 = ops
    assert max(R.stem_stage_maxima(*ops)) <= R.EXACT_MAX
    ref = R.stem_ref(*ops, "bf16", False)
    assert ref.shape == (1, 112, 112, 32) and ref.dtype == torch.float64
    assert torch.equal(ref, R.stem_ref(*ops, "fp16", False, acc=torch.float32).double())
    x = inp.permute(0, 2, 3, 1)
    for w, b in ((w1, b1), (w2, b2)):
        x = _conv_by_shifts(x, w, b).clamp_min(0)
    want = _conv_by_shifts(x, w3, b3).clamp_min(0).view(1, 112, 2, 112, 2, 32).amax(dim=(2, 4))
    assert torch.equal(ref, want)
    border = R.stem_ref(*ops, "bf16", False, mutant="pad_relu_b1") != ref
    assert bool(border.any()) and not bool(border[:, 1:-1, 1:-1].any())
    tap = R.stem_ref(*ops, "bf16", False, mutant="drop_tap") != ref
    assert bool(tap[:, 1:-1, 1:-1].any())


def test_stem_ref_u8_input_is_the_rounded_fp32_normalisation():
    u8 = torch.arange(256, dtype=torch.uint8).view(1, 16, 16, 1).expand(1, 16, 16, 3).contiguous()
    x = R.normalize_u8_f32(u8)
    assert x.dtype == torch.float32 and x.shape == (1, 3, 16, 16)
    for c in range(3):
        v = torch.arange(256, dtype=torch.float64)
        want = ((v / 255 - R.MEAN[c]) / R.STD[c])
        # fp32: v/255, the fp32 mean and the subtraction each err by <= 2^-25 (values < 1), divided by
        # std >= 0.224 (x 4.5: 4e-7); std's own rounding 2^-25 relative of |x| < 2.7 (8e-8); the last
        # rounding 2^-23 (|x| < 4): under 2^-20 in all
        assert float((x[0, c].reshape(-1).double() - want).abs().max()) <= 2.0 ** -20


def test_recorded_envelope_is_complete_and_its_mutants_miss_the_gate(golden):
    env = golden("conv_stack_envelope.json")
    assert env["margin"] == 2.0 and env["n"] == R.STEM_RANDOM_N and env["seed"] == R.STEM_RANDOM_SEED
    for dt in ("fp16", "bf16"):
        for path in ("u8", "f32"):
            e = env[dt][path]
            assert 0 < e["ulp"] < 4 and 0 < e["flips"] < 0.05, (dt, path, e)
            assert set(e["mutants"]) == {"drop_tap", "pad_relu_b1"}
            assert all(m["ratio"] >= 10 for m in e["mutants"].values()), (dt, path, e)
    assert len(json.dumps(env)) < 2048
