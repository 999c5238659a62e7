"""The gates of test_gpu_side_ops.py, checked without a GPU on the references
alone (tests/side_ops_ref.py): if plain fp32 torch could not meet a gate
against the fp64 truth, a kernel that misses it would prove nothing.

* GGCA: the oracle's fp32 arithmetic and the fp64 reference, both rounded to
  16 bits, differ by at most one 16-bit value, on at most 0.1 % of the outputs
  (the GPU gate allows 0.5 %), on every case of GGCA_CASES, both types.
* KANLinear: the fp32 oracle stays inside (9 in_f + 32) 2^-24 A of fp64 on
  every case of KAN_CASES, with the planted knot / out-of-range / +-1e4 inputs.
* kan_ref reproduces the reference module's own outputs (resvitkan_golden.npz).
"""
import numpy as np
import pytest
import torch

import side_ops_ref as R
from fac_fake_amd.weights import make_resvitkan_state_dict


def test_round16_rounds_once():
    """A value just above an fp16 midpoint that fp32 rounds ONTO the midpoint: two roundings tie to even
    (down), one rounding goes up."""
    x = torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -40, -(1.0 + 2.0 ** -11 + 2.0 ** -40), 1.0 + 2.0 ** -11, 0.1],
                     dtype=torch.float64)
    got = R.round16(x, "fp16").double()
    assert got.tolist() == [1.0 + 2.0 ** -10, -(1.0 + 2.0 ** -10), 1.0, float(torch.tensor(0.1).half())]
    assert x.float().half().double()[0] == 1.0           # what two roundings give
    a = torch.tensor([1.0, -0.0, 2.0 ** -24], dtype=torch.float16)
    b = torch.tensor([1.0 + 2.0 ** -10, 0.0, -(2.0 ** -24)], dtype=torch.float16)
    assert R.ulp_dist(a, b).tolist() == [1, 0, 2]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("case", R.GGCA_CASES, ids=lambda c: "x".join(map(str, c)))
def test_ggca_fp32_oracle_within_flip_cap(case, dt, torch_threads):
    x16, prm = R.ggca_inputs(case, dt)
    xn = x16.permute(0, 3, 1, 2)
    r64 = R.round16(R.ggca_ref(xn, *prm, case[4]), dt)
    r32 = R.round16(R.ggca_ref(xn, *prm, case[4], dtype=torch.float32), dt)
    d = R.ulp_dist(r32, r64)
    share = float((d > 0).float().mean())
    print(f"ggca {case} {dt}: fp32 vs fp64 max {int(d.max())} ulp, share {share:.5f}")
    assert int(d.max()) <= 1 and share <= R.GGCA_FLIP_CAP_REF, (int(d.max()), share)
    # the inputs keep the edges the cases are there for: an all-negative pooled line, BN weights of both signs
    assert bool((x16.float().amax(dim=2) < 0).any()) and bool((x16.float().amax(dim=1) < 0).any())
    assert case[3] // case[4] < 32 or (bool((prm[2][2] > 0).any()) and bool((prm[2][2] < 0).any()))


@pytest.mark.parametrize("case", R.KAN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_kan_fp32_oracle_within_bound(case, torch_threads):
    ops = R.kan_inputs(case)
    y64, a = R.kan_ref(*ops)
    y32, _ = R.kan_ref(*ops, dtype=torch.float32)
    err, bound = (y32.double() - y64).abs(), R.kan_bound(a, case[1])
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"kan {case}: fp32 vs fp64 max err/bound {ratio:.4f}")
    assert bool((err <= bound).all()), ratio
    dead = a == 0                                        # rows whose features are all zero
    assert case[0] < 3 or bool(dead.any())
    assert bool((y32[dead] == 0).all()) and bool((y64[dead] == 0).all())


def test_kan_inputs_plant_the_edges():
    x, grid, *_ = R.kan_inputs((33, 40, 70))
    for i in (0, 1, 39):
        assert torch.equal(x[:12, i], grid[i])           # every knot, the first and the last included
    assert bool((grid[:, 1:] - grid[:, :-1] >= 0.1 - 1e-6).all())
    assert bool((x[32] < grid[:, 0]).any()) and bool((x[32] > grid[:, -1]).any())
    assert 1e4 in x[32].tolist() and -1e4 in x[32].tolist() and bool((x[31] == -1e4).all())
    z = x[32][x[32] == 0]
    assert z.numel() == 2 and sorted(torch.signbit(z).tolist()) == [False, True]
    x5, g5, *_ = R.kan_inputs((5, 500, 3))
    hit = {int(j) for i in range(24) for j in torch.nonzero(g5[i].unsqueeze(0) == x5[:, i].unsqueeze(1))[:, 1]}
    assert hit == set(range(12))


def test_kan_ref_reproduces_the_golden(golden):
    g = golden("resvitkan_golden.npz")
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in make_resvitkan_state_dict(0).items()}
    p = "kan_head.3.layers.0"
    y, a = R.kan_ref(torch.from_numpy(g["kan_x"]), sd[p + ".grid"], sd[p + ".base_weight"], sd[p + ".spline_weight"],
                     sd[p + ".spline_scaler"])
    assert np.abs(y.numpy() - g["kan_y"]).max() <= 1e-5
    assert bool((a >= y.abs() - 1e-12).all())


def test_pack_refs_place_every_pixel():
    """The two packer references against plain index loops on a tiny input."""
    g = torch.Generator().manual_seed(2)
    clip = torch.randint(0, 256, (2, 3, 3, 4, 6), generator=g).float()
    ref = R.pack_s2d_ref(clip, 1, 2, 1.0, None, None, "fp16")
    assert tuple(ref.shape) == (2, 3, 5, 6, 16)
    want = torch.zeros_like(ref)
    for b in range(2):
        for f in range(3):
            for y in range(4):
                for x in range(6):
                    for c in range(3):
                        want[b, f, y // 2 + 1, x // 2 + 1, 4 * (2 * (y % 2) + x % 2) + c] = clip[b, c, f, y, x]
    assert torch.equal(ref, want)
    pk = R.pack_input_ref(clip, False, 1.0, None, None, 24, "bf16")
    assert tuple(pk.shape) == (2, 72, 24) and bool((pk[..., 3:] == 0).all())
    assert torch.equal(pk[1, 2 * 24 + 3 * 6 + 5, :3].float(), clip[1, :, 2, 3, 5].bfloat16().float())


def test_sigmoid_inputs_and_bound():
    for n in (1, 257, 1000):
        x = R.sigmoid_inputs(n)
        assert x.numel() == n and x[0] == 0
    x = R.sigmoid_inputs(1000)
    assert x.min() == -float("inf") and x.max() == float("inf") and x[3] == -104 and x[-1] == 104
    ref = R.sigmoid_ref(x)
    y32 = torch.sigmoid(x)                                # torch's own fp32 sigmoid meets the gate
    assert bool(((y32.double() - ref).abs() <= R.sigmoid_bound(ref)).all())
