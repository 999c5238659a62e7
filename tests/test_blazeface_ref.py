"""tests/blazeface_ref.py pinned on the CPU, without the kernels:

(a) composed with the trained weights it reproduces the fp64 activations the
    fixture generator recorded from the reference's own classes;
(b) a float32 evaluation of it lies inside gamma_n A at every case of
    tests/test_blazeface_layers_gpu.py, so that gate admits a correct float32
    kernel;
(c) each of eleven wrong kernels, built into the reference as ``mutant=``, is
    outside BOTH of that file's gates (bit equality on the exact operands,
    gamma_n A on the random ones) at every case it applies to, so those gates
    can see such a fault;
and the fast tile reference equals the int64 restatement.
"""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import blazeface_ref as R  # noqa: E402
from fac_fake_amd import blazeface as bz  # noqa: E402


@functools.lru_cache(maxsize=None)
def _sd(kind):
    return R.exact_state_dict() if kind == "exact" else R.random_state_dict()


@functools.lru_cache(maxsize=None)
def _case(kind, kernel):
    """(inputs, outputs, A) of one layer case at T = 3, float64; T = 1 is its first tile."""
    inputs = R.case_inputs(kind, kernel)
    out, mags = R.run_ref(_sd(kind), kernel, inputs)
    return inputs, out, mags


def test_reference_reproduces_the_golden_fp64_activations(golden):
    G, W = golden("blazeface_golden.npz"), golden("blazeface_weights.npz")
    crops = golden("golden_real.npz")["crops"]
    tiles = bz.tile_frames_np(bz.fixture_input("video", crops, G["video_paste"]))[:5]
    b1, b2, r, c = R.net_ref(W, tiles)
    got = {"b1": b1.reshape(5, 256, 88)[:, G["b1_pix"]], "b2": b2.reshape(5, 64, 96)[:, G["b2_pix"]],
           "r": r[:, G["r_rows"]], "c": c[..., None]}
    for k, v in got.items():
        err = float(np.abs(v - G[f"{k}_64"]).max())
        print(f"{k}: max|ref - golden fp64| = {err:.3e}")
        assert v.shape == G[f"{k}_64"].shape and err <= 1e-12, k
    assert float(np.abs(G["c_64"]).max()) > 1 and float(np.abs(G["r_64"]).max()) > 1      # not a comparison of zeros


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_exact_operands_are_exact(kernel):
    """Integers throughout, every partial sum below 2^24: any float32 evaluation gives these bits."""
    inputs, out, mags = _case("exact", kernel)
    assert all(float(a.max()) < 2 ** 24 for a in mags)
    assert all(np.array_equal(o, np.round(o)) for o in out)
    assert all(float(o.max()) > 0 for o in out) and all(float((o == 0).mean()) < 0.9 for o in out)
    out32, _ = R.run_ref(_sd("exact"), kernel, inputs, dt=np.float32)
    assert all(o.dtype == np.float32 and np.array_equal(o, w) for o, w in zip(out32, out))
    print(f"{kernel}: max |v| {max(float(a.max()) for a in mags):.0f}")


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_float32_evaluation_is_inside_the_bound(kernel):
    for kind in ("random", "exact"):
        inputs, out, mags = _case(kind, kernel)
        out32, _ = R.run_ref(_sd(kind), kernel, inputs, dt=np.float32)
        worst = R.worst_ratio(kernel, out32, out, mags)
        print(f"{kernel} {kind}: float32 evaluation at {worst:.3f} of gamma_n A")
        assert worst <= 1.0, (kernel, kind, worst)
        if kind == "random":
            assert worst > 0                                    # the float32 run does round: the gate is not vacuous
            one = R.worst_ratio(kernel, [o[:1] for o in out32], [o[:1] for o in out], [a[:1] for a in mags])
            assert one <= 1.0                                   # T = 1


def test_stem_edge_tiles_tell_the_pad_value():
    sd, tiles = _sd("exact"), R.stem_edge_tiles()
    out, _ = R.stem_ref(tiles, sd["backbone1.0.weight"], sd["backbone1.0.bias"])
    assert np.array_equal(out, np.round(out))
    for m in ("stem_pad_before_norm", "stem_pad_2121"):
        bad, _ = R.stem_ref(tiles, sd["backbone1.0.weight"], sd["backbone1.0.bias"], mutant=m)
        assert all(not np.array_equal(bad[t], out[t]) for t in range(3)), m
    # the all-0 tile is -1 everywhere inside: interior outputs are b - sum(w), edge outputs differ
    w, b = sd["backbone1.0.weight"].astype(np.float64), sd["backbone1.0.bias"].astype(np.float64)
    assert np.array_equal(out[0, 5, 7], np.maximum(b - w.sum((1, 2, 3)), 0))
    assert np.array_equal(out[0, 0, 0], np.maximum(b - w[:, :, 1:, 1:].sum((1, 2, 3)), 0))
    assert np.array_equal(out[1, 63, 63], np.maximum(b + w[:, :, :3, :3].sum((1, 2, 3)), 0))


@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_mutant_fails_the_exact_and_the_bound_check(mutant):
    assert R.MUTANTS[mutant]
    for kernel in R.MUTANTS[mutant]:
        inputs, out, _ = _case("exact", kernel)
        bad, _ = R.run_ref(_sd("exact"), kernel, inputs, mutant=mutant)
        assert any(not np.array_equal(b, o) for b, o in zip(bad, out)), (mutant, kernel, "exact")
        inputs, out, mags = _case("random", kernel)
        bad, _ = R.run_ref(_sd("random"), kernel, inputs, mutant=mutant)
        # 2: the wrong kernel's own float32 rounding cannot bring it back inside
        worst3 = R.worst_ratio(kernel, bad, out, mags)
        worst1 = R.worst_ratio(kernel, [o[:1] for o in bad], [o[:1] for o in out], [a[:1] for a in mags])
        print(f"{mutant} {kernel}: {worst1:.3g} (T = 1), {worst3:.3g} (T = 3) of gamma_n A")
        assert worst1 > 2 and worst3 > 2, (mutant, kernel, worst1, worst3)


def test_the_mutant_list_is_the_one_the_checks_were_designed_against():
    assert len(R.MUTANTS) == 11
    used = {k for v in R.MUTANTS.values() for k in v}
    assert used == set(R.KERNELS)
    with_index = {i: bz.BlazeFace.block_shapes(i) for i in range(16)}
    assert all(R.block_shapes(i) == s for i, s in with_index.items())
    assert with_index[0] == ((64, 64, 24), (64, 64, 24)) and with_index[15] == ((8, 8, 96), (8, 8, 96))
    assert with_index[11] == ((16, 16, 88), (8, 8, 96))


@pytest.mark.parametrize("H,Wd", [(300, 301), (131, 517), (128, 128), (256, 256)])
def test_fast_tile_reference_equals_the_integer_restatement(H, Wd):
    fr = np.random.default_rng(H).integers(0, 256, (2, H, Wd, 3), dtype=np.uint8)
    assert np.array_equal(R.tile_frames_ref(fr), bz.tile_frames_np(fr))
    lim = R.limit_frame(H, Wd)
    assert float((lim == 255).mean()) > 0.98 and int((lim != 255).sum()) > 100
    assert np.array_equal(R.tile_frames_ref(lim), bz.tile_frames_np(lim))


def test_fast_tile_reference_at_the_accumulator_limit():
    """2048 px all 255: the largest numerator, 255 n^2, and the result is 255; one
    exact column of the 2049 px case against Python integers."""
    assert np.array_equal(R.area_resize_ref(np.full((2048, 2048, 3), 255, np.uint8)),
                          np.full((128, 128, 3), 255, np.uint8))
    fr = R.limit_frame(2049, 2049)[0]
    got = R.area_resize_ref(fr)
    n, ov = 2049, bz._overlap(2049, 128)
    for oy, ox in ((0, 0), (127, 127), (64, 3)):
        ys, xs = np.nonzero(ov[oy])[0], np.nonzero(ov[ox])[0]
        num = sum(int(ov[oy, y]) * int(ov[ox, x]) * int(fr[y, x, 1]) for y in ys for x in xs)
        assert got[oy, ox, 1] == (2 * num + n * n) // (2 * n * n)
