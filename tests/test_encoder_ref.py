"""The gates of test_gpu_encoder.py, proven without a GPU on the references
alone (tests/encoder_ref.py).

* The references pass: for every case and both 16-bit types the float32
  restatement of each kernel (the kernel's own order: per-lane partial sums,
  then the xor butterfly of wave_sum) passes ``compare16`` against fp64 and
  changes under half of FLIP_CAP of the outputs; the residual sums are exact.
* Wrong arithmetic fails: each mutant (eps 1e-6 for 1e-5 and the reverse,
  unbiased variance, a slab left out, slab stride B for 2B, pos row off by
  one, the clamps exchanged, attention scale 128^-0.5, attention rows
  swapped, softmax without the max subtraction in float32, q and k offsets
  exchanged) is REJECTED by the same comparator on a committed case.
* The floor constant F of encoder_ref.py is twice what these restatements need.
* The video-score inputs are exact: fp64 and a sequential float32 sum agree
  bit for bit, on every branch of pre_process_prediction and across the LDS
  pass boundaries of both kernels.
"""
import pytest
import torch

import encoder_ref as E

DTS = ["bf16", "fp16"]


def _resid(R, S, eps, dt, mut=None, ref_eps=None):
    """compare16 of resid_layernorm's restatement (mut None) or of a mutated fp64 result against the reference."""
    i = E.resid_inputs(R, S)
    a = (i["x"], i["slab"], i["bias"], i["gamma"], i["beta"])
    x64, y64 = E.resid_ln_ref(*a, eps)
    if mut is None and ref_eps is None:
        x32, y = E.resid_ln_f32(*a, eps, dt)
        assert torch.equal(x32.double(), x64) and torch.equal(x64, i["rows"])     # the residual sum is exact
    else:
        y = E.round16(E.resid_ln_ref(*a, eps if ref_eps is None else ref_eps, mut)[1], dt)
    return E.compare16(y, y64, dt)


def _embed(B, S, which, dt, mut=None):
    i = E.embed_inputs(B, S)
    a = (i["slab"], i["bias"], i["cls"], i["pos"])
    pidx = E.PIDX[B][which]
    x64, y64 = E.embed_ref(*a, pidx, i["gamma"], i["beta"])
    if mut is None:
        x32, y = E.embed_f32(*a, pidx, i["gamma"], i["beta"], dt)
        assert torch.equal(x32.double(), x64)
        assert which != "in_range" or torch.equal(x64, i["rows"])
    else:
        y = E.round16(E.embed_ref(*a, pidx, i["gamma"], i["beta"], mut=mut)[1], dt)
    return E.compare16(y, y64, dt)


def _attention(B, dt, mut=None):
    qkv = E.attention_inputs(B)
    ref = E.attention_ref(qkv)
    if mut is None:
        got = E.attention_f32(qkv, dt)
    elif mut == "no_max":
        got = E.attention_f32(qkv, dt, max_subtract=False)
    else:
        got = E.round16(E.attention_ref(qkv, mut=mut), dt)
    return E.compare16(got, ref, dt)


def _all_reference_results(dt):
    out = {}
    for R in (6, 2):
        for S in E.RESID_S:
            for eps in E.RESID_EPS:
                out[f"resid_ln R{R} S{S} eps{eps:g}"] = _resid(R, S, eps, dt)
    for B in (3, 1):
        for S in E.EMBED_S:
            for which in E.PIDX[B]:
                out[f"embed_ln B{B} S{S} {which}"] = _embed(B, S, which, dt)
    for B in (6, 1):
        out[f"attention B{B}"] = _attention(B, dt)
    return out


@pytest.fixture(scope="module")
def reference_results():
    return {dt: _all_reference_results(dt) for dt in DTS}


@pytest.mark.parametrize("dt", DTS)
def test_float32_restatements_pass_the_comparator(reference_results, dt):
    for name, c in reference_results[dt].items():
        print(f"{dt} {name}: share {c['share']:.5f} max {c['max_ulps']:.2f} ulp excess {c['excess']:.3g}")
        assert c["ok"] and c["share"] <= E.FLIP_CAP / 2, (dt, name, c)


def test_floor_constant_is_twice_the_measured_excess(reference_results):
    """F of encoder_ref.py: the largest amount by which a float32 restatement exceeds one 16-bit ulp of the
    reference, relative to the row maximum, doubled.  (Measured: no output of any case exceeds one ulp, so the
    excess and the floor are 0 and the GPU gate is one ulp everywhere.)"""
    worst = max(c["excess"] for r in reference_results.values() for c in r.values())
    print(f"largest excess over one ulp, relative to the row maximum: {worst:.3g}")
    assert max(worst, 0.0) <= E.F_MEASURED and E.F == 2 * E.F_MEASURED


def test_out_of_range_slots_clamp_to_the_ends():
    for S in E.EMBED_S:
        i = E.embed_inputs(3, S)
        a = (i["slab"], i["bias"], i["cls"], i["pos"])
        lo = E.embed_ref(*a, E.PIDX[3]["out_of_range"], i["gamma"], i["beta"])
        hi = E.embed_ref(*a, E.PIDX[3]["clamped"], i["gamma"], i["beta"])
        assert torch.equal(lo[0], hi[0]) and torch.equal(lo[1], hi[1])


def test_ln_rows_are_the_six_kinds():
    rows = E.ln_rows(6)
    var = rows.var(dim=-1, unbiased=False)
    assert torch.equal(rows, torch.round(rows / E.Q) * E.Q) and float(rows.abs().max()) <= 448
    assert 0.8 < var[0] < 1.2 and abs(float(rows[1].mean()) - 3) < 0.1 and 0.2 < var[1] < 0.3
    assert 2e-6 < var[2] < 6e-6 and abs(float(rows[2].mean()) - 0.25) < 1e-3      # below eps 1e-5, above 1e-6
    assert var[3] == 0 and bool((rows[3] == 0.75).all())
    assert rows[4, E.SPIKE_COL] == 40 and float(rows[4].abs().sort().values[-2]) < 0.03
    assert 80 ** 2 < var[5] < 120 ** 2
    assert torch.equal(E.ln_rows(2), torch.stack([x for x in E.ln_rows(2)])) and E.ln_rows(2).shape == (2, E.DIM)
    g, b = E.ln_params()
    assert 0.8 <= float(g.min()) and float(g.max()) <= 1.2 and -0.1 <= float(b.min()) and float(b.max()) <= 0.1


# (name, thunk -> compare16 result of the mutant); every one must be rejected
MUTANTS = [
    ("eps 1e-6 where 1e-5 was asked", lambda dt: _resid(6, 4, 1e-5, dt, ref_eps=1e-6)),
    ("eps 1e-5 where 1e-6 was asked", lambda dt: _resid(6, 4, 1e-6, dt, ref_eps=1e-5)),
    ("eps 1e-5 where 1e-2 was asked", lambda dt: _resid(6, 1, 1e-2, dt, ref_eps=1e-5)),
    ("one slab left out (resid_ln S 4)", lambda dt: _resid(6, 4, 1e-5, dt, mut="drop_slab")),
    ("one slab left out (resid_ln S 2, R 2)", lambda dt: _resid(2, 2, 1e-5, dt, mut="drop_slab")),
    ("slab stride B instead of 2B", lambda dt: _resid(6, 2, 1e-5, dt, mut="stride")),
    ("one slab left out (embed_ln S 28)", lambda dt: _embed(3, 28, "in_range", dt, mut="drop_slab")),
    ("one slab left out (embed_ln S 7, B 1)", lambda dt: _embed(1, 7, "in_range", dt, mut="drop_slab")),
    ("pos row off by one", lambda dt: _embed(3, 14, "in_range", dt, mut="pos_shift")),
    ("clamp to 0 / 31 exchanged", lambda dt: _embed(3, 14, "out_of_range", dt, mut="clamp_swap")),
    ("attention scale 128 ** -0.5", lambda dt: _attention(6, dt, mut="head_scale")),
    ("attention scale 128 ** -0.5 (B 1)", lambda dt: _attention(1, dt, mut="head_scale")),
    ("attention rows swapped", lambda dt: _attention(6, dt, mut="swap_rows")),
    ("q and k head offsets exchanged", lambda dt: _attention(6, dt, mut="swap_qk")),
    ("softmax without max subtraction in float32", lambda dt: _attention(6, dt, mut="no_max")),
]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name,run", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_wrong_arithmetic_is_rejected(name, run, dt):
    c = run(dt)
    print(f"{dt} {name}: share {c['share']:.4f} max {c['max_ulps']:.1f} ulp")
    assert not c["ok"], (name, dt, c)


def test_unbiased_variance_is_rejected():
    """Variance / 1023 moves every normalised value by 4.9e-4 of itself, at most one 16-bit value away from zero,
    so it shows in the flip share: fp16 (ulp 4.9e-4 .. 9.8e-4 of the value) flips 38 - 55 % of a case's outputs,
    bf16 (ulp 8x larger) 7.6 % of the six-row case; both are past the 5 % cap, and outputs near zero (beta against
    the normalised value) sit tens of ulps off besides."""
    for R, S, eps in ((6, 4, 1e-5), (6, 1, 1e-6), (2, 2, 1e-5)):
        c = _resid(R, S, eps, "fp16", mut="unbiased")
        print(f"fp16 unbiased R{R} S{S}: share {c['share']:.4f} max {c['max_ulps']:.1f} ulp")
        assert not c["ok"] and c["share"] > 4 * E.FLIP_CAP, c
    assert not _embed(3, 14, "in_range", "fp16", mut="unbiased")["ok"]
    c = _resid(6, 4, 1e-5, "bf16", mut="unbiased")
    print(f"bf16 unbiased R6 S4: share {c['share']:.4f} max {c['max_ulps']:.1f} ulp")
    assert not c["ok"] and c["share"] > E.FLIP_CAP, c


def test_attention_inputs_reach_past_expf_overflow():
    """Crop 4's largest logit is beyond 88.72 (expf overflows fp32 there), crop 5 attends uniformly, and the
    amplitudes grow as documented."""
    lg = E.attention_logits(E.attention_inputs(6))
    top = lg.abs().amax(dim=(1, 2, 3))
    print("largest |logit| per crop:", [round(float(t), 2) for t in top])
    assert 3 < top[0] < 6 and 10 < top[1] < 20 and 20 < top[2] < 30 and 50 < top[3] < 80 and float(lg[4].max()) > 89
    assert top[5] == 0
    ref = E.attention_ref(E.attention_inputs(6))
    qkv = E.attention_inputs(6).double()
    mean_v = 0.5 * (qkv[10, 2 * E.DIM:] + qkv[11, 2 * E.DIM:])
    assert torch.equal(ref[10], mean_v) and torch.equal(ref[11], mean_v)
    assert bool(torch.isnan(E.attention_f32(E.attention_inputs(6), "fp16", max_subtract=False).float()).any())


@pytest.mark.parametrize("B", [1, 5])
def test_head_restatement_within_the_dot_product_bound(B):
    i = E.head_inputs(B)
    logits, probs, bound = E.head_ref(**i)
    l32, p32 = E.head_f32(**i)
    assert float(logits.min()) < -29 and float(logits.max()) > 29          # both sides of the sigmoid saturate
    assert bool(((l32.double() - logits).abs() <= bound).all())
    assert bool(((p32.double() - probs).abs() <= bound + E.HEAD_SIGMOID_U).all())
    assert float(p32.max()) == 1.0 and float(p32.min()) < 1e-12
    print(f"head B{B}: logits err/bound {float(((l32.double() - logits).abs() / bound).max()):.4f}")


def test_resid_cls_reads_only_the_cls_rows():
    for B in (1, 3):
        for S in E.RESID_S:
            i = E.resid_cls_inputs(B, S)
            ref = E.resid_cls_ref(**i)
            assert bool(torch.isnan(i["x"][1::2]).all()) and bool(torch.isnan(i["slab"][:, 1::2]).all())
            assert bool(torch.isfinite(ref).all()) and tuple(ref.shape) == (B, E.DIM)
            assert torch.equal(ref.float().double(), ref)                    # exact in fp32: one rounding to 16 bits
            for dt in DTS:
                assert not E.compare16(E.round16(E.resid_cls_ref(**i, mut="drop_slab"), dt), ref, dt)["ok"]


@pytest.mark.parametrize("n,rest,edge,branch", E.SCORE_CASES + E.SEG_CASES,
                         ids=[f"n{c[0]}-{c[3]}" for c in E.SCORE_CASES + E.SEG_CASES])
def test_video_score_inputs_are_exact(n, rest, edge, branch):
    """The fp64 score rounded once equals the kernels' arithmetic (sequential fp32 sums, fp32 divides) bit for
    bit, and the case takes the branch it is listed for."""
    lg = E.score_logits(n, rest, edge)
    want, took = E.score_ref(lg)
    assert took == branch
    got = E.score_f32(lg)
    assert got.dtype == torch.float32 and want.dtype == torch.float32
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (float(got), float(want))
    if n > 2:
        p = E.sigmoid_f32(lg)
        assert set(p.unique().tolist()) <= {0.0, 0.5, 1.0}
        for base in range(0, n, E.PASS):                     # the ends of every pass differ from the rest
            last = min(base + E.PASS, n) - 1
            for c in range(2):
                assert rest[c] == edge[c] or (p[base, c] == edge[c] and p[last, c] == edge[c])


def test_video_score_cases_cover_the_issue_list():
    assert {c[0] for c in E.SCORE_CASES} == {0, 1, 2, 3, 4096, 4097, 8193}
    assert sorted(c[0] for c in E.SEG_CASES) == [0, 2, 3, 1024, 1025, 2049]
    for cases in (E.SCORE_CASES, E.SEG_CASES):
        assert {"f>r", "f<r", "f==r"} <= {c[3] for c in cases}
