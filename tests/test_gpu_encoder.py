"""The CViT encoder's row kernels (csrc/transformer.hip) on the GPU, one at a
time through the fac_debug_* entry points, against the fp64 references of
tests/encoder_ref.py: embed_finalize_ln (7, 14 and 28 slabs), resid_layernorm
and resid_cls (1, 2 and 4 slabs), attention2, head_out, and the two video-score
kernels across their LDS pass boundaries.

The gate of the 16-bit outputs is encoder_ref.compare16 (one 16-bit ulp of the
fp64 reference + F of the row maximum, at most 5 % of a case's outputs
different at all); test_encoder_ref.py shows on the CPU that honest fp32
arithmetic passes it and that each listed piece of wrong arithmetic does not.
Every output buffer carries sentinels on both sides that must survive.  Two
further tests check that the options "proj_splits" and "ffn_ln_eps_exp" reach
the kernels of a loaded tail.

Observed on an MI355X, over every case and both types: never more than one
16-bit value from the rounded reference, on at most 0.049 % of a case's
outputs; every residual sum and both score kernels bit-exact; head_out within
2.6e-4 of its bound.
"""
import ctypes

import numpy as np
import pytest
import torch

import encoder_ref as E
from fac_fake_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTS = ["bf16", "fp16"]
SENT = 77.0           # exactly representable in both 16-bit types and fp32
PAD = 1024            # sentinel elements on either side of an output: one whole row


@pytest.fixture(scope="module")
def ctxs(built_lib):
    """One bare context per 16-bit type (no weights, no workspace): the row-kernel entry points take only its
    type and device."""
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    lib = _lib.load()
    out = {}
    for dt in DTS:
        h = ctypes.c_void_p()
        _lib.check(lib.fac_create(0, _lib.DTYPES[dt], ctypes.byref(h)), None, "fac_create")
        out[dt] = h
    yield out
    torch.cuda.synchronize()
    for h in out.values():
        lib.fac_destroy(h)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(shape, dtype):
    n = int(np.prod(shape))
    buf = torch.full((PAD + n + PAD,), SENT, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n].view(*shape)


def _intact(buf):
    return bool((buf[:PAD] == SENT).all()) and bool((buf[-PAD:] == SENT).all())


def _dev(*ts):
    return [t.contiguous().to(DEV) for t in ts]


def _report(what, c):
    print(f"{what}: share {c['share']:.5f} max {c['max_ulps']:.2f} ulp excess {c['excess']:.3g}")
    assert c["ok"], (what, c)


# ---------------------------------------------------------------- resid_layernorm
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("S", E.RESID_S)
@pytest.mark.parametrize("R", [6, 2])
def test_resid_layernorm_vs_fp64(ctxs, R, S, dt):
    """x += sum of S slabs + bias, bit-equal to the exact sum (the six LayerNorm rows), then LayerNorm with eps
    1e-5, 1e-6 and 1e-2: the low-variance row (variance 4e-6) tells them apart by hundreds of ulps."""
    lib = _lib.load()
    i = E.resid_inputs(R, S)
    slab, bias, g, b = _dev(i["slab"], i["bias"], i["gamma"], i["beta"])
    for eps in E.RESID_EPS:
        x64, y64 = E.resid_ln_ref(i["x"], i["slab"], i["bias"], i["gamma"], i["beta"], eps)
        xbuf, x = _guarded((R, E.DIM), torch.float32)
        x.copy_(i["x"])
        ybuf, y = _guarded((R, E.DIM), E.T16[dt])
        rc = lib.fac_debug_resid_ln(ctxs[dt], x.data_ptr(), slab.data_ptr(), S, bias.data_ptr(), g.data_ptr(),
                                    b.data_ptr(), y.data_ptr(), R, eps, _stream())
        _lib.check(rc, ctxs[dt], "fac_debug_resid_ln")
        torch.cuda.synchronize()
        assert torch.equal(x.cpu().double(), x64)
        _report(f"resid_ln R{R} S{S} eps{eps:g} {dt}", E.compare16(y.cpu(), y64, dt))
        assert _intact(xbuf) and _intact(ybuf)
    assert torch.equal(slab.cpu(), i["slab"])                # read only


# ---------------------------------------------------------------- embed_finalize_ln
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("S", E.EMBED_S)
@pytest.mark.parametrize("B", [3, 1])
def test_embed_finalize_ln_vs_fp64(ctxs, B, S, dt):
    """Token rows from S slabs, bias, cls and the slot's pos row, then layer 0's LayerNorm (eps 1e-5), for slots
    in range, out of range on both sides (clamped to 0 / 31) and the clamped slots themselves: x exact on the CLS
    rows (one fp32 add) and within the (S + 2)-term fp32 bound on the patch rows, y by compare16; the
    out-of-range result equals the clamped one bit for bit."""
    lib = _lib.load()
    i = E.embed_inputs(B, S)
    host = (i["slab"], i["bias"], i["cls"], i["pos"])
    slab, bias, cls, pos, g, b = _dev(*host, i["gamma"], i["beta"])
    got = {}
    for which, pidx in E.PIDX[B].items():
        x64, y64 = E.embed_ref(*host, pidx, i["gamma"], i["beta"])
        p = torch.tensor(pidx, dtype=torch.int32, device=DEV)
        xbuf, x = _guarded((2 * B, E.DIM), torch.float32)
        ybuf, y = _guarded((2 * B, E.DIM), E.T16[dt])
        rc = lib.fac_debug_embed_ln(ctxs[dt], slab.data_ptr(), S, B, bias.data_ptr(), cls.data_ptr(), pos.data_ptr(),
                                    p.data_ptr(), x.data_ptr(), g.data_ptr(), b.data_ptr(), y.data_ptr(), _stream())
        _lib.check(rc, ctxs[dt], "fac_debug_embed_ln")
        torch.cuda.synchronize()
        xc, yc = x.cpu(), y.cpu()
        assert torch.equal(xc[0::2].double(), x64[0::2])
        xerr = (xc[1::2].double() - x64[1::2]).abs()
        assert bool((xerr <= E.embed_x_bound(i["slab"], i["bias"], i["pos"], pidx)).all())
        _report(f"embed_ln B{B} S{S} {which} {dt}", E.compare16(yc, y64, dt))
        assert _intact(xbuf) and _intact(ybuf)
        got[which] = (xc, yc)
    assert torch.equal(got["out_of_range"][0], got["clamped"][0])
    assert torch.equal(got["out_of_range"][1].view(torch.int16), got["clamped"][1].view(torch.int16))
    flags = ctypes.c_int(-1)                                 # the debug entry raises no pos_index flag
    assert lib.fac_check_device_errors(ctxs[dt], ctypes.byref(flags)) == 0 and flags.value == 0


# ---------------------------------------------------------------- resid_cls
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("S", E.RESID_S)
@pytest.mark.parametrize("B", [3, 1])
def test_resid_cls_vs_fp64(ctxs, B, S, dt):
    """CLS rows = x + S slabs + bias -> 16 bits with every patch row of x and of the slabs NaN: the sums are
    exact in fp32, so the result is the reference rounded once, bit for bit (compare16 holds a fortiori)."""
    lib = _lib.load()
    i = E.resid_cls_inputs(B, S)
    ref = E.resid_cls_ref(**i)
    x, slab, bias = _dev(i["x"], i["slab"], i["bias"])
    cbuf, c = _guarded((B, E.DIM), E.T16[dt])
    rc = lib.fac_debug_resid_cls(ctxs[dt], x.data_ptr(), slab.data_ptr(), S, bias.data_ptr(), c.data_ptr(), B,
                                 _stream())
    _lib.check(rc, ctxs[dt], "fac_debug_resid_cls")
    torch.cuda.synchronize()
    got = c.cpu()
    _report(f"resid_cls B{B} S{S} {dt}", E.compare16(got, ref, dt))
    assert torch.equal(got.view(torch.int16), E.round16(ref, dt).view(torch.int16))
    assert _intact(cbuf)


# ---------------------------------------------------------------- attention2
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B", [6, 1])
def test_attention_vs_fp64(ctxs, B, dt):
    """Two-token attention at scale 1 / 32 with logits up to 4, 17, 21, 58 and 93 (expf overflows past 88.7
    unless the row maximum is subtracted) and a crop with q = 0, whose two outputs are exactly the mean of its
    two v rows; B = 6 is 48 waves in 12 workgroups, B = 1 two workgroups."""
    lib = _lib.load()
    qkv = E.attention_inputs(B)
    ref = E.attention_ref(qkv)
    q, = _dev(qkv)
    obuf, o = _guarded((2 * B, E.DIM), E.T16[dt])
    rc = lib.fac_debug_attention(ctxs[dt], q.data_ptr(), o.data_ptr(), B, E.ATT_SCALE, _stream())
    _lib.check(rc, ctxs[dt], "fac_debug_attention")
    torch.cuda.synchronize()
    got = o.cpu()
    _report(f"attention B{B} {dt}", E.compare16(got, ref, dt))
    for b in range(B):                                       # per crop too: one wrong crop must not hide in six
        _report(f"attention B{B} crop {b} {dt}", E.compare16(got[2 * b:2 * b + 2], ref[2 * b:2 * b + 2], dt))
    if B == 6:
        want = E.round16(ref[10:12], dt)
        assert torch.equal(got[10:12].view(torch.int16), want.view(torch.int16))
    assert _intact(obuf) and torch.equal(q.cpu(), qkv)


# ---------------------------------------------------------------- head_out
@pytest.mark.parametrize("B,with_probs", [(1, False), (5, True), (5, False), (1, True)])
def test_head_out_vs_fp64(ctxs, B, with_probs):
    """Linear(2048, 2) + sigmoid on logits spread over +-30, within 2048 2^-24 sum |h w| of fp64 (+ 2^-22 on
    the probabilities); B = 5 is a partial last workgroup of four waves; probabilities optional."""
    lib = _lib.load()
    i = E.head_inputs(B)
    logits, probs, bound = E.head_ref(**i)
    hid, w2, b2 = _dev(i["hid"], i["w2"], i["b2"])
    lbuf, lg = _guarded((B, 2), torch.float32)
    pbuf, pr = _guarded((B, 2), torch.float32)
    rc = lib.fac_debug_head_out(ctxs["fp16"], hid.data_ptr(), w2.data_ptr(), b2.data_ptr(), lg.data_ptr(),
                                pr.data_ptr() if with_probs else None, B, _stream())
    _lib.check(rc, ctxs["fp16"], "fac_debug_head_out")
    torch.cuda.synchronize()
    err = (lg.cpu().double() - logits).abs()
    print(f"head_out B{B}: logits err/bound {float((err / bound).max()):.5f}")
    assert bool(torch.isfinite(lg).all()) and bool((err <= bound).all())
    if with_probs:
        perr = (pr.cpu().double() - probs).abs()
        print(f"head_out B{B}: probs err {float(perr.max()):.3g}")
        assert bool((perr <= bound + E.HEAD_SIGMOID_U).all())
        assert float(pr.max()) == 1.0 and 0 < float(pr.min()) < 1e-12
    else:
        assert bool((pr == SENT).all())
    assert _intact(lbuf) and _intact(pbuf)


# ---------------------------------------------------------------- video scores
def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("n,rest,edge,branch", E.SCORE_CASES, ids=[f"n{c[0]}-{c[3]}" for c in E.SCORE_CASES])
def test_video_score_exact(n, rest, edge, branch):
    """fac_video_score on logits whose fp32 sigmoids are exactly 0, 0.5 and 1, the first and last crop of every
    LDS pass holding the value the rest do not: the fp64 score rounded once, bit for bit, at n below, on and
    past one and two 4096-crop passes."""
    lib = _lib.load()
    lg = E.score_logits(n, rest, edge)
    want, took = E.score_ref(lg)
    assert took == branch
    d, = _dev(lg)
    sbuf, s = _guarded((1,), torch.float32)
    _lib.check(lib.fac_video_score(d.data_ptr() if n else None, n, s.data_ptr(), _stream()), None, "fac_video_score")
    torch.cuda.synchronize()
    assert int(_bits(s)[0]) == int(_bits(want.reshape(1))[0]), (float(s[0]), float(want))
    assert _intact(sbuf)


def test_video_score_seg_exact():
    """fac_video_score_seg over segments of 3, 0, 1024, 2, 1025 and 2049 crops in one call (1024-crop passes):
    each score is the fp64 value rounded once, bit for bit, and equals fac_video_score on the segment's own
    rows bit for bit."""
    lib = _lib.load()
    parts = [E.score_logits(n, rest, edge) for n, rest, edge, _ in E.SEG_CASES]
    seg = np.concatenate([[0], np.cumsum([c[0] for c in E.SEG_CASES])]).astype(np.int32)
    lg, = _dev(torch.cat(parts))
    dseg = torch.from_numpy(seg).to(DEV)
    nv = len(parts)
    sbuf, s = _guarded((nv,), torch.float32)
    _lib.check(lib.fac_video_score_seg(lg.data_ptr(), dseg.data_ptr(), nv, s.data_ptr(), _stream()), None,
               "fac_video_score_seg")
    one = torch.full((nv,), SENT, dtype=torch.float32, device=DEV)
    for v in range(nv):
        n = int(seg[v + 1] - seg[v])
        rows = lg[int(seg[v]):int(seg[v + 1])]
        _lib.check(lib.fac_video_score(rows.data_ptr() if n else None, n, one[v:].data_ptr(), _stream()), None,
                   "fac_video_score")
    torch.cuda.synchronize()
    for v, (n, rest, edge, branch) in enumerate(E.SEG_CASES):
        want, took = E.score_ref(parts[v])
        assert took == branch
        assert int(_bits(s)[v]) == int(_bits(want.reshape(1))[0]), (v, n, float(s[v]), float(want))
    assert torch.equal(_bits(s), _bits(one))
    assert _intact(sbuf)


# ---------------------------------------------------------------- argument checks (nothing is launched)
def test_debug_entry_argument_checks(ctxs):
    """A slab count the launcher has no instantiation for, a null pointer, B or R <= 0 and a null context give
    FAC_ERR_ARG (-1); d_probs alone may be null."""
    lib = _lib.load()
    c = ctxs["fp16"]
    t = torch.zeros(64 * E.DIM, device=DEV)                  # larger than anything a call wrongly launched would touch
    p = t.data_ptr()
    for S in (0, 1, 8, 13, 29):
        assert lib.fac_debug_embed_ln(c, p, S, 1, p, p, p, p, p, p, p, p, None) == -1, S
    for S in (0, 3, 5, 8):
        assert lib.fac_debug_resid_ln(c, p, p, S, p, p, p, p, 2, 1e-5, None) == -1, S
        assert lib.fac_debug_resid_cls(c, p, p, S, p, p, 1, None) == -1, S
    assert b"S must be" in lib.fac_last_error(c)
    for bad in (0, -1):
        assert lib.fac_debug_embed_ln(c, p, 14, bad, p, p, p, p, p, p, p, p, None) == -1
        assert lib.fac_debug_resid_ln(c, p, p, 4, p, p, p, p, bad, 1e-5, None) == -1
        assert lib.fac_debug_resid_cls(c, p, p, 4, p, p, bad, None) == -1
        assert lib.fac_debug_attention(c, p, p, bad, 0.03125, None) == -1
        assert lib.fac_debug_head_out(c, p, p, p, p, p, bad, None) == -1
    for k in range(9):                                        # each pointer of embed_ln in turn
        a = [p] * 9
        a[k] = None
        assert lib.fac_debug_embed_ln(c, a[0], 14, 1, *a[1:], None) == -1, k
    for k in range(6):
        a = [p] * 6
        a[k] = None
        assert lib.fac_debug_resid_ln(c, a[0], a[1], 4, *a[2:], 2, 1e-5, None) == -1, k
    for k in range(4):
        a = [p] * 4
        a[k] = None
        assert lib.fac_debug_resid_cls(c, a[0], a[1], 4, a[2], a[3], 1, None) == -1, k
        assert lib.fac_debug_head_out(c, *a, None, 1, None) == -1, k
    assert lib.fac_debug_attention(c, None, p, 1, 0.03125, None) == -1
    assert lib.fac_debug_attention(c, p, None, 1, 0.03125, None) == -1
    assert lib.fac_debug_resid_ln(c, p, p, 4, p, p, p, p, 2, 0.0, None) == -1      # eps must be positive
    assert lib.fac_debug_attention(None, p, p, 1, 0.03125, None) == -1
    assert lib.fac_debug_head_out(None, p, p, p, p, None, 1, None) == -1
    torch.cuda.synchronize()
    assert bool((t == 0).all())


# ---------------------------------------------------------------- options reach the kernels of a loaded tail
TAIL_B = 4
TAIL_SLOTS = np.array([0, 5, 31, 7])


@pytest.fixture(scope="module")
def tail(sd, built_lib, torch_threads):
    """A loaded fp16 tail-only context (patch embedding .. head of the synthetic state dict) and the oracle's
    stem output of 4 crops."""
    from fac_fake_amd.weights import make_crops
    from oracle.cvit_torch import forward_emulated, normalize_u8
    lib = _lib.load()
    h = ctypes.c_void_p()
    _lib.check(lib.fac_create(0, _lib.DTYPES["fp16"], ctypes.byref(h)), None, "fac_create")
    _lib.check(lib.fac_set_option(h, b"tail_only", 1), h, "fac_set_option")
    keep, descs = [], []
    for k, v in sd.items():
        if k.startswith("features."):
            continue
        t = torch.from_numpy(np.asarray(v)).float().contiguous()
        keep.append(t)
        d = _lib.TensorDesc()
        d.name, d.data, d.ndim = k.encode(), t.data_ptr(), t.dim()
        for j, s in enumerate(t.shape):
            d.shape[j] = s
        descs.append(d)
    arr = (_lib.TensorDesc * len(descs))(*descs)
    _lib.check(lib.fac_load_weights(h, ctypes.cast(arr, ctypes.c_void_p), len(descs)), h, "fac_load_weights")
    _, feats = forward_emulated(sd, normalize_u8(make_crops(TAIL_B, seed=11)), dtype="fp16", return_features=True)
    stem = feats[16]
    x = stem.permute(0, 2, 3, 1).contiguous().to(torch.float16).to(DEV)
    pidx = torch.from_numpy(TAIL_SLOTS.astype(np.int32)).to(DEV)

    def run():
        out = torch.empty(TAIL_B, 2, device=DEV)
        _lib.check(lib.fac_debug_tail(h, x.data_ptr(), TAIL_B, pidx.data_ptr(), out.data_ptr(), _stream()), h, "tail")
        torch.cuda.synchronize()
        return out.cpu()

    def option(key, value):
        _lib.check(lib.fac_set_option(h, key, value), h, "fac_set_option")

    yield {"run": run, "option": option, "stem": stem}
    torch.cuda.synchronize()
    lib.fac_destroy(h)


def _sig(t):
    return torch.sigmoid(t.double())


def _rms_rel(a, b):
    return float((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30))


def test_proj_splits_reach_the_kernels(tail, sd):
    """proj_splits 1, 2 and 4 (resid_layernorm / resid_cls on 1, 2 and 4 slabs inside the real tail): each stays
    inside test_tail_isolated's gates against the oracle, and the three differ from one another by no more than
    the summation order allows.  That bound is stated from the oracle: its emulated tail (fp32 sums, 16-bit
    rounding points -- the order of an fp32 sum flips 16-bit roundings downstream, which the pure fp32 tail
    cannot show) with the two projections summed as 1, 2 and 4 K ranges spreads the logits by 4e-4 .. 8e-4
    between splits on these inputs (the figure moves with the CPU's GEMM order); the gate is 4x the largest of the
    three pairwise spreads, computed here.  Observed on an MI355X: 3.8e-4 .. 4.5e-4 against a gate of 2.4e-3."""
    from oracle.cvit_torch import tail_emulated, tail_fp32
    em = {s: tail_emulated(sd, tail["stem"], TAIL_SLOTS, "fp16", proj_splits=s) for s in (1, 2, 4)}
    fp = tail_fp32(sd, tail["stem"], TAIL_SLOTS)
    spread = max(float((em[a] - em[b]).abs().max()) for a, b in ((1, 2), (1, 4), (2, 4)))
    got = {}
    try:
        for s in (1, 2, 4):
            tail["option"](b"proj_splits", s)
            got[s] = tail["run"]()
    finally:
        tail["option"](b"proj_splits", 4)
    for s in (1, 2, 4):
        d = float((got[s] - em[1]).abs().max())
        print(f"proj_splits {s}: gpu-emu {d:.3g}, rms rel vs fp32 {_rms_rel(got[s], fp):.3g} "
              f"(emu {_rms_rel(em[1], fp):.3g})")
        assert _rms_rel(got[s], fp) <= 1.5 * _rms_rel(em[1], fp) + 1e-4
        assert float((_sig(got[s]) - _sig(em[1])).abs().max()) <= 1e-3
    for a, b in ((1, 2), (1, 4), (2, 4)):
        d = float((got[a] - got[b]).abs().max())
        print(f"proj_splits {a} vs {b}: {d:.3g} (oracle spread {spread:.3g})")
        assert d <= 4 * spread
    assert torch.equal(tail["run"](), got[4])                # restored


def test_ffn_ln_eps_option_reaches_the_kernel(tail, sd):
    """ffn_ln_eps_exp 2 against 5: on these inputs the emulated logits move by d = 9e-3 .. 1e-2 between eps 1e-2
    and 1e-5, more than 8x the fp16 emulation's own distance from fp32 (8e-4; asserted), so the stem needs no
    scaling.  With the option at 2 the tail is within d / 4 of the 1e-2 emulation, at 5 within d / 4 of the 1e-5
    one.  Observed on an MI355X: 5.5e-4 and 1.0e-3 to its own emulation, 9.8e-3 and 9.4e-3 to the other."""
    from oracle.cvit_torch import tail_emulated, tail_fp32
    em = {n: tail_emulated(sd, tail["stem"], TAIL_SLOTS, "fp16", ff_eps=10.0 ** -n) for n in (2, 5)}
    fp = tail_fp32(sd, tail["stem"], TAIL_SLOTS)
    d = float((em[2] - em[5]).abs().max())
    noise = float((em[5] - fp).abs().max())
    print(f"d {d:.3g}, emulation vs fp32 {noise:.3g}")
    assert d >= 8 * noise
    got = {}
    try:
        for n in (2, 5):
            tail["option"](b"ffn_ln_eps_exp", n)
            got[n] = tail["run"]()
    finally:
        tail["option"](b"ffn_ln_eps_exp", 5)
    for n in (2, 5):
        near, far = float((got[n] - em[n]).abs().max()), float((got[n] - em[7 - n]).abs().max())
        print(f"ffn_ln_eps_exp {n}: to its own emulation {near:.3g}, to the other {far:.3g}")
        assert near <= d / 4
    assert torch.equal(tail["run"](), got[5])
