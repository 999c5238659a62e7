"""msca_S3D on the GPU: the msca.hip kernels against the fp64 restatement
(tests/msca_s3d_ref.py), and the model against outputs of the reference module
(tests/golden/msca_s3d_*, tools/make_golden_msca_s3d.py)."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import msca_s3d_ref as R  # noqa: E402
from fac_fake_amd.weights import make_msca_s3d_state_dict, s3d_clips, s3d_clips_varied  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T16 = {"fp16": torch.float16, "bf16": torch.bfloat16}

# (n, T, H, W, C, kt, k): the model's maps at 5 x 14^2 and 10 x 28^2, a 7-window
# on a 4 x 4 map with T < kt, one 16-byte column on an odd map, the Mlp's 1280
# channels (more than one block per position), and the 4 x 7^2 fixture map
DW_SHAPES = [(2, 5, 14, 14, 96, 3, 3), (2, 5, 14, 14, 160, 3, 7), (1, 10, 28, 28, 64, 1, 5), (2, 2, 4, 4, 48, 3, 7),
             (3, 1, 5, 9, 8, 3, 5), (1, 5, 14, 14, 1280, 3, 3), (2, 4, 7, 7, 224, 3, 5)]
ACTS = ["none", "affine2", "gelu"]
_ids = lambda s: "x".join(map(str, s))  # noqa: E731


def _ordered(t16):
    """16-bit floats as integers in value order: neighbours differ by 1."""
    i = t16.view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def _ulps(a16, b16):
    return int((_ordered(a16.cpu()) - _ordered(b16.cpu())).abs().max())


@functools.lru_cache(maxsize=None)
def _dw_case(shape, dt, act):
    """Input, weights and the fp64 / fp32 restatement, once per case.  The
    BatchNorm table puts pre-activations near N(2.5, 2.5^2): both ReLU6 cuts
    are hit."""
    n, t, h, w, c, kt, k = shape
    g = torch.Generator().manual_seed(100 * c + 10 * k + kt + n)
    x16 = torch.randn(n, t, h, w, c, generator=g).to(T16[dt])
    a = (3.0 / (k * k)) ** 0.5
    ws = (2 * torch.rand(c, 1, 1, k, k, generator=g) - 1) * a
    wt = (2 * torch.rand(c, 1, kt, 1, 1, generator=g) - 1) * (3.0 / kt) ** 0.5
    scale, shift = 2 + torch.rand(c, generator=g), 2 + torch.rand(c, generator=g)
    scale2, shift2 = (0.5 + torch.rand(c, generator=g), torch.rand(c, generator=g) - 0.5) if act == "affine2" else (None, None)
    wts = (ws, wt, scale, shift, act, scale2, shift2)
    ref64 = R.dwsep_cl(x16.double(), *wts)
    ref32 = R.dwsep_cl(x16.float(), *wts)
    return x16, wts, ref64, ref32


def _dw_layer(wts, dt):
    from fac_fake_amd.ops import DWSepLayer
    ws, wt, scale, shift, act, scale2, shift2 = wts
    return DWSepLayer(ws, wt, scale, shift, act=act, scale2=scale2, shift2=shift2, dtype=dt, device=DEV)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", DW_SHAPES, ids=_ids)
def test_dwsep3d_parity(shape, dt, act):
    """The kernel's fp32 value within 4 E of the fp64 restatement, E = the fp32
    torch restatement's own distance from fp64 on the same inputs + 1e-6 rms;
    the stored 16-bit output bit-equal to the rounding of that fp32 value."""
    x16, wts, ref64, ref32 = _dw_case(shape, dt, act)
    rms = float(ref64.pow(2).mean().sqrt())
    E = float((ref32.double() - ref64).abs().max()) + 1e-6 * rms
    layer, x = _dw_layer(wts, dt), x16.to(DEV)
    v32 = layer(x, out_f32=True)
    out = layer(x)
    torch.cuda.synchronize()
    err = float((v32.double().cpu() - ref64).abs().max())
    print(f"dwsep3d {shape} {dt} {act}: |v - fp64| {err:.3e}  E {E:.3e}  rms {rms:.3e}")
    assert torch.equal(x.cpu(), x16), "the input was written"
    assert err <= 4 * E, (err, E)
    assert torch.equal(out.view(torch.int16), v32.to(T16[dt]).view(torch.int16))
    if act == "none":   # both cuts of the ReLU6 are exercised
        assert float((ref64 == 6).double().mean()) > 0.002 and float((ref64 == 0).double().mean()) > 0.002


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", [DW_SHAPES[0], DW_SHAPES[3], DW_SHAPES[4]], ids=_ids)
def test_dwsep3d_slices(shape, dt):
    """Channels [c0, c0 + C) of a wider tensor in, an offset slot of a wider
    tensor out: bit-equal to the contiguous run, the other channels of out
    untouched, the input never written."""
    n, t, h, w, c, _, _ = shape
    x16, wts, _, _ = _dw_case(shape, dt, "affine2")
    layer = _dw_layer(wts, dt)
    want = layer(x16.to(DEV))
    wide = torch.full((n, t, h, w, c + 24), float("nan"), dtype=T16[dt])
    wide[..., 16:16 + c] = x16
    wide_d = wide.to(DEV)
    sentinel = 0x5A5A
    obuf = torch.full((n, t, h, w, c + 40), sentinel, dtype=torch.int16, device=DEV)
    layer(wide_d, c_in_off=16, out=obuf.view(T16[dt]), c_off=8)
    torch.cuda.synchronize()
    assert torch.equal(obuf[..., 8:8 + c], want.view(torch.int16))
    assert bool((obuf[..., :8] == sentinel).all()) and bool((obuf[..., 8 + c:] == sentinel).all())
    assert torch.equal(wide_d.view(torch.int16).cpu(), wide.view(torch.int16))


def _ew_inputs(shape, dt, seed):
    g = torch.Generator().manual_seed(seed)
    return [(3 * torch.randn(*shape, generator=g) + 1.5).to(T16[dt]) for _ in range(3)]


EW_ARITY = {"gelu": 1, "clamp6": 1, "mul": 2, "add": 2, "add_gelu": 2, "add3": 3, "affine": 1}


@pytest.mark.parametrize("op", sorted(EW_ARITY))
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_ew_ops(op, dt):
    """Every element-wise op within one 16-bit ulp of the rounded fp64 value
    (one fp32 evaluation, one rounding).  The two GELU ops are held to the 4 E
    rule instead (E: fp32 torch's distance from fp64 on the same inputs + 1e-6
    rms), plus the half ulp of the one 16-bit rounding: in GELU's negative tail
    1 + erf(x / sqrt 2) cancels in fp32, for torch as for the kernel, and an
    ulp count of values near 1e-7 says nothing.  With offsets into wider tensors
    bit-equal to the contiguous run, the rest of out untouched; in place equal
    to out of place; clip k alone bit-equal to clip k of the batch of 3."""
    from fac_fake_amd import ops
    shape, c = (3, 2, 5, 7, 48), 48
    ins = _ew_inputs(shape, dt, 7)[:EW_ARITY[op]]
    g = torch.Generator().manual_seed(11)
    kw = {}
    if op == "affine":
        sc, sh = torch.rand(c, generator=g) * 2 - 1, torch.randn(c, generator=g)
        kw = dict(scale=sc.to(DEV), shift=sh.to(DEV))
        ref = ins[0].double() * sc.double() + sh.double()
    else:
        ref = R.EW[op](*[t.double() for t in ins])
    dins = [t.to(DEV) for t in ins]
    out = ops.ew(op, *dins, **kw)
    torch.cuda.synchronize()
    if "gelu" in op:
        ref32 = R.EW[op](*[t.float() for t in ins]).double()
        E = float((ref32 - ref).abs().max()) + 1e-6 * float(ref.pow(2).mean().sqrt())
        half_ulp = ref.abs() * 2.0 ** (-11 if dt == "fp16" else -8) + 2.0 ** (-25 if dt == "fp16" else -134)
        assert bool(((out.double().cpu() - ref).abs() <= 4 * E + half_ulp).all()), E
    else:
        assert _ulps(out, ref.to(T16[dt])) <= 1
    assert float((out.double().cpu() - ref).abs().max()) <= 2.0 ** (-10 if dt == "fp16" else -7) * float(ref.abs().max())
    # offsets
    wides = []
    for k, t in enumerate(ins):
        wd = torch.full(shape[:-1] + (c + 16 + 8 * k,), float("nan"), dtype=T16[dt])
        wd[..., 8 * (k + 1):8 * (k + 1) + c] = t
        wides.append(wd.to(DEV))
    obuf = torch.full(shape[:-1] + (c + 24,), 0x5A5A, dtype=torch.int16, device=DEV)
    offs = dict(zip(("a_off", "b_off", "c3_off"), (8, 16, 24)))
    ops.ew(op, *wides, c=c, out=obuf.view(T16[dt]), o_off=16, **{k: v for k, v in offs.items() if k[0] in "abc"[:len(ins)]}, **kw)
    torch.cuda.synchronize()
    assert torch.equal(obuf[..., 16:16 + c], out.view(torch.int16))
    assert bool((obuf[..., :16] == 0x5A5A).all()) and bool((obuf[..., 16 + c:] == 0x5A5A).all())
    # in place, and one clip alone
    a = dins[0].clone()
    assert ops.ew(op, a, *dins[1:], out=a, **kw) is a
    one = ops.ew(op, *[t[1:2].contiguous() for t in dins], **kw)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int16), out.view(torch.int16))
    assert torch.equal(one[0].view(torch.int16), out[1].view(torch.int16))
    for t, t0 in zip(dins[1:], ins[1:]):
        assert torch.equal(t.cpu().view(torch.int16), t0.view(torch.int16))


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", [(2, 5, 14, 14, 96, 3), (3, 1, 5, 9, 8, 3), (2, 4, 7, 7, 48, 1), (3, 2, 3, 3, 64, 3)], ids=_ids)
def test_bn_max_pool(shape, dt):
    """The sliced BatchNorm + MaxPool3d((kt,3,3)) with scales of both signs
    (where the BatchNorm does not commute with the max): within one 16-bit ulp
    of the rounded fp64 value; the slice of a wider tensor into an offset slot
    bit-equal; clip k alone bit-equal."""
    from fac_fake_amd import ops
    n, t, h, w, c, kt = shape
    g = torch.Generator().manual_seed(c + kt)
    x16 = torch.randn(n, t, h, w, c + 16, generator=g).to(T16[dt])
    scale, shift = torch.randn(c, generator=g), torch.randn(c, generator=g)
    assert bool((scale < 0).any()) and bool((scale > 0).any())
    ref = R.bn_pool_cl(x16[..., 8:8 + c].double(), scale.double(), shift.double(), kt)
    x = x16.to(DEV)
    sd, sh = scale.to(DEV), shift.to(DEV)
    obuf = torch.full((n, t, h, w, c + 8), 0x5A5A, dtype=torch.int16, device=DEV)
    ops.bn_max_pool(x, sd, sh, kt, c_in_off=8, c=c, out=obuf.view(T16[dt]), c_off=8)
    got = ops.bn_max_pool(x[..., 8:8 + c].contiguous(), sd, sh, kt)
    one = ops.bn_max_pool(x[n - 1:], sd, sh, kt, c_in_off=8, c=c)
    torch.cuda.synchronize()
    assert _ulps(got, ref.to(T16[dt])) <= 1
    assert torch.equal(obuf[..., 8:], got.view(torch.int16)) and bool((obuf[..., :8] == 0x5A5A).all())
    assert torch.equal(one[0].view(torch.int16), got[n - 1].view(torch.int16))
    assert torch.equal(x.cpu().view(torch.int16), x16.view(torch.int16))


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_msca_sum_and_batch_independence(dt):
    """ops.msca_sum is, bit for bit, its unfused parts (two fac_dwsep3d
    launches, one 'add3'); its value is within 4 E + the three roundings of
    the fp64 restatement; a clip alone is bit-equal to the clip in a batch of
    3, for fac_dwsep3d and for the sum."""
    from fac_fake_amd import ops
    n, t, h, w, c = 3, 4, 7, 7, 128
    x16, w5, _, _ = _dw_case((n, t, h, w, c, 3, 5), dt, "none")
    w7 = _dw_case((n, t, h, w, c, 3, 7), dt, "none")[1]
    a16 = x16.clamp(0, 6)     # the sum's first term is a ReLU6 output in the model
    r5_64, r7_64 = R.dwsep_cl(a16.double(), *w5), R.dwsep_cl(a16.double(), *w7)
    r5_32, r7_32 = R.dwsep_cl(a16.float(), *w5), R.dwsep_cl(a16.float(), *w7)
    L5, L7 = _dw_layer(w5, dt), _dw_layer(w7, dt)
    a = a16.to(DEV)
    s = ops.msca_sum(a, L5, L7)
    t5, t7 = L5(a), L7(a)
    parts = ops.ew("add3", a, t5, t7)
    torch.cuda.synchronize()
    assert torch.equal(s.view(torch.int16), parts.view(torch.int16))
    ref = (a16.double() + r5_64) + r7_64
    E = float((r5_32.double() - r5_64).abs().max() + (r7_32.double() - r7_64).abs().max()) + 1e-6 * float(ref.pow(2).mean().sqrt())
    u = 2.0 ** (-11 if dt == "fp16" else -8)          # half an ulp, relative
    bound = 4 * E + u * (6 + 6 + 18)                  # roundings of t5, t7 (<= 6) and of the sum (<= 18)
    err = float((s.double().cpu() - ref).abs().max())
    print(f"msca_sum {dt}: err {err:.3e} bound {bound:.3e}")
    assert err <= bound, (err, bound)
    for k in range(n):
        ak = a[k:k + 1].contiguous()
        s1, d1 = ops.msca_sum(ak, L5, L7), L7(ak)
        torch.cuda.synchronize()
        assert torch.equal(s1[0].view(torch.int16), s[k].view(torch.int16)), k
        assert torch.equal(d1[0].view(torch.int16), t7[k].view(torch.int16)), k


def test_wrappers_name_the_constraint():
    from fac_fake_amd import ops
    x = torch.zeros(1, 2, 4, 4, 16, dtype=torch.float16, device=DEV)
    with pytest.raises(ValueError, match="multiples of 8"):
        ops.ew("gelu", x, a_off=4, c=8)
    with pytest.raises(ValueError, match="op must be one of"):
        ops.ew("tanh", x)
    with pytest.raises(ValueError, match="takes 1 operand"):
        ops.ew("add", x)
    with pytest.raises(ValueError, match="16-byte"):
        ops.ew("gelu", torch.zeros(8 + 2 * 4 * 4 * 16, dtype=torch.float16, device=DEV)[8 - 4:-4].view(1, 2, 4, 4, 16))
    with pytest.raises(ValueError, match="kt must be 1 or 3"):
        ops.bn_max_pool(x, torch.ones(16, device=DEV), torch.zeros(16, device=DEV), 2)
    with pytest.raises(ValueError, match="k must be 3, 5 or 7"):
        ops.DWSepLayer(torch.zeros(8, 1, 1, 9, 9), torch.zeros(8, 1, 3, 1, 1), torch.ones(8), torch.zeros(8), dtype="fp16", device=DEV)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.DWSepLayer(torch.zeros(12, 1, 1, 3, 3), torch.zeros(12, 1, 3, 1, 1), torch.ones(12), torch.zeros(12), dtype="fp16", device=DEV)
    with pytest.raises(ValueError, match="affine2"):
        ops.DWSepLayer(torch.zeros(8, 1, 1, 3, 3), torch.zeros(8, 1, 3, 1, 1), torch.ones(8), torch.zeros(8), act="affine2", dtype="fp16", device=DEV)


def test_dwsep3d_abi_errors():
    """Bad k, kt, c -> FAC_ERR_SHAPE; null or misaligned pointers, a slice
    outside its row, a bad act or op -> FAC_ERR_ARG; nothing is launched."""
    import ctypes
    from fac_fake_amd import _lib, ops
    lib = _lib.load()
    c = 16
    x = torch.zeros(1, 2, 4, 4, c, dtype=torch.float16, device=DEV)
    out = torch.full((1, 2, 4, 4, c), 3.0, dtype=torch.float16, device=DEV)
    tab = torch.ones(49 * c, dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(**kw):
        d = ops.DWSepDesc()
        d.dtype, d.inp, d.ldi, d.i_off = 1, x.data_ptr(), c, 0
        d.n, d.t, d.h, d.w, d.c, d.kt, d.k = 1, 2, 4, 4, c, 3, 3
        d.ws = d.wt = d.scale = d.shift = tab.data_ptr()
        d.out, d.ldo, d.o_off = out.data_ptr(), c, 0
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.fac_dwsep3d(ctypes.byref(d), st)
    SHAPE, ARG = -2, -1
    assert call(k=4) == SHAPE and call(kt=2) == SHAPE and call(c=12) == SHAPE and call(n=0) == SHAPE
    assert call(inp=None) == ARG and call(ws=None) == ARG and call(wt=None) == ARG and call(act=3) == ARG
    assert call(act=1) == ARG                                  # affine2 without its tables
    assert call(i_off=8) == ARG and call(o_off=4) == ARG and call(inp=x.data_ptr() + 8) == ARG
    assert lib.fac_ew(1, 9, x.data_ptr(), c, 0, None, 0, 0, None, 0, 0, None, None, out.data_ptr(), c, 0, 32, c, st) == ARG
    assert lib.fac_ew(1, 3, x.data_ptr(), c, 0, None, 0, 0, None, 0, 0, None, None, out.data_ptr(), c, 0, 32, c, st) == ARG
    assert lib.fac_bn_maxpool3d(1, x.data_ptr(), c, 0, 1, 2, 4, 4, c, 5, tab.data_ptr(), tab.data_ptr(), out.data_ptr(), c, 0, st) == SHAPE
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out == 3.0).all())


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_relu6_by_clamp_equals_one_epilogue(dt):
    """fac_conv_nd is launched as before (this model adds no flag to it: the
    launch is the legacy wrapper's); its ReLU6 is the conv's ReLU, then
    ops.clamp6_ in place.  On three S3D layer shapes: the clamp leaves exactly
    min(legacy, 6), with a share of the legacy outputs above 6 (rounding is
    monotonic and 6 is a 16-bit value, so this is round16(min(max(v, 0), 6)):
    test_msca_s3d.py checks that identity)."""
    from fac_fake_amd import ops
    g = torch.Generator().manual_seed(3)
    for (cin, cout, k, pad, shape) in [(64, 64, (1, 1, 1), 0, (2, 4, 14, 14)), (96, 208, (1, 3, 3), (0, 1, 1), (2, 4, 7, 7)),
                                       (208, 208, (3, 1, 1), (1, 0, 0), (1, 4, 7, 7))]:
        w = torch.randn(cout, cin, *k, generator=g) * (6.0 / (cin * k[0] * k[1] * k[2])) ** 0.5
        b = 2 + torch.rand(cout, generator=g)
        layer = ops.ConvLayer(w, b, 1, pad, dtype=dt, device=DEV)
        x = (1.5 * torch.randn(*shape, cin, generator=g)).to(T16[dt]).to(DEV)
        legacy = layer(x)
        keep = legacy.clone()
        got = ops.clamp6_(legacy)
        torch.cuda.synchronize()
        assert got is legacy and float((keep > 6).float().mean()) > 0.01 and float((keep == 0).float().mean()) > 0.01
        assert torch.equal(got.view(torch.int16), keep.float().clamp(max=6).to(T16[dt]).view(torch.int16))


# ---------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def models():
    from fac_fake_amd.msca_s3d import msca_S3D
    out = {}
    for srm in ("no", "yes"):
        sd = {k: torch.from_numpy(np.asarray(v)) for k, v in make_msca_s3d_state_dict(0, 1, srm == "yes").items()}
        for dt in ("fp16", "bf16"):
            m = msca_S3D(1, srm, dtype=dt)
            m.load_state_dict(sd)
            out[(srm, dt)] = m
    return out


@pytest.fixture(scope="module")
def block_clips(golden):
    g = R.load_blocks(golden)
    return g, torch.from_numpy(s3d_clips_varied(int(g["n_clips"]), 16, 112, int(g["clip_seed"]))).to(DEV)


def _rel_to_rms(got, ref):
    return float(np.abs(got - ref).max() / (np.sqrt((ref.astype(np.float64) ** 2).mean()) + 1e-30))


def _check_logits(g, gb, lg, pr, srm, dt, what):
    """Logits within 2x the recorded logit envelope; fp16 probabilities within
    1e-3 where the recorded fp16 probability envelope is below 5e-4 (else the
    logit bound alone stands).  The envelope is the larger of fixture `g`'s
    and the 4-clip fixture `gb`'s for the same model and dtype, as
    ca_s3d_ref.logit_gate takes it: one clip samples the rounding envelope
    poorly (the harness-shape clip's recorded fp16 envelope with SRM is
    7e-6, where the emulation happened to land on the reference; the 4-clip
    one is 1e-3)."""
    dl = float(np.abs(lg.double().cpu().numpy() - g[f"logits_{srm}"]).max())
    gate = 2 * max(float(g[f"env_logit_{srm}_{dt}"]), float(gb[f"env_logit_{srm}_{dt}"]))
    p_ref = 1 / (1 + np.exp(-g[f"logits_{srm}"].astype(np.float64)))
    dp = float(np.abs(pr.double().cpu().numpy() - p_ref).max())
    print(f"msca_s3d {what} {srm} {dt}: |dlogit| {dl:.3e} gate {gate:.3e}  |dp| {dp:.3e} "
          f"env_prob {float(g[f'env_prob_{srm}_{dt}']):.3e}")
    assert dl <= gate, (dl, gate)
    if dt == "fp16" and float(g[f"env_prob_{srm}_fp16"]) < 5e-4:
        assert dp <= 1e-3, dp


@pytest.mark.parametrize("srm", ["no", "yes"])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_msca_s3d_every_block_matches_reference(models, block_clips, srm, dt):
    """4 content-varied clips of 16 x 112^2: the per-channel means of all 21
    base[i] outputs and of the 18 inceptionmixer / mlp outputs within 2 env +
    1e-4 of the reference module's (relative to the rms of its means; env: the
    recorded 16-bit rounding envelope, the factor 2 for the kernels' summation
    order); logits within 2x the logit envelope."""
    g, x = block_clips
    m = models[(srm, dt)]
    taps, extra = m.base_outputs(x), m.block_outputs(x)
    torch.cuda.synchronize()
    assert len(taps) == 21 and len(extra) == 18
    for name, ts, env in (("mean", taps, g[f"env_{srm}_{dt}"]), ("xmean", extra, g[f"xenv_{srm}_{dt}"])):
        for i, t in enumerate(ts):
            got = t.float().mean(dim=(1, 2, 3)).double().cpu().numpy()
            ref = g[f"{name}_{srm}_{i}"].astype(np.float64)
            assert got.shape == ref.shape, (name, i, got.shape, ref.shape)
            err = _rel_to_rms(got, ref)
            print(f"msca_s3d {srm} {dt} {name} {i}: err {err:.3e} gate {2 * env[i] + 1e-4:.3e}")
            assert err <= 2 * env[i] + 1e-4, (name, i, err, env[i])
    lg, pr = m(x, return_probs=True)
    torch.cuda.synchronize()
    _check_logits(g, g, lg, pr, srm, dt, "16x112")


@pytest.mark.parametrize("srm", ["no", "yes"])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_msca_s3d_reference_harness_shape(models, golden, srm, dt):
    g = golden("msca_s3d_golden_20x224.npz")
    x = torch.from_numpy(s3d_clips_varied(1, int(g["frames"]), int(g["size"]), seed=int(g["clip_seed"]))).to(DEV)
    lg, pr = models[(srm, dt)](x, return_probs=True)
    torch.cuda.synchronize()
    assert lg.shape == (1, 1)
    _check_logits(g, R.load_blocks(golden), lg, pr, srm, dt, "20x224")


@pytest.mark.parametrize("srm", ["no", "yes"])
def test_msca_s3d_batch_independence_and_uint8(models, block_clips, srm):
    """Clip k alone is bit-equal to clip k in a batch of 3; a uint8 clip gives
    the logits of its float copy (the fused uint8 base.0 launch has no 6-clamp
    and is not taken by this model)."""
    _, x = block_clips
    m = models[(srm, "fp16")]
    lg = m(x[:3])
    for k in range(3):
        one = m(x[k:k + 1])
        torch.cuda.synchronize()
        assert torch.equal(one[0], lg[k]), k
    lg8 = m(x[:3].to(torch.uint8))
    torch.cuda.synchronize()
    assert torch.isfinite(lg).all() and torch.equal(lg8, lg)


def test_msca_s3d_graph_replay_matches_eager(models):
    m = models[("no", "fp16")]
    x = torch.from_numpy(s3d_clips(2, 16, 112, seed=5)).to(DEV)
    eager = m(x).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m(x)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            out = m(x)
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_msca_s3d_video_predictions(models, block_clips):
    from fac_fake_amd.s3d import video_predictions
    _, x = block_clips
    m = models[("no", "fp16")]
    preds = video_predictions(m, x, batch=3)
    lg = m(x)
    torch.cuda.synchronize()
    want = torch.sigmoid(lg.double().cpu())[:, 0].numpy()
    assert len(preds) == x.shape[0] and np.abs(np.array(preds) - want).max() <= 1e-6


def test_msca_s3d_refuses_cpu_and_training(models):
    m = models[("no", "fp16")]
    with pytest.raises(RuntimeError):
        m.train(True)
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 16, 112, 112))
