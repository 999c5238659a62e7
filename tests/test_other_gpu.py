"""The model/other/ CViTs on the GPU: fac_smfa (smfa.hip) against a float64
reference of its own arithmetic (tests/smfa_ref.py), and the four drop-ins of
fac_fake_amd/other.py against the reference classes' recorded outputs
(tests/golden/other_*, tools/make_golden_other.py).
"""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import smfa_ref as R  # noqa: E402
from fac_fake_amd import _lib  # noqa: E402
from fac_fake_amd.weights import make_crops, make_other_state_dict  # noqa: E402
from oracle.cvit_torch import normalize_u8  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
MANT = {"fp16": 10, "bf16": 7}
# |got - ref| / max(|ref|, 1e-3): twice the half-ulp of the one output rounding (KERNEL_BOUND of test_dconv_gpu.py)
KERNEL_BOUND = {"fp16": 2 ** -10 + 1e-5, "bf16": 2 ** -7 + 1e-5}
# (n, h, w, c): the smallest legal map and width; odd, non-square, 135 rows per crop; the model's shape, whose 980
# rows make the 32-row wave tiles straddle crops and leave the last one partly empty; a single crop.
SHAPES = [(2, 8, 8, 64), (3, 9, 15, 128), (5, 14, 14, 256), (1, 14, 14, 256)]
SID = lambda s: "x".join(map(str, s))  # noqa: E731
SHAPE_ERR, ARG_ERR = -2, -1


def _signed(g, *s, lo, hi):
    """Magnitudes in [lo, hi) with a random sign."""
    return (torch.rand(*s, generator=g) * (hi - lo) + lo) * torch.where(torch.rand(*s, generator=g) < 0.5, -1.0, 1.0)


@functools.lru_cache(maxsize=None)
def _operands(c, dt, x_identity=False, belt=(0.5, 1.5)):
    """Random fac_smfa_pack operands (fp32; the three MFMA weights already on
    the 16-bit grid, so the float64 reference and the kernel use the same
    values): linear_0's bias non-zero, alpha and belt non-zero with both signs.
    x_identity: the x half of linear_0 is the identity with bias 0, so the
    statistics' input is the test's input exactly."""
    g = torch.Generator().manual_seed(900 + c)
    u = lambda *s, a=1.0: (torch.rand(*s, generator=g) * 2 - 1) * a  # noqa: E731
    ops = dict(w0=u(2 * c, c, a=(3.0 / c) ** 0.5), b0=u(2 * c, a=0.5),
               gate4=torch.stack([_signed(g, c, lo=0.5, hi=1.5), u(c), u(c, a=0.3), _signed(g, c, lo=belt[0], hi=belt[1])]),
               w1=u(c, c, a=1.5 * (3.0 / c) ** 0.5), b1=u(c, a=0.3), dww=u(2 * c, 9, a=0.6), dwb=u(2 * c, a=0.3),
               wpw=u(2 * c, 2 * c, a=(1.5 / c) ** 0.5), bpw=u(2 * c, a=0.3), wcat=u(c, 3 * c, a=(1.0 / c) ** 0.5),
               bcat=u(c, a=0.3))
    if x_identity:
        ops["w0"][c:] = torch.eye(c)
        ops["b0"][c:] = 0
    for k in ("w0", "wpw", "wcat"):
        ops[k] = R.round_to(ops[k], dt)
    return ops


@functools.lru_cache(maxsize=None)
def _input(shape, dt):
    """Signed, every seventh channel all-negative; NHWC 16-bit."""
    n, h, w, c = shape
    g = torch.Generator().manual_seed(17 + h * w + c)
    x = torch.randn(n, h, w, c, generator=g) * 1.5
    x[..., ::7] = -x[..., ::7].abs() - 0.25
    return x.to(T16[dt])


def _nchw(x16, dtype):
    return x16.to(dtype).permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def _reference(shape, dt, residual):
    """(float64 reference, the CPU emulation of the kernel's rounding points), NHWC, from the 16-bit inputs."""
    x, ops = _input(shape, dt), _operands(shape[3], dt)
    with torch.no_grad():
        ref = R.smfa_block(_nchw(x, torch.float64), ops, bool(residual))
        emu = R.smfa_block(_nchw(x, torch.float32), ops, bool(residual), dtype=torch.float32, round=dt)
    return ref.permute(0, 2, 3, 1).contiguous(), emu.double().permute(0, 2, 3, 1).contiguous()


_PACKED = {}


def _packed(ops, dt):
    from fac_fake_amd import other
    key = (id(ops), dt)
    if key not in _PACKED:
        _PACKED[key] = (ops, other.smfa_pack(ops, dt, DEV))      # keeps ops alive: id() stays unique
    return _PACKED[key][1]


def _run(x16, ops, residual, dt, shape=None, gate=False, out=None, scratch=None, wpk=None, dtype_id=None):
    """fac_smfa on a device tensor [n,h,w,c]; returns (status, out, gate_out)."""
    lib = _lib.load()
    n, h, w, c = shape or x16.shape
    if wpk is None:
        wpk = _packed(ops, dt)
    if out is None:
        out = torch.empty(x16.shape, dtype=x16.dtype, device=DEV)
    if scratch is None:
        scratch = torch.empty(max(lib.fac_smfa_scratch_bytes(*x16.shape), 16), dtype=torch.uint8, device=DEV)
    g = torch.full((x16.shape[0], x16.shape[3]), float("nan"), dtype=torch.float32, device=DEV) if gate else None
    rc = lib.fac_smfa(_lib.DTYPES[dt] if dtype_id is None else dtype_id, x16.data_ptr(), n, h, w, c, wpk.data_ptr(),
                      int(residual), out.data_ptr(), g.data_ptr() if gate else None, scratch.data_ptr(),
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out, g


def _rule1(got, ref, emu, dt):
    """The block rule: the GPU's error against the float64 reference measured
    by the CPU emulation's own error against it.  Returns (relative L2 ratio,
    max|d| ratio), each against its allowance: 2x / 4x the emulation's figure,
    never tighter than twice the half-ulp of the output rounding."""
    e_gpu, e_emu = got.double() - ref, emu - ref
    l2_allow = max(2 * float(e_emu.norm() / ref.norm()), KERNEL_BOUND[dt])
    mx_allow = max(4 * float(e_emu.abs().max()), KERNEL_BOUND[dt] * float(ref.abs().max()))
    return float(e_gpu.norm() / ref.norm()) / l2_allow, float(e_gpu.abs().max()) / mx_allow


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("residual", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_smfa_vs_float64_reference(shape, residual, dt):
    """SMFA(x) and x + SMFA(x) against smfa_block(float64) on the same 16-bit
    inputs and weights.  The yardstick is the CPU emulation of the five
    rounding points (smfa_block(round=dt)): relative L2 within 2x its error,
    max|d| within 4x (fp32 summation order flips 16-bit roundings at the five
    points, and the extreme value is the noisier statistic).
    Measured on an MI355X over the 16 cases: the relative L2 error is
    0.75-0.84x the emulation's (0.37-0.42 of the allowance) and max|d| equals
    the emulation's in every case (0.25 of the allowance): the largest error
    is the same 16-bit rounding in both."""
    x = _input(shape, dt)
    rc, got, _ = _run(x.to(DEV), _operands(shape[3], dt), residual, dt)
    assert rc == 0
    ref, emu = _reference(shape, dt, residual)
    assert got.shape == ref.shape
    l2, mx = _rule1(got.cpu(), ref, emu, dt)
    print(f"{shape} residual {residual} {dt}: relative L2 at {l2:.3f} of its allowance, max|d| at {mx:.3f}")
    assert torch.isfinite(got.float()).all()
    assert l2 <= 1 and mx <= 1, (shape, residual, dt, l2, mx)


def _gate_reference(x16, ops):
    """With the identity x half: g, u's parts and the summation bounds in float64 from the input itself."""
    n, h, w, c = x16.shape
    N = h * w
    xx = x16.double().reshape(n, N, c)
    alpha, cw, cb, belt = ops["gate4"].double()
    mx, var = xx.amax(1), xx.var(1, unbiased=True)
    u = alpha * (cw * mx + cb) + belt * var
    w1 = ops["w1"].double()
    pre = u @ w1.t() + ops["b1"].double()
    g = torch.nn.functional.gelu(pre)
    # fp32 summation bounds: N 2^-24 sum |t_i| with t_i = (x_i - mean)^2 / (N - 1) for the variance (the sum is
    # the variance itself), carried through belt and |W1|; c 2^-24 sum |W1 u| for the GEMV; |GELU'| <= 1.13
    u_b = belt.abs() * (N * 2.0 ** -24 * var)
    pre_b = u_b @ w1.abs().t() + c * 2.0 ** -24 * (u.abs() @ w1.abs().t())
    # the same formula in torch fp32: the project's CPU yardstick
    x32 = x16.float().reshape(n, N, c)
    a32, cw32, cb32, b32 = ops["gate4"]
    u32 = a32 * (cw32 * x32.amax(1) + cb32) + b32 * x32.var(1, unbiased=True)
    g32 = torch.nn.functional.gelu(u32 @ ops["w1"].t() + ops["b1"])
    return g, 1.13 * pre_b, float((g32.double() - g).abs().max())


def _far_mean_input(shape, dt):
    """Channel means of +-8 with standard deviation 0.05: what a one-pass sum x^2 - (sum x)^2 / N cancels on."""
    n, h, w, c = shape
    g = torch.Generator().manual_seed(77)
    mean = torch.where(torch.arange(c) % 2 == 0, 8.0, -8.0)
    return (mean + 0.05 * torch.randn(n, h, w, c, generator=g)).to(T16[dt])


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("case", ["2x8x8x64", "3x9x15x128", "5x14x14x256", "1x14x14x256", "far-mean"])
def test_gate_vs_float64_reference(case, dt):
    """g through gate_out, with linear_0's x half the identity so that the
    statistics see the test's input.  |g - g64| within the larger of 4x the
    fp32 CPU yardstick (the same formula in torch fp32 against float64) and the
    fp32 summation bound of the variance and the GEMV (_gate_reference).  The
    far-mean case (means +-8, standard deviation 0.05, belt +-[50, 150]) is
    the one a one-pass variance fails.  residual does not enter g and stays 0.
    Measured on an MI355X: max|dg| 1.7e-6 .. 1.3e-5 over the ten cases against CPU
    yardsticks of 1.4e-6 .. 4.7e-6; the worst element is at 0.014 of its
    allowance (bf16, 2x8x8x64), which the summation bound sets (up to 1.6e-3
    where |W1| |u| is large)."""
    if case == "far-mean":
        shape = (2, 14, 14, 256)
        x, ops = _far_mean_input(shape, dt), _operands(256, dt, True, (50.0, 150.0))
    else:
        shape = tuple(int(v) for v in case.split("x"))
        x, ops = _input(shape, dt), _operands(shape[3], dt, True)
    rc, _, gate = _run(x.to(DEV), ops, 0, dt, gate=True)
    assert rc == 0
    g64, bound, yard = _gate_reference(x, ops)
    err = (gate.cpu().double() - g64).abs()
    allow = torch.clamp(bound, min=4 * yard)
    ratio = float((err / allow).max())
    print(f"gate {case} {dt}: max|dg| {float(err.max()):.3e}, fp32 CPU yardstick {yard:.3e}, summation bound up to "
          f"{float(bound.max()):.3e}; worst element at {ratio:.3f} of its allowance")
    assert torch.isfinite(gate).all() and ratio <= 1, (case, dt, ratio)


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_gate_max_is_exact_and_starts_from_minus_infinity(dt):
    """belt 0, linear_1 the identity, the centre tap 1 and its bias 0: u = alpha
    * max.  Even channels have a positive max 8 + k/8 and alpha 1, odd channels
    are all-negative with max -(8 + k/8) and alpha -1, so u >= 8 everywhere,
    where GELU(u) == u in fp32 (erf(u / sqrt 2) rounds to 1): g must equal
    |max| bit for bit.  A max that starts from 0 gives 0 on the odd channels."""
    n, h, w, c = 2, 9, 15, 128
    ops = dict(_operands(c, dt, True))
    sign = torch.where(torch.arange(c) % 2 == 0, 1.0, -1.0)
    ops["gate4"] = torch.stack([sign, torch.ones(c), torch.zeros(c), torch.zeros(c)])
    ops["w1"], ops["b1"] = torch.eye(c), torch.zeros(c)
    top = 8 + (torch.arange(c) % 32) / 8.0                                    # exact in bf16 and fp16
    g = torch.Generator().manual_seed(5)
    x = sign * top - 0.5 - 3 * torch.rand(n, h, w, c, generator=g)            # below the max everywhere ...
    x.view(n, h * w, c)[:, 37] = sign * top                                   # ... but at one position
    x = x.to(T16[dt])                                                         # odd channels: all-negative, max = -top
    want = x.float().reshape(n, h * w, c).amax(1) * sign
    assert torch.equal(want, top.expand(n, c)) and (x.float()[..., 1::2] < 0).all()
    rc, _, gate = _run(x.to(DEV), ops, 0, dt, gate=True)
    assert rc == 0
    assert torch.equal(gate.cpu(), want)


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_padded_taps_contribute_zero_not_linear_0_bias(dt):
    """linear_0 = 0 with bias 1 on the y half, all-ones depthwise taps without
    bias, the 2c -> 2c conv an identity and Wcat selecting h[2 ch]: the output
    is GELU(number of in-map taps): GELU(4), GELU(6), GELU(9) at corner, edge
    and interior.  A padded tap taken as linear_0's bias would give GELU(9)
    everywhere."""
    n, h, w, c = 1, 9, 11, 64
    z = torch.zeros
    wcat = z(c, 3 * c)
    wcat[torch.arange(c), c + 2 * torch.arange(c)] = 1
    ops = dict(w0=z(2 * c, c), b0=torch.cat([torch.ones(c), z(c)]), gate4=z(4, c), w1=z(c, c), b1=z(c),
               dww=torch.ones(2 * c, 9), dwb=z(2 * c), wpw=torch.eye(2 * c), bpw=z(2 * c), wcat=wcat, bcat=z(c))
    x = _input((n, h, w, c), dt)
    rc, got, _ = _run(x.to(DEV), ops, 0, dt)
    assert rc == 0
    ys, xs = torch.arange(h).view(h, 1), torch.arange(w).view(1, w)
    rows = torch.minimum(ys + 1, torch.tensor(h - 1)) - torch.clamp(ys - 1, min=0) + 1
    cols = torch.minimum(xs + 1, torch.tensor(w - 1)) - torch.clamp(xs - 1, min=0) + 1
    count = (rows * cols).double()
    assert count[0, 0] == 4 and count[0, 5] == 6 and count[4, 5] == 9
    want = torch.nn.functional.gelu(count).view(1, h, w, 1).expand(n, h, w, c)
    ulp = 2.0 ** (torch.floor(torch.log2(want)) - MANT[dt])
    err = (got.cpu().double() - want).abs()
    assert (err <= ulp).all(), float((err / ulp).max())
    # and against the float64 reference of the block
    ref = R.smfa_block(_nchw(x, torch.float64), ops, False).permute(0, 2, 3, 1)
    assert ((got.cpu().double() - ref).abs() <= ulp).all()


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("residual", [0, 1])
@pytest.mark.parametrize("shape", [(3, 9, 15, 128), (3, 14, 14, 256)], ids=SID)
def test_a_crop_does_not_depend_on_its_batch(shape, residual, dt):
    x = _input(shape, dt).to(DEV)
    ops = _operands(shape[3], dt)
    rc3, three, g3 = _run(x, ops, residual, dt, gate=True)
    rc1, one, g1 = _run(x[1:2].contiguous(), ops, residual, dt, gate=True)
    assert rc3 == 0 and rc1 == 0
    assert torch.equal(three[1:2].view(torch.int16), one.view(torch.int16))
    assert torch.equal(g3[1:2], g1)


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("residual", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_nothing_is_written_outside_out_and_scratch(shape, residual, dt):
    """out and scratch (exactly fac_smfa_scratch_bytes) carved from larger
    device buffers filled with a pattern: the guard words on both sides are
    unchanged, and the result is the plain call's.  (2,8,8,64) is the one case
    whose last GEMM stores through the 64-column tile, in a single workgroup."""
    guard = 256                                   # bytes; keeps the 16-byte alignment
    lib = _lib.load()
    x = _input(shape, dt).to(DEV)
    ops = _operands(shape[3], dt)
    nbytes = lib.fac_smfa_scratch_bytes(*shape)
    n, h, w, c = shape
    assert nbytes == n * h * w * 2 * c * 2 * 2 + n * c * 4
    sbuf = torch.full((guard + nbytes + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    obuf = torch.full((guard + x.numel() * 2 + guard,), 0x5A, dtype=torch.uint8, device=DEV)
    out = obuf[guard:guard + x.numel() * 2].view(T16[dt]).view(x.shape)
    rc, got, _ = _run(x, ops, residual, dt, out=out, scratch=sbuf[guard:guard + nbytes])
    assert rc == 0
    for buf, pat, size in ((sbuf, 0xA5, nbytes), (obuf, 0x5A, x.numel() * 2)):
        assert bool((buf[:guard] == pat).all()) and bool((buf[guard + size:] == pat).all())
    assert torch.equal(got.view(torch.int16), _run(x, ops, residual, dt)[1].view(torch.int16))


def test_error_returns():
    """Every rejected call returns before a launch: out keeps its pattern."""
    dt = "fp16"
    lib = _lib.load()
    x = torch.zeros(1, 16, 16, 320, dtype=torch.float16, device=DEV)
    out = torch.full_like(x, 7.0)
    scratch = torch.empty(1 << 22, dtype=torch.uint8, device=DEV)
    ops = _operands(64, dt)
    run = lambda shape, **kw: _run(x, ops, 0, dt, shape=shape, out=out, scratch=scratch, **kw)[0]  # noqa: E731
    assert run((1, 7, 8, 64)) == SHAPE_ERR
    assert run((1, 16, 8, 64)) == SHAPE_ERR
    assert run((1, 8, 16, 64)) == SHAPE_ERR
    assert run((1, 8, 8, 96)) == SHAPE_ERR
    assert run((1, 8, 8, 320)) == SHAPE_ERR
    assert run((0, 8, 8, 64)) == ARG_ERR
    assert run((1, 8, 8, 64), dtype_id=2) == ARG_ERR
    wpk = _packed(ops, dt)
    st = torch.cuda.current_stream().cuda_stream
    args = lambda xp, wp, op, sp: (1, xp, 1, 8, 8, 64, wp, 0, op, None, sp, st)  # noqa: E731
    assert lib.fac_smfa(*args(None, wpk.data_ptr(), out.data_ptr(), scratch.data_ptr())) == ARG_ERR
    assert lib.fac_smfa(*args(x.data_ptr(), wpk.data_ptr(), None, scratch.data_ptr())) == ARG_ERR
    assert lib.fac_smfa(*args(x.data_ptr(), wpk.data_ptr(), out.data_ptr(), None)) == ARG_ERR
    assert lib.fac_smfa(*args(x.data_ptr(), None, out.data_ptr(), scratch.data_ptr())) == ARG_ERR
    # x, the weight blob, out and scratch must be 16-byte aligned
    assert lib.fac_smfa(*args(x.data_ptr() + 2, wpk.data_ptr(), out.data_ptr(), scratch.data_ptr())) == ARG_ERR
    assert lib.fac_smfa(*args(x.data_ptr(), wpk.data_ptr() + 8, out.data_ptr(), scratch.data_ptr())) == ARG_ERR
    assert lib.fac_smfa(*args(x.data_ptr(), wpk.data_ptr(), out.data_ptr() + 2, scratch.data_ptr())) == ARG_ERR
    assert lib.fac_smfa(*args(x.data_ptr(), wpk.data_ptr(), out.data_ptr(), scratch.data_ptr() + 4)) == ARG_ERR
    for bad in [(1, 7, 8, 64), (1, 8, 16, 64), (1, 8, 8, 96), (0, 8, 8, 64)]:
        assert lib.fac_smfa_scratch_bytes(*bad) == 0
    assert lib.fac_smfa_packed_bytes(96) == 0 and lib.fac_smfa_packed_bytes(320) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert run((1, 8, 8, 64)) == 0                # and the legal call next to them runs


# ---------------------------------------------------------------- fac_ggca_scale
GGCA_SITES = [(3, 7, 7, 512), (3, 14, 14, 256)]     # cvit_GGCA's and cvit_GGCA4's; 4 groups


@functools.lru_cache(maxsize=None)
def _ggca_weights(c):
    """Random GGCA(c, ., ., 16, 4).shared_conv weights, the reference module's shapes."""
    g = torch.Generator().manual_seed(1000 + c)
    cg, cr = c // 4, c // 64
    u = lambda *s, lo=-1.0, hi=1.0: torch.rand(*s, generator=g) * (hi - lo) + lo  # noqa: E731
    w1 = u(cr, cg, 1, 1) * (3.0 / cg) ** 0.5
    bn = (u(cr, lo=-0.2, hi=0.2), u(cr, lo=0.5, hi=1.5), u(cr, lo=0.8, hi=1.2), u(cr, lo=-0.2, hi=0.2))
    return w1, u(cr, lo=-0.1, hi=0.1), bn, u(cg, cr, 1, 1), u(cg, lo=-0.1, hi=0.1)


def _ggca_scale(x16, dt, shape=None, groups=4, dtype_id=None, x_ptr=0):
    """fac_ggca_scale on a device tensor [n,h,w,c]; returns (status, out)."""
    n, h, w, c = shape or x16.shape
    w1, b1, bn, w2, b2 = _ggca_weights(x16.shape[3])
    cr, cg = w1.shape[:2]
    wts = [t.to(DEV, torch.float32).contiguous() for t in (w1.reshape(cr, cg), b1, torch.stack(bn), w2.reshape(cg, cr), b2)]
    out = torch.full_like(x16, 7.0)
    rc = _lib.load().fac_ggca_scale(_lib.DTYPES[dt] if dtype_id is None else dtype_id,
                                    x_ptr if x_ptr != 0 else x16.data_ptr(), n, h, w, c, groups,
                                    *[t.data_ptr() for t in wts], out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", GGCA_SITES, ids=SID)
def test_ggca_scale_vs_reference(torch_threads, shape, dt):
    """GGCA(x) = (x * att_h) * att_w within one 16-bit rounding of the fp32
    reference module (variants_ref.ggca), on non-negative and on signed inputs,
    as test_variants_gpu.py holds fac_ggca_apply; and a crop does not depend
    on its batch."""
    from variants_ref import ggca
    n, h, w, c = shape
    for signed in (False, True):
        g = torch.Generator().manual_seed(7 + h * w + c + int(signed))
        x = (torch.randn(n, h, w, c, generator=g) * 1.5 if signed else torch.rand(n, h, w, c, generator=g) * 3).to(T16[dt])
        rc, got = _ggca_scale(x.to(DEV), dt)
        assert rc == 0
        with torch.no_grad():
            ref = ggca(_ggca_weights(c), x.float().permute(0, 3, 1, 2).contiguous()).permute(0, 2, 3, 1)
        err = float(((got.float().cpu() - ref).abs() / ref.abs().clamp_min(1e-3)).max())
        print(f"fac_ggca_scale {shape} {dt} signed {signed}: max rel err {err:.3e} (bound {KERNEL_BOUND[dt]:.3e})")
        assert err <= KERNEL_BOUND[dt], (shape, dt, signed, err)
        rc1, one = _ggca_scale(x[1:2].contiguous().to(DEV), dt)
        assert rc1 == 0 and torch.equal(got[1:2].view(torch.int16), one.view(torch.int16))


def test_ggca_scale_error_returns():
    x = torch.zeros(1, 56, 56, 256, dtype=torch.float16, device=DEV)
    assert _ggca_scale(x, "fp16", shape=(1, 56, 56, 256))[0] == SHAPE_ERR     # the streaming route's shape
    assert _ggca_scale(x, "fp16", shape=(1, 17, 17, 256))[0] == SHAPE_ERR     # 17 > 16
    assert _ggca_scale(x, "fp16", shape=(1, 14, 14, 96))[0] == SHAPE_ERR      # cg = 24, no multiple of 16
    assert _ggca_scale(x, "fp16", shape=(1, 14, 14, 256), groups=3)[0] == ARG_ERR
    assert _ggca_scale(x, "fp16", shape=(0, 14, 14, 256))[0] == ARG_ERR
    assert _ggca_scale(x, "fp16", shape=(1, 14, 14, 256), dtype_id=2)[0] == ARG_ERR
    assert _ggca_scale(x, "fp16", shape=(1, 14, 14, 256), x_ptr=None)[0] == ARG_ERR
    rc, out = _ggca_scale(x, "fp16", shape=(1, 17, 17, 256))
    assert rc == SHAPE_ERR and bool((out == 7.0).all())                       # returned before any launch
    assert _ggca_scale(x, "fp16", shape=(1, 14, 14, 256))[0] == 0


# ---------------------------------------------------------------- the drop-ins
def _sd_t(name):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in make_other_state_dict(name, 0).items()}


@pytest.fixture(scope="module")
def models():
    """The drop-ins per (class, dtype), built on first use, released when the module is done."""
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from fac_fake_amd import other
    built = {}

    def get(name, dt):
        if (name, dt) not in built:
            m = other.CViT(name, dtype=dt)
            m.load_state_dict(_sd_t(name))
            m.to(DEV)
            built[name, dt] = m
        return built[name, dt]
    yield get
    torch.cuda.synchronize()
    for m in built.values():
        m._release()


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("name", R.NAMES)
def test_model_matches_reference(golden, models, name, dt):
    """forward_u8 on the 4 golden crops against the reference class's fp32
    probabilities, within 2x the recorded 16-bit emulation envelope of that
    class and dtype (test_other.py holds the emulation to 1.25x)."""
    g = golden("other_golden.npz")
    tol = 2 * golden("other_envelope.json")[name][dt]
    crops = torch.from_numpy(make_crops(4, seed=int(g["crop_seed"]))).to(DEV)
    with torch.no_grad():
        lg, pr = models(name, dt).forward_u8(crops, return_probs=True)
        torch.cuda.synchronize()
    lg, pr = lg.cpu().numpy(), pr.cpu().numpy()
    p_ref = 1 / (1 + np.exp(-g[f"{name}/logits"]))
    d = float(np.abs(pr - p_ref).max())
    print(f"{name} {dt}: max|dp| vs reference {d:.3e} (tolerance {tol:.3e})")
    assert np.isfinite(lg).all()
    assert d <= tol, (name, dt, d, tol)
    assert np.allclose(pr, 1 / (1 + np.exp(-lg)), atol=1e-6)


def test_smfa_map_in_the_model_matches_the_block_reference(models):
    """The GPU's own features1 map [B,14,14,256] through smfa_block on the CPU
    against the GPU's map after x + SMFA(x), under the block rule of
    test_smfa_vs_float64_reference: this isolates the block, with the model's
    weights and activations, from the 13 convs before it.  Measured on an
    MI355X: relative L2 at 0.36 of its allowance, max|d| at 0.25."""
    dt = "fp16"
    crops = torch.from_numpy(make_crops(2, seed=44)).to(DEV)
    m = models("cvit_GGCA_SMFA", dt)
    with torch.no_grad():
        m.forward_u8(crops)   # prepares the packed layers
        f1 = m.stem_features(crops, u8=True, upto="features1").cpu()
        got = m.stem_features(crops, u8=True, upto="smfa").cpu()
    assert tuple(f1.shape) == (2, 14, 14, 256) and got.shape == f1.shape
    ops = R.smfa_fold(make_other_state_dict("cvit_GGCA_SMFA", 0))
    ops = {k: (R.round_to(v, dt) if k in ("w0", "wpw", "wcat") else v) for k, v in ops.items()}
    with torch.no_grad():
        ref = R.smfa_block(_nchw(f1, torch.float64), ops, True).permute(0, 2, 3, 1)
        emu = R.smfa_block(_nchw(f1, torch.float32), ops, True, dtype=torch.float32, round=dt).double().permute(0, 2, 3, 1)
    l2, mx = _rule1(got, ref, emu, dt)
    print(f"x + SMFA(x) in the model: relative L2 at {l2:.3f} of its allowance, max|d| at {mx:.3f}")
    assert l2 <= 1 and mx <= 1, (l2, mx)


def test_reserve_covers_the_smfa_scratch(models):
    """After reserve(B) a forward of up to B crops allocates no SMFA scratch: the buffer is the reserved one."""
    m = models("cvit_GGCA_SMFA", "fp16")
    m.reserve(8, DEV)
    buf = m._smfa_scratch
    assert buf.numel() >= _lib.load().fac_smfa_scratch_bytes(8, 14, 14, 256)
    with torch.no_grad():
        m.forward_u8(torch.from_numpy(make_crops(5, seed=46)).to(DEV))
    assert m._smfa_scratch is buf and m._smfa_scratch.data_ptr() == buf.data_ptr()


def test_u8_and_nchw_paths_agree(models):
    crops = make_crops(3, seed=43)
    m = models("cvit_GGCA_SMFA", "fp16")
    with torch.no_grad():
        a = m.forward_u8(torch.from_numpy(crops).to(DEV))
        b = m(normalize_u8(crops).to(DEV))
        torch.cuda.synchronize()
        assert torch.equal(a, b)
        with pytest.raises(RuntimeError):      # the reference's pos_embedding[0:B] past 32 crops
            m.forward_u8(torch.zeros(33, 224, 224, 3, dtype=torch.uint8, device=DEV))


def test_graph_replay_matches_eager(models):
    crops = torch.from_numpy(make_crops(8, seed=45)).to(DEV)
    slots = torch.arange(8, dtype=torch.int32, device=DEV) * 3 % 32
    m = models("cvit_GGCA_SMFA", "bf16")
    with torch.no_grad():
        eager = m.forward_u8(crops, pos_index=slots)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            m.forward_u8(crops, pos_index=slots)    # warm up on the capture stream before the capture
            with torch.cuda.graph(g, stream=s):
                out = m.forward_u8(crops, pos_index=slots)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
        del g


def test_predict_video_takes_the_model(models):
    """video.predict_video on a 30-frame synthetic video (3 crops): the logits
    of the model on those crops, and prediction.predict_crops' score up to the
    device sigmoid's last bit."""
    from fac_fake_amd.prediction import chunk_slots, predict_crops
    from fac_fake_amd.video import crop_faces, predict_video, reference_boxes, synthetic_video
    frames, boxes = synthetic_video(30, 360, 640, seed=3, device=DEV)
    m = models("cvit_GGCA_SMFA", "fp16")
    score, logits = predict_video(m, frames, boxes, return_logits=True)
    sel = reference_boxes(boxes, 30)
    crops = crop_faces(frames, sel)
    with torch.no_grad():
        want = m.forward_u8(crops, pos_index=torch.from_numpy(chunk_slots(len(sel))))
    assert len(sel) == 3 and torch.equal(logits, want)
    assert abs(score - predict_crops(m, crops)) <= 1e-6
