"""The ODConv2d block and the two ODConv CViT classes on the GPU: fac_odconv
(odconv.hip) against the float64 restatement of the block (tests/odconv_ref.py),
and the drop-ins of fac_fake_amd/odconv.py against the reference classes'
recorded outputs (tests/golden/odconv_*, tools/make_golden_odconv.py).

The conv weights differ per crop.  Every block input here gives each crop its
own per-channel offset, and the references assert that the crops' attentions
really differ (argmax ka, and ca by at least 0.2), so a kernel that used one
crop's attention or aggregated weight for another could not pass.
"""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))

import odconv_ref as R  # noqa: E402
from fac_fake_amd import _lib  # noqa: E402
from fac_fake_amd.weights import make_crops, make_odconv_state_dict  # noqa: E402
from oracle.cvit_torch import normalize_u8, round_to  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
# |got - ref| / max(|ref|, 1e-3): twice the half-ulp of the output rounding (KERNEL_BOUND of test_mdfa_gpu.py)
KERNEL_BOUND = {"fp16": 2 ** -10 + 1e-5, "bf16": 2 ** -7 + 1e-5}
# (n, h, w, c).  Small and non-square, one per width; the two 7x7 / 14x14 maps of 49 / 196 rows, which
# are no multiple of a wave's 32 rows or a workgroup's 128; 15 rows per crop, three crops to a 32-row tile if tiles
# ran over the flattened batch; the smallest legal map.
SHAPES = [(2, 10, 14, 64), (3, 6, 6, 128), (1, 4, 18, 256), (2, 7, 7, 256), (3, 14, 14, 256), (5, 3, 5, 64), (5, 3, 5, 256),
          (2, 2, 2, 128)]
SID = lambda s: "x".join(map(str, s))  # noqa: E731


def _with_pool(shapes):
    """(shape, pool) for pool off and, where h and w are even, on."""
    return [(s, p) for s in shapes for p in (0, 1) if not (p and (s[-3] % 2 or s[-2] % 2))]


PID = lambda v: SID(v) if isinstance(v, tuple) else f"pool{v}"  # noqa: E731
KINDS = ("signed", "relu")
SHAPE_ERR, ARG_ERR = -2, -1
GUARD = 256                                       # bytes; keeps the 16-byte alignment
ULP1 = 2.0 ** -23
NAMES = R.NAMES


def _nchw(x16, dtype=torch.float64):
    return x16.to(dtype).permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def _operands(c):
    """Random fac_odconv_pack operands (fp32): four independent W_k in +-8
    sqrt(6 / 9c), fc in +-sqrt(3 / c), the attention's folded BatchNorm with
    scale in [0.5, 1.5] and shift in +-0.5, heads in +-0.6 with biases in +-1
    (kernel head: biases in +-0.5), scale in +-[0.5, 1.5], shift in +-0.3.
    The blob holds no 16-bit value, so the operands serve both dtypes."""
    g = torch.Generator().manual_seed(2400 + c)
    u = lambda *s, a=1.0: (torch.rand(*s, generator=g) * 2 - 1) * a  # noqa: E731
    sgn = lambda n: torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)  # noqa: E731
    return dict(weight=u(4, c, c, 3, 3, a=8 * (6.0 / (9 * c)) ** 0.5), fc=u(16, c, a=(3.0 / c) ** 0.5),
                bn_scale=0.5 + torch.rand(16, generator=g), bn_shift=u(16, a=0.5),
                channel_fc=u(c, 16, a=0.6), channel_b=u(c), filter_fc=u(c, 16, a=0.6), filter_b=u(c),
                spatial_fc=u(9, 16, a=0.6), spatial_b=u(9), kernel_fc=u(4, 16, a=0.6), kernel_b=u(4, a=0.5),
                scale=(0.5 + torch.rand(c, generator=g)) * sgn(c), shift=u(c, a=0.3))


def _draw(shape, dt, kind, seed):
    n, h, w, c = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, c, generator=g) * 1.5 + (torch.rand(n, 1, 1, c, generator=g) * 2 - 1) * 1.5
    return (torch.relu(x + 0.5) if kind == "relu" else x).to(T16[dt])


@functools.lru_cache(maxsize=None)
def _input(shape, dt, kind):
    """NHWC 16-bit, every crop with its own per-channel offset: "signed" randn
    1.5 + offset, "relu" relu(that + 0.5).  For n >= 2 the seed is the first of
    41 + h w + c + len(kind) + 1000 k for which, on the float64 reference alone,
    argmax ka differs between two crops and max |ca_b - ca_b'| >= 0.2."""
    n, h, w, c = shape
    seed = 41 + h * w + c + len(kind)
    ops = _operands(c)
    for k in range(64):
        x = _draw(shape, dt, kind, seed + 1000 * k)
        if n < 2:
            return x
        ca, _fa, _sa, ka = R.attentions(_nchw(x), ops)
        if len(set(ka.argmax(1).tolist())) >= 2 and float((ca.unsqueeze(0) - ca.unsqueeze(1)).abs().max()) >= 0.2:
            return x
    raise AssertionError(f"no seed gives crops of different attentions for {shape} {dt} {kind}")


def _finish(pre, dt, relu, pool):
    """A pre-activation map -> act -> (dt: output rounding) -> pool."""
    out = F.relu(pre) if relu else pre
    if dt:
        out = round_to(out, dt)
    return F.max_pool2d(out, 2, 2) if pool else out


@functools.lru_cache(maxsize=None)
def _case(shape, dt, kind):
    """dict(ref, emu: the pre-activation maps [B,C,H,W] in float64 and of the
    fp32 emulation with the kernel's declared weight rounding; att: the float64
    attentions), on the CPU, once per input."""
    torch.set_num_threads(16)
    x = _nchw(_input(shape, dt, kind))
    ops = _operands(shape[3])
    with torch.no_grad():
        ref, att = R.odconv_block(x, ops, torch.float64, relu=False, parts=True)
        ca, fa, sa, ka = R.attentions(x.float(), ops, torch.float32)
        wagg = round_to(R.aggregate(ops, ca, sa, ka, torch.float32), dt)
        B, C, H, W = x.shape
        emu = F.conv2d(x.float().reshape(1, B * C, H, W), wagg.reshape(B * C, C, 3, 3), padding=1, groups=B).view(B, C, H, W)
        emu = emu * fa.view(B, C, 1, 1) * ops["scale"].view(1, C, 1, 1) + ops["shift"].view(1, C, 1, 1)
    if shape[0] >= 2:                  # the crops' weights really differ
        assert len(set(att["ka"].argmax(1).tolist())) >= 2
        assert float((att["ca"].unsqueeze(0) - att["ca"].unsqueeze(1)).abs().max()) >= 0.2
    return dict(ref=ref, emu=emu.double(), att=att)


_PACKED = {}


def _packed(ops, dt):
    from fac_fake_amd import odconv
    key = (id(ops), dt)
    if key not in _PACKED:
        _PACKED[key] = (ops, odconv.odconv_pack(ops, dt, DEV))       # keeps ops alive: id() stays unique
    return _PACKED[key][1]


def _scratch(shape):
    return torch.empty(_lib.load().fac_odconv_scratch_bytes(*shape), dtype=torch.uint8, device=DEV)


def _run(x16, packed, dt, relu=1, pool=0, shape=None, out=None, att=None, scratch=None, dtype_id=None):
    """fac_odconv on a device tensor [n,h,w,c]; returns (status, out, att_out)."""
    n, h, w, c = shape or x16.shape
    if out is None:
        out = torch.empty((n, h // 2, w // 2, c) if pool else (n, h, w, c), dtype=x16.dtype, device=DEV)
    if att is None:
        att = torch.zeros(max(n, 1), 2 * c + 13, dtype=torch.float32, device=DEV)
    if scratch is None:
        scratch = _scratch(tuple(x16.shape))
    rc = _lib.load().fac_odconv(_lib.DTYPES[dt] if dtype_id is None else dtype_id, x16.data_ptr(), n, h, w, c,
                                packed.data_ptr(), relu, pool, out.data_ptr(), att.data_ptr(), scratch.data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out, att


def _rule1(got, ref, emu, dt):
    """The block rule (_rule1 of test_mdfa_gpu.py): the GPU's error against the
    float64 reference measured by the CPU emulation's own error against it.
    Returns (relative L2 ratio, max|d| ratio, relative L2, max|d|)."""
    e_gpu, e_emu = got.double() - ref, emu - ref
    l2_allow = max(2 * float(e_emu.norm() / ref.norm()), KERNEL_BOUND[dt])
    mx_allow = max(4 * float(e_emu.abs().max()), KERNEL_BOUND[dt] * float(ref.abs().max()))
    l2, mx = float(e_gpu.norm() / ref.norm()), float(e_gpu.abs().max())
    return l2 / l2_allow, mx / mx_allow, l2, mx


def _att_bound(x16, ops):
    """(bound, att64 [B, 2c + 13]): 8 x the largest |fp32 - float64| of the
    formula evaluated with torch's tensor ops on this input, never below 4 fp32
    ulps of 1."""
    x = _nchw(x16)
    with torch.no_grad():
        a64 = R.att_row(dict(zip(("ca", "fa", "sa", "ka"), R.attentions(x, ops, torch.float64))))
        a32 = R.att_row(dict(zip(("ca", "fa", "sa", "ka"), R.attentions(x.float(), ops, torch.float32))))
    return max(8 * float((a32.double() - a64).abs().max()), 4 * ULP1), a64


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_attentions(shape, kind, dt):
    """att_out (ca | fa | sa | ka as the conv used them) against float64 on the
    same 16-bit input, within 8 x the error of a plain fp32 torch evaluation of
    the formula on that input (the kernel's reduction order differs from
    torch's), never tighter than 4 fp32 ulps of 1.
    Measured on an MI355X over the 32 cases: max|d| 7.5e-8 .. 1.5e-7 against
    bounds of 6.1e-7 .. 1.7e-6, a ratio of 0.06 .. 0.15."""
    x, ops = _input(shape, dt, kind), _operands(shape[3])
    bound, a64 = _att_bound(x, ops)
    rc, _out, att = _run(x.to(DEV), _packed(ops, dt), dt)
    assert rc == 0
    d = float((att.cpu().double() - a64).abs().max())
    print(f"att {shape} {kind} {dt}: max|d| {d:.3e}, bound {bound:.3e}, ratio {d / bound:.3f}")
    assert d <= bound, (d, bound)


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,pool", _with_pool(SHAPES), ids=PID)
def test_block_vs_float64_reference(shape, kind, pool, relu, dt):
    """fac_odconv against odconv_block(float64) on the same 16-bit inputs and
    fp32 operands.  The yardstick is the CPU emulation of the declared roundings
    (the aggregated weight, the output): relative L2 within 2x its error,
    max|d| within 4x, never tighter than KERNEL_BOUND.
    Measured on an MI355X over the 104 cases: relative L2 up to 3.1e-4 (fp16) /
    2.4e-3 (bf16), at most 0.31 of its allowance; max|d| at 0.18 .. 0.27 of its
    allowance (it mostly equals the emulation's, 0.25)."""
    n, h, w, c = shape
    x, ops = _input(shape, dt, kind), _operands(c)
    case = _case(shape, dt, kind)
    rc, got, _ = _run(x.to(DEV), _packed(ops, dt), dt, relu=relu, pool=pool)
    assert rc == 0
    ref, emu = _finish(case["ref"], None, relu, pool), _finish(case["emu"].float(), dt, relu, pool).double()
    g = _nchw(got.cpu())
    assert g.shape == ref.shape and torch.isfinite(g).all()
    l2r, mxr, l2, mx = _rule1(g, ref, emu, dt)
    print(f"{shape} {kind} pool {pool} relu {relu} {dt}: relative L2 {l2:.3e} at {l2r:.3f} of its allowance, max|d| {mx:.3e} at "
          f"{mxr:.3f}")
    assert l2r <= 1 and mxr <= 1, (shape, kind, pool, relu, dt, l2r, mxr)


# ---------------------------------------------------------------- exact cases
def _exact_ops(c, seed):
    """All attention weights and biases zero (ca = fa = sa = 1/2, ka = 1/4
    exactly), four different W_k with entries in {-1, 0, 1} on two input channels
    per output channel, scale and shift left to the caller."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randint(-1, 2, (4, c, c, 3, 3), generator=g).float()
    o, i = torch.arange(c).view(c, 1), torch.arange(c).view(1, c)
    w = w * ((i % (c // 2)) == (o % (c // 2))).float().view(1, c, c, 1, 1)
    z = torch.zeros
    return dict(weight=w, fc=z(16, c), bn_scale=torch.ones(16), bn_shift=z(16), channel_fc=z(c, 16), channel_b=z(c),
                filter_fc=z(c, 16), filter_b=z(c), spatial_fc=z(9, 16), spatial_b=z(9), kernel_fc=z(4, 16), kernel_b=z(4),
                scale=torch.ones(c), shift=z(c))


def _int_input(shape, dt, seed):
    return torch.randint(-2, 3, shape, generator=torch.Generator().manual_seed(seed)).to(T16[dt])


def _exact(x16, ops, w_eff, dt, relu, pool):
    """fac_odconv's output and the integer conv of x with w_eff [c, c, 3, 3] (-> act -> pool), both NCHW float64."""
    from fac_fake_amd import odconv
    want = _finish(F.conv2d(_nchw(x16), w_eff.double(), padding=1), None, relu, pool)
    assert float(want.abs().max()) <= 256          # integers that both 16-bit formats hold exactly
    rc, got, att = _run(x16.to(DEV), odconv.odconv_pack(ops, dt, DEV), dt, relu=relu, pool=pool)
    assert rc == 0
    return _nchw(got.cpu()), want, att.cpu()


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("shape,pool", _with_pool([(2, 4, 6, 64), (5, 3, 5, 64), (2, 7, 7, 256), (2, 2, 2, 128)]), ids=PID)
def test_uniform_attentions_are_an_integer_conv(shape, pool, dt):
    """Zero heads: ca = fa = sa = 0.5 and ka = 0.25 exactly, so with scale 32 the
    block is the integer conv with sum_k W_k, bit for bit, borders included
    (4, 6 or 9 taps in the map)."""
    n, h, w, c = shape
    relu = pool                        # identity without the pool, ReLU with it
    ops = _exact_ops(c, 7 + c)
    ops["scale"] = torch.full((c,), 32.0)
    x = _int_input(shape, dt, 5 + h * w)
    got, want, att = _exact(x, ops, ops["weight"].sum(0), dt, relu, pool)
    assert torch.equal(att[:, :2 * c + 9], torch.full((n, 2 * c + 9), 0.5)) and torch.equal(att[:, 2 * c + 9:], torch.full((n, 4), 0.25))
    assert float(want.abs().max()) > 4 and torch.equal(got, want)


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("j", [0, 1, 2, 3])
def test_one_hot_kernel_attention_reads_each_kernel_from_its_place(j, dt):
    """kernel_fc bias 0 for kernel j and -200 for the rest: ka is exactly one-hot,
    and with scale 8 the block is the integer conv with W_j alone."""
    shape, c = (2, 5, 6, 128), 128
    ops = _exact_ops(c, 11)
    ops["kernel_b"] = torch.full((4,), -200.0)
    ops["kernel_b"][j] = 0.0
    ops["scale"] = torch.full((c,), 8.0)
    assert all(not torch.equal(ops["weight"][j], ops["weight"][k]) for k in range(4) if k != j)
    got, want, att = _exact(_int_input(shape, dt, 13), ops, ops["weight"][j], dt, 0, 0)
    assert torch.equal(att[:, 2 * c + 9:], F.one_hot(torch.tensor([j, j]), 4).float())
    assert float(want.abs().max()) > 4 and torch.equal(got, want)


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("tap", range(9))
def test_one_hot_spatial_attention_pins_each_tap(tap, dt):
    """spatial_fc bias +200 for one tap and -200 for the rest (sigmoid(+-200) is
    exactly 1 / 0 in fp32), on a 3x3 map: with scale 16 the block is the integer
    conv with that tap alone, which pins the tap's (dy, dx)."""
    shape, c = (2, 3, 3, 64), 64
    ops = _exact_ops(c, 17)
    ops["spatial_b"] = torch.full((9,), -200.0)
    ops["spatial_b"][tap] = 200.0
    ops["scale"] = torch.full((c,), 16.0)
    w_eff = torch.zeros(c, c, 9)
    w_eff[:, :, tap] = ops["weight"].sum(0).reshape(c, c, 9)[:, :, tap]
    got, want, att = _exact(_int_input(shape, dt, 19), ops, w_eff.view(c, c, 3, 3), dt, 0, 0)
    assert torch.equal(att[:, 2 * c:2 * c + 9], F.one_hot(torch.tensor([tap, tap]), 9).float())
    assert float(want.abs().max()) > 2 and torch.equal(got, want)


# ---------------------------------------------------------------- robustness
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("hwc,pool", _with_pool([(6, 6, 128), (3, 5, 64), (4, 4, 256)]), ids=PID)
def test_a_crop_does_not_depend_on_its_batch(hwc, pool, dt):
    """Crop k alone against crop k inside batches of 2, 5, 33 and (c = 256, where
    the 48 MiB of aggregated weights hold 42 crops and 43 need a second chunk) 43, at different
    positions: output and att_out, bitwise."""
    h, w, c = hwc
    pk = _packed(_operands(c), dt)
    crop = _draw((1, h, w, c), dt, "relu", 77)
    rc, one, att1 = _run(crop.to(DEV), pk, dt, pool=pool)
    assert rc == 0
    for n, pos in ((2, 1), (5, 3), (33, 32), (43, 42)):
        if n == 43 and c != 256:
            continue
        x = _draw((n, h, w, c), dt, "relu", 78 + n)
        x[pos] = crop[0]
        rc, many, att = _run(x.to(DEV), pk, dt, pool=pool)
        assert rc == 0
        assert torch.equal(many[pos:pos + 1].view(torch.int16), one.view(torch.int16)), (n, pos)
        assert torch.equal(att[pos:pos + 1], att1), (n, pos)
        assert not torch.equal(att[(pos + 1) % n:(pos + 1) % n + 1], att1)


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("shape,pool", _with_pool([(2, 10, 14, 64), (3, 6, 6, 128), (5, 3, 5, 256), (2, 2, 2, 128)]), ids=PID)
def test_nothing_is_written_outside_out_att_or_the_scratch(shape, pool, dt):
    """out, att_out and a scratch of exactly fac_odconv_scratch_bytes carved from
    larger device buffers filled with a pattern: the guard bytes on both sides
    of each are unchanged, the result is the plain call's and x is unchanged."""
    n, h, w, c = shape
    x = _input(shape, dt, "relu").to(DEV)
    keep = x.clone()
    pk = _packed(_operands(c), dt)
    nb = x.numel() * 2 // (4 if pool else 1)
    ns, nt = _lib.load().fac_odconv_scratch_bytes(*shape), n * (2 * c + 13) * 4
    assert ns > 0 and ns % 16 == 0
    nt_pad = (nt + 15) // 16 * 16
    bufs = [torch.full((GUARD + k + GUARD,), 0x5A, dtype=torch.uint8, device=DEV) for k in (nb, nt_pad, ns)]
    out = bufs[0][GUARD:GUARD + nb].view(T16[dt]).view((n, h // 2, w // 2, c) if pool else (n, h, w, c))
    att = bufs[1][GUARD:GUARD + nt].view(torch.float32).view(n, 2 * c + 13)
    rc, got, a = _run(x, pk, dt, pool=pool, out=out, att=att, scratch=bufs[2][GUARD:GUARD + ns])
    assert rc == 0
    for b, k in zip(bufs, (nb, nt, ns)):
        assert bool((b[:GUARD] == 0x5A).all()) and bool((b[GUARD + k:] == 0x5A).all())
    rc2, plain, a2 = _run(x, pk, dt, pool=pool)
    assert rc2 == 0 and torch.equal(got.view(torch.int16), plain.view(torch.int16)) and torch.equal(a, a2)
    assert torch.equal(x.view(torch.int16), keep.view(torch.int16))


def test_error_returns():
    """Every rejected call returns before a launch: out keeps its pattern.  Argument checks only."""
    dt = "fp16"
    lib = _lib.load()
    x = torch.zeros(1, 16, 16, 256, dtype=torch.float16, device=DEV)
    out = torch.full_like(x, 7.0)
    pk = _packed(_operands(64), dt)
    scr = _scratch((1, 16, 16, 256))
    run = lambda shape, **kw: _run(x, pk, dt, shape=shape, out=out, scratch=scr, **kw)[0]  # noqa: E731
    for bad in ((1, 8, 8, 32), (1, 8, 8, 96), (1, 1, 8, 64), (1, 8, 1, 64), (1, 225, 8, 64), (1, 8, 8, 512)):
        assert run(bad) == SHAPE_ERR, bad
        assert lib.fac_odconv_scratch_bytes(*bad) == 0, bad
    assert run((1, 7, 8, 64), pool=1) == SHAPE_ERR and run((1, 8, 7, 64), pool=1) == SHAPE_ERR
    assert run((0, 8, 8, 64)) == ARG_ERR and run((-1, 8, 8, 64)) == ARG_ERR
    assert run((1, 8, 8, 64), dtype_id=2) == ARG_ERR and run((1, 8, 8, 64), pool=2) == ARG_ERR
    assert run((1, 8, 8, 64), relu=2) == ARG_ERR and run((1, 8, 8, 64), relu=-1) == ARG_ERR
    assert lib.fac_odconv_scratch_bytes(0, 8, 8, 64) == 0 and lib.fac_odconv_scratch_bytes(65536, 2, 2, 64) == 0
    # the limits on n and on n h w, on fac_odconv itself (both return before anything is read or launched)
    assert run((65536, 2, 2, 64)) == SHAPE_ERR and run((65535, 224, 224, 64)) == SHAPE_ERR
    assert lib.fac_odconv_scratch_bytes(65535, 224, 224, 64) == 0 and lib.fac_odconv_scratch_bytes(65535, 2, 2, 64) > 0
    assert lib.fac_odconv_chunk(256, 256) == 42 and lib.fac_odconv_chunk(43, 256) == 42 and lib.fac_odconv_chunk(8, 256) == 8 and lib.fac_odconv_chunk(256, 64) == 256
    assert lib.fac_odconv_chunk(0, 64) == 0 and lib.fac_odconv_chunk(8, 96) == 0
    assert lib.fac_odconv_packed_bytes(96) == 0 and lib.fac_odconv_packed_bytes(32) == 0
    assert all(lib.fac_odconv_packed_bytes(k) > 0 for k in (64, 128, 256))
    # the scratch is bounded: 256 crops at 256 channels keep 42 crops' aggregated weights, not 256
    assert lib.fac_odconv_scratch_bytes(256, 28, 28, 256) < (48 << 20) + (2 << 20)
    st = torch.cuda.current_stream().cuda_stream
    args = lambda xp, pp, op, sp, ap=None: (1, xp, 1, 8, 8, 64, pp, 1, 0, op, ap, sp, st)  # noqa: E731
    X, P, O, S = x.data_ptr(), pk.data_ptr(), out.data_ptr(), scr.data_ptr()
    assert lib.fac_odconv(*args(None, P, O, S)) == ARG_ERR
    assert lib.fac_odconv(*args(X, None, O, S)) == ARG_ERR
    assert lib.fac_odconv(*args(X, P, None, S)) == ARG_ERR
    assert lib.fac_odconv(*args(X, P, O, None)) == ARG_ERR
    assert lib.fac_odconv(*args(O, P, O, S)) == ARG_ERR          # not in place
    assert lib.fac_odconv(*args(X + 2, P, O, S)) == ARG_ERR      # 16-byte alignment, of each of the four
    assert lib.fac_odconv(*args(X, P + 8, O, S)) == ARG_ERR
    assert lib.fac_odconv(*args(X, P, O + 4, S)) == ARG_ERR
    assert lib.fac_odconv(*args(X, P, O, S + 2)) == ARG_ERR
    assert lib.fac_odconv(*args(X, P, O, S, S + 2)) == ARG_ERR   # att_out: 4-byte alignment
    c = 64
    host = [torch.zeros(k) for k in (36 * c * c, 16 * c, 16, 16, 16 * c, c, 16 * c, c, 144, 9, 64, 4, c, c)]
    ptrs = [t.data_ptr() for t in host]
    blob = torch.zeros(lib.fac_odconv_packed_bytes(c), dtype=torch.uint8)
    assert lib.fac_odconv_pack(2, c, *ptrs, blob.data_ptr()) == ARG_ERR
    assert lib.fac_odconv_pack(1, 96, *ptrs, blob.data_ptr()) == SHAPE_ERR
    assert lib.fac_odconv_pack(1, c, None, *ptrs[1:], blob.data_ptr()) == ARG_ERR
    assert lib.fac_odconv_pack(1, c, *ptrs[:-1], None, blob.data_ptr()) == ARG_ERR
    assert lib.fac_odconv_pack(1, c, *ptrs, None) == ARG_ERR
    assert lib.fac_odconv_pack(1, c, *ptrs, blob.data_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert run((1, 8, 8, 64)) == 0                # and the legal call next to them runs


# ---------------------------------------------------------------- the drop-ins
def _sd_t(name):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in make_odconv_state_dict(name, 0).items()}


@pytest.fixture(scope="module")
def models():
    """The drop-ins per (class, dtype), built on first use, released when the module is done."""
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from fac_fake_amd import odconv
    built = {}

    def get(name, dt):
        if (name, dt) not in built:
            m = odconv.CViT(name, dtype=dt)
            m.load_state_dict(_sd_t(name))
            m.to(DEV)
            built[name, dt] = m
        return built[name, dt]
    yield get
    torch.cuda.synchronize()
    for m in built.values():
        m._release()


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("name", NAMES)
def test_model_matches_reference(golden, models, name, dt):
    """forward_u8 on the 8 golden crops against the reference class's fp32
    probabilities, within 2x the recorded 16-bit emulation envelope of that
    class and dtype.  Measured on an MI355X: cvit_GGCA_ADD_ODConv 2.2e-4 of 4.7e-4
    allowed (fp16) and 1.6e-3 of 4.0e-3 (bf16); cvit_GGCA_ODConv 3.7e-4 of 9.4e-4
    and 4.0e-3 of 8.9e-3."""
    g = golden("odconv_golden.npz")
    tol = 2 * golden("odconv_envelope.json")[name][dt]
    want = g[name + "/probs"]
    crops = torch.from_numpy(make_crops(want.shape[0], seed=int(g["crop_seed"]))).to(DEV)
    with torch.no_grad():
        lg, pr = models(name, dt).forward_u8(crops, return_probs=True)
        torch.cuda.synchronize()
    lg, pr = lg.cpu().numpy(), pr.cpu().numpy()
    d = float(np.abs(pr - want).max())
    print(f"{name} {dt}: max|dp| vs reference {d:.3e} (tolerance {tol:.3e})")
    assert np.isfinite(lg).all()
    assert d <= tol, (name, dt, d, tol)
    assert np.allclose(pr, 1 / (1 + np.exp(-lg)), atol=1e-6)


_MODEL_SITES = [(NAMES[0], i) for i in range(4)] + [(NAMES[1], 0)]


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("name,site", _MODEL_SITES, ids=[f"{n}-{i}" for n, i in _MODEL_SITES])
def test_odconv_site_in_the_model_matches_the_block_reference(models, name, site, dt):
    """The GPU's own map before an ODConv site through odconv_block on the CPU
    (float64, and the emulation of the declared roundings) against the GPU's
    map after it, under the block rule: this isolates the block, with the
    model's weights and activations, from the convs around it.
    Measured on an MI355X over the ten cases: relative L2 at 0.27 .. 0.31 of its
    allowance, max|d| at 0.23 .. 0.25."""
    p, bn, c, H, pool = R.SITES[name][site]
    crops = torch.from_numpy(make_crops(8, seed=41)).to(DEV)
    m = models(name, dt)
    if p == "odconv":
        before, after = "features1", "odconv"
    else:
        after = [i + 1 for i, l in enumerate(R.LAYERS[name]) if f"{l[0]}.{l[1]}" == p][0]
        before = after - 1
    with torch.no_grad():
        f = m.stem_features(crops, u8=True, upto=before).cpu()
        got = m.stem_features(crops, u8=True, upto=after)
    assert tuple(f.shape[1:]) == (H, H, c)
    ops = R.odconv_fold(_sd_t(name), p, bn)
    relu = bn is not None
    x = _nchw(f)
    with torch.no_grad():
        ref = R.odconv_block(x, ops, torch.float64, relu=relu, pool=pool)
        emu = R.odconv_block(x.float(), ops, torch.float32, round=dt, relu=relu, pool=pool).double()
    l2r, mxr, l2, mx = _rule1(_nchw(got.cpu()), ref, emu, dt)
    print(f"{name} {p} {dt}: relative L2 {l2:.3e} at {l2r:.3f} of its allowance, max|d| {mx:.3e} at {mxr:.3f}")
    assert l2r <= 1 and mxr <= 1, (l2r, mxr)


@pytest.mark.parametrize("name", NAMES)
def test_u8_and_nchw_paths_agree(models, name):
    crops = make_crops(3, seed=43)
    m = models(name, "fp16")
    with torch.no_grad():
        a = m.forward_u8(torch.from_numpy(crops).to(DEV))
        b = m(normalize_u8(crops).to(DEV))
        torch.cuda.synchronize()
        assert torch.equal(a, b)
        with pytest.raises(RuntimeError):      # the reference's pos_embedding[0:B] past 32 crops
            m.forward_u8(torch.zeros(33, 224, 224, 3, dtype=torch.uint8, device=DEV))


@pytest.mark.parametrize("name", NAMES)
def test_graph_replay_matches_eager(models, name):
    crops = torch.from_numpy(make_crops(8, seed=45)).to(DEV)
    slots = torch.arange(8, dtype=torch.int32, device=DEV) * 3 % 32
    m = models(name, "bf16")
    m.reserve(8, DEV)                               # the scratch is then fixed before the capture
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


@pytest.mark.parametrize("name", NAMES)
def test_reserve_then_two_forwards_allocate_nothing_new(models, name):
    """After reserve(B) and one forward at that batch, a second forward of B
    crops takes no new memory from the device, and the block's scratch is the
    buffer reserve() made, sized for the largest site."""
    m = models(name, "fp16")
    m.reserve(8, DEV)
    scratch, outgrown = m._odconv_scratch, len(m._odconv_outgrown)
    assert scratch is not None
    assert scratch.numel() >= max(_lib.load().fac_odconv_scratch_bytes(8, H, H, c) for _p, _bn, c, H, _pool in R.SITES[name])
    crops = torch.from_numpy(make_crops(8, seed=46)).to(DEV)
    with torch.no_grad():
        first = m.forward_u8(crops)
        torch.cuda.synchronize()
        before = torch.cuda.memory_reserved()
        again = m.forward_u8(crops)
        torch.cuda.synchronize()
    assert torch.cuda.memory_reserved() == before and torch.equal(first, again)
    assert m._odconv_scratch is scratch and len(m._odconv_outgrown) == outgrown and m._scconv_scratch is None


def test_predict_video_takes_the_model(models):
    """video.predict_video on a 30-frame synthetic video (3 crops): the logits
    of the model on those crops, and prediction.predict_crops' score up to the
    device sigmoid's last bit."""
    from fac_fake_amd.prediction import chunk_slots, predict_crops
    from fac_fake_amd.video import crop_faces, predict_video, reference_boxes, synthetic_video
    frames, boxes = synthetic_video(30, 360, 640, seed=3, device=DEV)
    m = models(NAMES[1], "fp16")
    score, logits = predict_video(m, frames, boxes, return_logits=True)
    sel = reference_boxes(boxes, 30)
    crops = crop_faces(frames, sel)
    with torch.no_grad():
        want = m.forward_u8(crops, pos_index=torch.from_numpy(chunk_slots(len(sel))))
    assert len(sel) == 3 and torch.equal(logits, want)
    assert abs(score - predict_crops(m, crops)) <= 1e-6


def test_the_unused_odconv_weights_do_not_reach_the_output():
    """cvit_GGCA_ADD_ODConv's top-level odconv is in the state_dict and never
    called: other values under odconv.* leave the logits bitwise unchanged, and
    the keys are kept.  (In cvit_GGCA_ODConv the same keys are the block that
    runs, and changing them changes the logits.)"""
    from fac_fake_amd import odconv
    crops = torch.from_numpy(make_crops(2, seed=47)).to(DEV)
    for name, unused in ((NAMES[0], True), (NAMES[1], False)):
        m = odconv.CViT(name, dtype="fp16")
        sd = _sd_t(name)
        m.load_state_dict(sd)
        m.to(DEV)
        with torch.no_grad():
            a = m.forward_u8(crops).clone()
            other = {k: (v * 0.5 + 0.25 if k.startswith("odconv.") and v.is_floating_point() and v.dim() > 0 else v) for k, v in sd.items()}
            m.load_state_dict(other)
            b = m.forward_u8(crops).clone()
            torch.cuda.synchronize()
        assert torch.equal(m.state_dict()["odconv.weight"].cpu(), other["odconv.weight"])
        assert torch.equal(a, b) == unused, name
        m._release()
