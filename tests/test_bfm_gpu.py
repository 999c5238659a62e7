"""cvit_GGCA4_BFM5 on the GPU: fac_bfm (bfm.hip) against a float64 reference
of its own arithmetic (tests/bfm_ref.py) and against the same block composed
from fac_conv_nd and fac_ew launches, and the drop-in of fac_fake_amd/bfm.py
against the reference class's recorded outputs (tests/golden/bfm_*,
tools/make_golden_bfm.py).
"""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import bfm_ref as R  # noqa: E402
from fac_fake_amd import _lib  # noqa: E402
from fac_fake_amd.weights import make_bfm_state_dict, make_crops, uniform  # noqa: E402
from oracle.cvit_torch import normalize_u8  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAME = "cvit_GGCA4_BFM5"
T16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
# |got - ref| / max(|ref|, 1e-3): twice the half-ulp of the one output rounding (KERNEL_BOUND of test_other_gpu.py)
KERNEL_BOUND = {"fp16": 2 ** -10 + 1e-5, "bf16": 2 ** -7 + 1e-5}
# (n, h, w, c): the smallest legal map and width, where every window leaves the map; odd, non-square, 117 rows per
# crop; BFM(256)'s shape, whose 980 rows make the 32-row wave tiles straddle crops and leave the last one partly
# empty; BFM(512)'s shape, 147 rows; a single crop with fewer rows than a workgroup's 128.
SHAPES = [(2, 7, 7, 64), (3, 9, 13, 128), (5, 14, 14, 256), (3, 7, 7, 512), (1, 7, 7, 512)]
SID = lambda s: "x".join(map(str, s))  # noqa: E731
SHAPE_ERR, ARG_ERR = -2, -1


@functools.lru_cache(maxsize=None)
def _operands(c, dt):
    """Random fac_bfm_pack operands (fp32): symmetric-uniform weights of about
    unit gain per conv, already on the 16-bit grid so that the float64
    reference and the kernel use the same values; biases of both signs."""
    g = torch.Generator().manual_seed(1300 + c)
    u = lambda *s, a=1.0: (torch.rand(*s, generator=g) * 2 - 1) * a  # noqa: E731
    ops = {f"w{k}": R.round_to(u(c, c, k, k, a=(3.0 / (c * k * k)) ** 0.5), dt) for k in R.KS}
    ops["bias3"] = u(3, c, a=0.3)
    return ops


@functools.lru_cache(maxsize=None)
def _input(shape, dt):
    """test_other_gpu.py's: signed, every seventh channel all-negative; NHWC 16-bit."""
    n, h, w, c = shape
    g = torch.Generator().manual_seed(17 + h * w + c)
    x = torch.randn(n, h, w, c, generator=g) * 1.5
    x[..., ::7] = -x[..., ::7].abs() - 0.25
    return x.to(T16[dt])


def _nchw(x16, dtype):
    return x16.to(dtype).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def _reference(shape, dt, scale):
    """(float64 reference, the CPU emulation of the kernel's one rounding, the
    emulation of the composed route's four, the mixed-sign share), NHWC, from
    the 16-bit inputs; computed once per case."""
    x, ops = _input(shape, dt), _operands(shape[3], dt)
    torch.set_num_threads(16)
    with torch.no_grad():
        ref = R.bfm_block(_nchw(x, torch.float64), ops, scale)
        emu = R.bfm_block(_nchw(x, torch.float32), ops, scale, dtype=torch.float32, round=dt)
        emc = R.bfm_block(_nchw(x, torch.float32), ops, scale, dtype=torch.float32, round=dt, route="composed")
        mixed = R.bfm_mixed_sign(_nchw(x, torch.float64), ops)
    return _nhwc(ref), _nhwc(emu.double()), _nhwc(emc.double()), mixed


_PACKED = {}


def _packed(ops, dt):
    from fac_fake_amd import bfm
    key = (id(ops), dt)
    if key not in _PACKED:
        _PACKED[key] = (ops, bfm.bfm_pack(ops, dt, DEV))         # keeps ops alive: id() stays unique
    return _PACKED[key][1]


def _run(x16, ops, dt, scale=4.0, shape=None, out=None, packed=None, dtype_id=None):
    """fac_bfm on a device tensor [n,h,w,c]; returns (status, out)."""
    n, h, w, c = shape or x16.shape
    wpk, bias3 = packed or _packed(ops, dt)
    if out is None:
        out = torch.empty(x16.shape, dtype=x16.dtype, device=DEV)
    rc = _lib.load().fac_bfm(_lib.DTYPES[dt] if dtype_id is None else dtype_id, x16.data_ptr(), n, h, w, c,
                             wpk.data_ptr(), bias3.data_ptr(), float(scale), out.data_ptr(),
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out


def _rule1(got, ref, emu, dt):
    """The block rule (_rule1 of test_other_gpu.py): the GPU's error against
    the float64 reference measured by the CPU emulation's own error against
    it.  Returns (relative L2 ratio, max|d| ratio), each against its allowance:
    2x / 4x the emulation's figure, never tighter than twice the half-ulp of
    the output rounding."""
    e_gpu, e_emu = got.double() - ref, emu - ref
    l2_allow = max(2 * float(e_emu.norm() / ref.norm()), KERNEL_BOUND[dt])
    mx_allow = max(4 * float(e_emu.abs().max()), KERNEL_BOUND[dt] * float(ref.abs().max()))
    return float(e_gpu.norm() / ref.norm()) / l2_allow, float(e_gpu.abs().max()) / mx_allow


CASES = [(s, 4.0) for s in SHAPES] + [((3, 9, 13, 128), 1.0)]
CID = lambda c: f"{SID(c[0])}-scale{c[1]:g}"  # noqa: E731


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=CID)
def test_bfm_vs_float64_reference(case, dt):
    """scale * sum_k ReLU(conv_k(x) + b_k) against bfm_block(float64) on the
    same 16-bit inputs and weights.  The yardstick is the CPU emulation of the
    one rounding point (bfm_block(round=dt)): relative L2 within 2x its error,
    max|d| within 4x, never tighter than KERNEL_BOUND.  Every case's reference
    has at least 25 % of its elements with pre-activations of mixed sign across
    the three convs (74-75 % on the CPU), so a kernel that merges the convs
    before the ReLU cannot pass.
    Measured on an MI355X over the 12 cases: relative L2 2.06e-4 .. 2.08e-4
    (fp16) and 1.63e-3 .. 1.66e-3 (bf16), 0.209 .. 0.213 of the allowance
    (KERNEL_BOUND sets it); max|d| equals the emulation's, 0.250 of the
    allowance, in every case but (2,7,7,64) bf16 at 0.211; mixed-sign shares
    0.744 .. 0.754."""
    shape, scale = case
    x = _input(shape, dt)
    rc, got = _run(x.to(DEV), _operands(shape[3], dt), dt, scale)
    assert rc == 0
    ref, emu, _emc, mixed = _reference(shape, dt, scale)
    assert got.shape == ref.shape and mixed >= 0.25, mixed
    l2, mx = _rule1(got.cpu(), ref, emu, dt)
    e = got.cpu().double() - ref
    print(f"{shape} scale {scale:g} {dt}: mixed-sign share {mixed:.3f}; relative L2 {float(e.norm() / ref.norm()):.3e} at "
          f"{l2:.3f} of its allowance, max|d| {float(e.abs().max()):.3e} at {mx:.3f}")
    assert torch.isfinite(got.float()).all()
    assert l2 <= 1 and mx <= 1, (shape, scale, dt, l2, mx)


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_bfm_vs_the_composed_route(shape, dt):
    """A second witness that shares no kernel code: three fac_conv_nd /
    fac_conv3x3 launches with ReLU, fac_ew add3 and the scale
    (bfm.bfm16_composed).  Each route is within its own allowance of the
    float64 reference, the fused kernel against the emulation of its one
    rounding, the composed route against the emulation of its four.
    Measured on an MI355X over the 10 cases: the composed route at 0.261 ..
    0.269 (relative L2) and 0.250 (max|d|) of its allowance; the two routes
    differ by 2.8e-4 .. 2.9e-4 (fp16) and 2.3e-3 .. 2.4e-3 (bf16) in relative L2."""
    from fac_fake_amd import bfm
    x, ops = _input(shape, dt).to(DEV), _operands(shape[3], dt)
    rc, fused = _run(x, ops, dt)
    assert rc == 0
    with torch.no_grad():
        comp = bfm.bfm16_composed(x, ops, dt, 4.0)
    torch.cuda.synchronize()
    ref, emu, emc, _ = _reference(shape, dt, 4.0)
    assert comp.shape == fused.shape == ref.shape
    lf, mf = _rule1(fused.cpu(), ref, emu, dt)
    lc, mc = _rule1(comp.cpu(), ref, emc, dt)
    d = (fused.double() - comp.double()).cpu()
    print(f"{shape} {dt}: fused at {lf:.3f} / {mf:.3f} of its allowance, composed at {lc:.3f} / {mc:.3f}; "
          f"fused vs composed relative L2 {float(d.norm() / ref.norm()):.3e}, max|d| {float(d.abs().max()):.3e}")
    assert lf <= 1 and mf <= 1 and lc <= 1 and mc <= 1, (shape, dt, lf, mf, lc, mc)


def _in_map_taps(h, w, k):
    ys, xs = torch.arange(h).view(h, 1), torch.arange(w).view(1, w)
    p = k // 2
    rows = torch.minimum(ys + p, torch.tensor(h - 1)) - torch.clamp(ys - p, min=0) + 1
    cols = torch.minimum(xs + p, torch.tensor(w - 1)) - torch.clamp(xs - p, min=0) + 1
    return (rows * cols).double()


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("shape,scale", [((2, 7, 7, 64), 4.0), ((3, 9, 13, 128), 1.0), ((2, 14, 14, 256), 4.0)],
                         ids=["2x7x7x64", "3x9x13x128", "2x14x14x256"])
def test_padding_contributes_zero(shape, scale, dt):
    """x = 1, b = 0 and every weight 1 / c: conv_k at a pixel is the number of
    in-map taps v_k of its k x k window, so every output is scale * (v3 + v5 +
    v7), exact in both dtypes (1 / c is a power of two, the sums are integers
    below 256), compared element by element, corners included.  A halo that
    picked up a neighbouring crop, a wrapped row or a bias would count a tap
    too many.  Then a large bias on the 5x5 conv alone shows up once per pixel,
    not once per tap."""
    n, h, w, c = shape
    ops = {f"w{k}": torch.full((c, c, k, k), 1.0 / c) for k in R.KS}
    ops["bias3"] = torch.zeros(3, c)
    x = torch.ones(n, h, w, c).to(T16[dt]).to(DEV)
    rc, got = _run(x, ops, dt, scale, packed=_fresh_pack(ops, dt))
    assert rc == 0
    v = sum(_in_map_taps(h, w, k) for k in R.KS)
    assert v[0, 0] == 4 + 9 + 16 and v[h // 2, w // 2] == 9 + 25 + 49
    want = (scale * v).view(1, h, w, 1).expand(n, h, w, c)
    assert torch.equal(got.cpu().double(), want)
    ops["bias3"][1] = 64.0
    rc, got = _run(x, ops, dt, scale, packed=_fresh_pack(ops, dt))
    assert rc == 0 and torch.equal(got.cpu().double(), want + scale * 64.0)


def _fresh_pack(ops, dt):
    from fac_fake_amd import bfm
    return bfm.bfm_pack(ops, dt, DEV)


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_each_conv_is_relued_alone(dt):
    """w5 = -w3 embedded in the 5x5 window's centre, w7 = 0 and zero biases:
    the output is scale * (ReLU(p) + ReLU(-p)) = scale * |conv3(x)|, where a
    kernel that sums before the ReLU gives 0."""
    shape = (3, 9, 13, 128)
    c = shape[3]
    base = _operands(c, dt)
    w5 = torch.zeros(c, c, 5, 5)
    w5[:, :, 1:4, 1:4] = -base["w3"]
    ops = dict(w3=base["w3"], w5=w5, w7=torch.zeros(c, c, 7, 7), bias3=torch.zeros(3, c))
    x = _input(shape, dt)
    rc, got = _run(x.to(DEV), ops, dt, 4.0, packed=_fresh_pack(ops, dt))
    assert rc == 0
    with torch.no_grad():
        p = torch.nn.functional.conv2d(_nchw(x, torch.float64), base["w3"].double(), padding=1)
        emu = R.round_to((4.0 * p.float().abs()), dt).double()
    ref = _nhwc(4.0 * p.abs())
    l2, mx = _rule1(got.cpu(), ref, _nhwc(emu), dt)
    print(f"|conv3| {dt}: relative L2 at {l2:.3f} of its allowance, max|d| at {mx:.3f}; mean output "
          f"{float(got.float().mean()):.3f}")
    assert float(got.float().mean()) > 1.0 and l2 <= 1 and mx <= 1


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", [(5, 14, 14, 256), (5, 7, 7, 512)], ids=SID)
def test_a_crop_does_not_depend_on_its_batch(shape, dt):
    x = _input(shape, dt).to(DEV)
    ops = _operands(shape[3], dt)
    rc5, five = _run(x, ops, dt)
    assert rc5 == 0
    for i in (0, 3, 4):
        rc1, one = _run(x[i:i + 1].contiguous(), ops, dt)
        assert rc1 == 0 and torch.equal(five[i:i + 1].view(torch.int16), one.view(torch.int16)), i


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_nothing_is_written_outside_out(shape, dt):
    """out carved from a larger device buffer filled with a pattern: the guard
    words on both sides are unchanged, the result is the plain call's and x is
    unchanged."""
    guard = 256                                   # bytes; keeps the 16-byte alignment
    x = _input(shape, dt).to(DEV)
    keep = x.clone()
    ops = _operands(shape[3], dt)
    obuf = torch.full((guard + x.numel() * 2 + guard,), 0x5A, dtype=torch.uint8, device=DEV)
    out = obuf[guard:guard + x.numel() * 2].view(T16[dt]).view(x.shape)
    rc, got = _run(x, ops, dt, out=out)
    assert rc == 0
    assert bool((obuf[:guard] == 0x5A).all()) and bool((obuf[guard + x.numel() * 2:] == 0x5A).all())
    assert torch.equal(got.view(torch.int16), _run(x, ops, dt)[1].view(torch.int16))
    assert torch.equal(x.view(torch.int16), keep.view(torch.int16))


def test_error_returns():
    """Every rejected call returns before a launch: out keeps its pattern.  Argument checks only."""
    dt = "fp16"
    lib = _lib.load()
    x = torch.zeros(1, 16, 16, 512, dtype=torch.float16, device=DEV)
    out = torch.full_like(x, 7.0)
    ops = _operands(64, dt)
    run = lambda shape, **kw: _run(x, ops, dt, shape=shape, out=out, **kw)[0]  # noqa: E731
    assert run((1, 6, 7, 64)) == SHAPE_ERR
    assert run((1, 15, 7, 64)) == SHAPE_ERR
    assert run((1, 7, 6, 64)) == SHAPE_ERR
    assert run((1, 7, 15, 64)) == SHAPE_ERR
    assert run((1, 7, 7, 96)) == SHAPE_ERR
    assert run((1, 7, 7, 32)) == SHAPE_ERR
    assert run((1, 7, 7, 1024)) == SHAPE_ERR
    assert run((0, 7, 7, 64)) == ARG_ERR
    assert run((-1, 7, 7, 64)) == ARG_ERR
    assert run((1, 7, 7, 64), dtype_id=2) == ARG_ERR
    wpk, b3 = _packed(ops, dt)
    st = torch.cuda.current_stream().cuda_stream
    args = lambda xp, wp, bp, op: (1, xp, 1, 7, 7, 64, wp, bp, 4.0, op, st)  # noqa: E731
    assert lib.fac_bfm(*args(None, wpk.data_ptr(), b3.data_ptr(), out.data_ptr())) == ARG_ERR
    assert lib.fac_bfm(*args(x.data_ptr(), None, b3.data_ptr(), out.data_ptr())) == ARG_ERR
    assert lib.fac_bfm(*args(x.data_ptr(), wpk.data_ptr(), None, out.data_ptr())) == ARG_ERR
    assert lib.fac_bfm(*args(x.data_ptr(), wpk.data_ptr(), b3.data_ptr(), None)) == ARG_ERR
    # the kernel reads halos: not in place, and no partial overlap either
    assert lib.fac_bfm(*args(out.data_ptr(), wpk.data_ptr(), b3.data_ptr(), out.data_ptr())) == ARG_ERR
    assert lib.fac_bfm(*args(out.data_ptr() + 64, wpk.data_ptr(), b3.data_ptr(), out.data_ptr())) == ARG_ERR
    # x, the packed weights, the biases and out must be 16-byte aligned
    assert lib.fac_bfm(*args(x.data_ptr() + 2, wpk.data_ptr(), b3.data_ptr(), out.data_ptr())) == ARG_ERR
    assert lib.fac_bfm(*args(x.data_ptr(), wpk.data_ptr() + 8, b3.data_ptr(), out.data_ptr())) == ARG_ERR
    assert lib.fac_bfm(*args(x.data_ptr(), wpk.data_ptr(), b3.data_ptr() + 4, out.data_ptr())) == ARG_ERR
    assert lib.fac_bfm(*args(x.data_ptr(), wpk.data_ptr(), b3.data_ptr(), out.data_ptr() + 2)) == ARG_ERR
    host = [torch.zeros(64 * 64 * k * k) for k in R.KS]
    pk = torch.zeros(83 * 64 * 64, dtype=torch.int16)
    ptrs = [t.data_ptr() for t in host]
    assert lib.fac_bfm_pack(2, 64, *ptrs, pk.data_ptr()) == ARG_ERR
    assert lib.fac_bfm_pack(1, 96, *ptrs, pk.data_ptr()) == SHAPE_ERR
    assert lib.fac_bfm_pack(1, 64, None, ptrs[1], ptrs[2], pk.data_ptr()) == ARG_ERR
    assert lib.fac_bfm_pack(1, 64, *ptrs, None) == ARG_ERR
    assert [lib.fac_bfm_packed_elems(c) for c in (32, 64, 96, 128, 256, 512, 1024)] == \
        [0, 83 * 64 * 64, 0, 83 * 128 * 128, 83 * 256 * 256, 83 * 512 * 512, 0]
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert run((1, 7, 7, 64)) == 0                # and the legal call next to them runs


# ---------------------------------------------------------------- the drop-in
def _sd_t(seed_tfam=None):
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in make_bfm_state_dict(NAME, 0).items()}
    if seed_tfam is not None:
        for k, v in sd.items():
            if ".tfam." in k:
                sd[k] = torch.from_numpy(uniform(k, v.numel(), seed_tfam).reshape(tuple(v.shape)).copy())
    return sd


@pytest.fixture(scope="module")
def models():
    """The drop-in per dtype, built on first use, released when the module is done."""
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from fac_fake_amd import bfm
    built = {}

    def get(dt):
        if dt not in built:
            m = bfm.CViT(NAME, dtype=dt)
            m.load_state_dict(_sd_t())
            m.to(DEV)
            built[dt] = m
        return built[dt]
    yield get
    torch.cuda.synchronize()
    for m in built.values():
        m._release()


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_model_matches_reference(golden, models, dt):
    """forward_u8 on the 4 golden crops against the reference class's fp32
    probabilities, within 2x the recorded 16-bit emulation envelope of that
    dtype (test_bfm.py holds the emulation to 1.25x).
    Measured on an MI355X: fp16 1.7e-4 of 4.7e-4 allowed, bf16 2.0e-3 of 4.8e-3."""
    g = golden("bfm_golden.npz")
    tol = 2 * golden("bfm_envelope.json")[NAME][dt]
    crops = torch.from_numpy(make_crops(4, seed=int(g["crop_seed"]))).to(DEV)
    with torch.no_grad():
        lg, pr = models(dt).forward_u8(crops, return_probs=True)
        torch.cuda.synchronize()
    lg, pr = lg.cpu().numpy(), pr.cpu().numpy()
    p_ref = 1 / (1 + np.exp(-g[f"{NAME}/logits"]))
    d = float(np.abs(pr - p_ref).max())
    print(f"{NAME} {dt}: max|dp| vs reference {d:.3e} (tolerance {tol:.3e})")
    assert np.isfinite(lg).all()
    assert d <= tol, (dt, d, tol)
    assert np.allclose(pr, 1 / (1 + np.exp(-lg)), atol=1e-6)


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_bfm_map_in_the_model_matches_the_block_reference(models, dt):
    """The GPU's own stem output [B,7,7,512] through bfm_block on the CPU
    against the GPU's map after the bfm step, under the block rule of
    test_bfm_vs_float64_reference: this isolates the block, with the model's
    weights and activations, from the 17 convs before it.  The yardstick is
    the emulation of the route the model's step takes (bfm.MODEL_ROUTE).
    Measured on an MI355X (composed route): relative L2 at 0.265 (fp16) and
    0.268 (bf16) of its allowance, max|d| at 0.250; mixed-sign share 0.762."""
    from fac_fake_amd import bfm
    assert bfm.MODEL_ROUTE == R.MODEL_ROUTE
    crops = torch.from_numpy(make_crops(2, seed=44)).to(DEV)
    m = models(dt)
    with torch.no_grad():
        m.forward_u8(crops)   # prepares the packed layers
        f = m.stem_features(crops, u8=True, upto=17).cpu()
        got = m.stem_features(crops, u8=True, upto="bfm").cpu()
        full = m.stem_features(crops, u8=True).cpu()
    assert tuple(f.shape) == (2, 7, 7, 512) and got.shape == f.shape
    assert torch.equal(got.view(torch.int16), full.view(torch.int16))          # bfm is the stem's last step
    ops = R.bfm_fold(make_bfm_state_dict(NAME, 0))
    ops = {k: (v if k == "bias3" else R.round_to(v, dt)) for k, v in ops.items()}
    with torch.no_grad():
        ref = _nhwc(R.bfm_block(_nchw(f, torch.float64), ops))
        emu = _nhwc(R.bfm_block(_nchw(f, torch.float32), ops, dtype=torch.float32, round=dt,
                                route=R.MODEL_ROUTE).double())
        mixed = R.bfm_mixed_sign(_nchw(f, torch.float64), ops)
    l2, mx = _rule1(got, ref, emu, dt)
    print(f"BFM(x, x) in the model {dt}: mixed-sign share {mixed:.3f}; relative L2 at {l2:.3f} of its allowance, "
          f"max|d| at {mx:.3f}")
    assert mixed >= 0.25 and l2 <= 1 and mx <= 1, (mixed, l2, mx)


def test_redrawing_the_tfam_tensors_changes_no_bit(models):
    """BFM(x, x) = 4 MSFE(x): the eight tfam.* tensors are loaded, kept and
    returned, and the logits do not depend on them."""
    from fac_fake_amd import bfm
    crops = torch.from_numpy(make_crops(3, seed=47)).to(DEV)
    a = models("fp16")
    b = bfm.CViT(NAME, dtype="fp16")
    sd2 = _sd_t(seed_tfam=7)
    b.load_state_dict(sd2)
    b.to(DEV)
    try:
        with torch.no_grad():
            la, lb = a.forward_u8(crops), b.forward_u8(crops)
            torch.cuda.synchronize()
        assert torch.equal(la, lb)
        back = b.state_dict()
        tf = [k for k in back if ".tfam." in k]
        assert len(tf) == 8 and all(torch.equal(back[k].cpu(), sd2[k]) for k in tf)
        assert any(not torch.equal(back[k].cpu(), a.state_dict()[k].cpu()) for k in tf)
    finally:
        b._release()


def test_u8_and_nchw_paths_agree(models):
    crops = make_crops(3, seed=43)
    m = models("fp16")
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
    m = models("bf16")
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


def test_reserve_then_a_forward_allocates_nothing_new(models):
    """After reserve(B) and one forward at that batch, a second forward of B
    crops takes no new memory from the device: the block has no scratch, its
    output comes from the caching allocator like every other step's."""
    m = models("fp16")
    m.reserve(8, DEV)
    crops = torch.from_numpy(make_crops(8, seed=46)).to(DEV)
    with torch.no_grad():
        first = m.forward_u8(crops)
        torch.cuda.synchronize()
        before = torch.cuda.memory_reserved()
        again = m.forward_u8(crops)
        torch.cuda.synchronize()
    assert torch.cuda.memory_reserved() == before and torch.equal(first, again)
    assert m._smfa_scratch is None and m._bfm is not None


def test_predict_video_takes_the_model(models):
    """video.predict_video on a 30-frame synthetic video (3 crops): the logits
    of the model on those crops, and prediction.predict_crops' score up to the
    device sigmoid's last bit."""
    from fac_fake_amd.prediction import chunk_slots, predict_crops
    from fac_fake_amd.video import crop_faces, predict_video, reference_boxes, synthetic_video
    frames, boxes = synthetic_video(30, 360, 640, seed=3, device=DEV)
    m = models("fp16")
    score, logits = predict_video(m, frames, boxes, return_logits=True)
    sel = reference_boxes(boxes, 30)
    crops = crop_faces(frames, sel)
    with torch.no_grad():
        want = m.forward_u8(crops, pos_index=torch.from_numpy(chunk_slots(len(sel))))
    assert len(sel) == 3 and torch.equal(logits, want)
    assert abs(score - predict_crops(m, crops)) <= 1e-6
