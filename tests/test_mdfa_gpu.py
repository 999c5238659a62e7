"""The MDFA block and the three MDFA CViT classes on the GPU: fac_mdfa
(mdfa.hip) against a float64 reference of its own arithmetic
(tests/mdfa_ref.py), and the drop-ins of fac_fake_amd/mdfa.py against the
reference classes' recorded outputs (tests/golden/mdfa_*,
tools/make_golden_mdfa.py).
"""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import mdfa_ref as R  # noqa: E402
from fac_fake_amd import _lib  # noqa: E402
from fac_fake_amd.weights import make_crops, make_mdfa_state_dict  # noqa: E402
from oracle.cvit_torch import normalize_u8  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
# |got - ref| / max(|ref|, 1e-3): twice the half-ulp of the one output rounding (KERNEL_BOUND of test_bfm_gpu.py)
KERNEL_BOUND = {"fp16": 2 ** -10 + 1e-5, "bf16": 2 ** -7 + 1e-5}
# (n, h, w, c): the smallest legal map and width, where only the corner pixels see a d = 6 tap; non-square, d = 12
# kept along w only, 117 rows per crop; MDFA(256)'s shape, whose 980 rows make the 32-row wave tiles straddle crops;
# MDFA(512)'s shape, 147 rows; a single crop with fewer rows than a workgroup's 128.
SHAPES = [(2, 7, 7, 64), (3, 9, 13, 128), (5, 14, 14, 256), (3, 7, 7, 512), (1, 7, 7, 512)]
SID = lambda s: "x".join(map(str, s))  # noqa: E731
SHAPE_ERR, ARG_ERR = -2, -1
GUARD = 256                                       # bytes; keeps the 16-byte alignment


@functools.lru_cache(maxsize=None)
def _input(shape, dt):
    """test_bfm_gpu.py's: signed, every seventh channel all-negative; NHWC 16-bit."""
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
def _operands(shape, dt, side="both"):
    """Random fac_mdfa_pack operands (fp32), the 16-bit ones already on the
    16-bit grid so that the float64 reference and the kernel use the same
    values: symmetric-uniform conv weights of about unit gain per branch,
    biases of both signs, a symmetric w_s.  w_t >= 0 is scaled, from the
    float64 reference alone, so that the mean t_b over the crops is the median
    of s_p: both sides of max(t_b, s_p) then occur on this input.
    side "s": w_t = 0, so m = s.  side "t": w_s strongly negative, so m = t_b."""
    c = shape[3]
    g = torch.Generator().manual_seed(2100 + c)
    u = lambda *s, a=1.0: (torch.rand(*s, generator=g) * 2 - 1) * a  # noqa: E731
    ops = {"w1": u(c, c, a=(3.0 / c) ** 0.5)}
    for i in (2, 3, 4):
        ops[f"w{i}"] = u(c, c, 3, 3, a=(3.0 / (c * 4)) ** 0.5)
    ops.update(bias4=u(4, c, a=0.3), w5=u(c, c, a=(3.0 / c) ** 0.5), b5=u(c, a=0.3),
               wcat=u(c, 5 * c, a=(3.0 / (5 * c)) ** 0.5) * 0.5, bcat=u(c, a=0.3),
               ws=u(5 * c, a=(3.0 / (5 * c)) ** 0.5), wt=torch.rand(5 * c, generator=g) / (5 * c))
    ops = R.round_ops(ops, dt)
    if side == "s":
        ops["wt"] = torch.zeros(5 * c)
    elif side == "t":
        ops["ws"] = -ops["ws"].abs() * 40 - 1.0
    else:
        with torch.no_grad():
            _, p = R.mdfa_block(_nchw(_input(shape, dt), torch.float64), ops, parts=True)
        ops["wt"] = (ops["wt"].double() * (p["s"].median() / p["t"].mean())).float()
    return ops


@functools.lru_cache(maxsize=None)
def _reference(shape, dt, side="both"):
    """(float64 reference, the CPU emulation of the kernel's two roundings, the
    share of pixels where t_b wins), NHWC, from the 16-bit inputs; computed once per case."""
    x, ops = _input(shape, dt), _operands(shape, dt, side)
    torch.set_num_threads(16)
    with torch.no_grad():
        ref, p = R.mdfa_block(_nchw(x, torch.float64), ops, parts=True)
        emu = R.mdfa_block(_nchw(x, torch.float32), ops, torch.float32, round=dt)
    share = float((p["t"].view(-1, 1, 1) > p["s"]).double().mean())
    return _nhwc(ref), _nhwc(emu.double()), share


_PACKED = {}


def _packed(ops, dt):
    from fac_fake_amd import mdfa
    key = (id(ops), dt)
    if key not in _PACKED:
        _PACKED[key] = (ops, mdfa.mdfa_pack(ops, dt, DEV))       # keeps ops alive: id() stays unique
    return _PACKED[key][1]


def _scratch(shape):
    return torch.empty(_lib.load().fac_mdfa_scratch_bytes(*shape), dtype=torch.uint8, device=DEV)


def _run(x16, packed, dt, shape=None, out=None, scratch=None, dtype_id=None):
    """fac_mdfa on a device tensor [n,h,w,c]; returns (status, out)."""
    n, h, w, c = shape or x16.shape
    if out is None:
        out = torch.empty(x16.shape, dtype=x16.dtype, device=DEV)
    if scratch is None:
        scratch = _scratch(tuple(x16.shape))
    rc = _lib.load().fac_mdfa(_lib.DTYPES[dt] if dtype_id is None else dtype_id, x16.data_ptr(), n, h, w, c,
                              packed.data_ptr(), out.data_ptr(), scratch.data_ptr(),
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out


def _rule1(got, ref, emu, dt):
    """The block rule (_rule1 of test_bfm_gpu.py): the GPU's error against the
    float64 reference measured by the CPU emulation's own error against it.
    Returns (relative L2 ratio, max|d| ratio), each against its allowance: 2x /
    4x the emulation's figure, never tighter than twice the half-ulp of the
    output rounding."""
    e_gpu, e_emu = got.double() - ref, emu - ref
    l2_allow = max(2 * float(e_emu.norm() / ref.norm()), KERNEL_BOUND[dt])
    mx_allow = max(4 * float(e_emu.abs().max()), KERNEL_BOUND[dt] * float(ref.abs().max()))
    return float(e_gpu.norm() / ref.norm()) / l2_allow, float(e_gpu.abs().max()) / mx_allow


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_mdfa_vs_float64_reference(shape, dt):
    """fac_mdfa against mdfa_block(float64) on the same 16-bit inputs and
    weights.  The yardstick is the CPU emulation of the two rounding points
    (mdfa_block(round=dt)): relative L2 within 2x its error, max|d| within 4x,
    never tighter than KERNEL_BOUND.  In every case's reference the channel
    gate t_b wins max(t_b, s_p) on 20 .. 80 % of the pixels, so a kernel that
    drops either side of the max cannot pass.
    Measured on an MI355X over the 10 cases: relative L2 2.68e-4 .. 2.83e-4
    (fp16) and 2.14e-3 .. 2.29e-3 (bf16), 0.272 .. 0.292 of the allowance;
    max|d| equals the emulation's, 0.250 of the allowance, in every case but
    (1,7,7,512) fp16 at 0.240; t wins on 0.496 .. 0.520 of the pixels."""
    x = _input(shape, dt)
    ops = _operands(shape, dt)
    rc, got = _run(x.to(DEV), _packed(ops, dt), dt)
    assert rc == 0
    ref, emu, share = _reference(shape, dt)
    assert got.shape == ref.shape and 0.2 <= share <= 0.8, share
    l2, mx = _rule1(got.cpu(), ref, emu, dt)
    e = got.cpu().double() - ref
    print(f"{shape} {dt}: t wins on {share:.3f}; relative L2 {float(e.norm() / ref.norm()):.3e} at {l2:.3f} of its "
          f"allowance, max|d| {float(e.abs().max()):.3e} at {mx:.3f}")
    assert torch.isfinite(got.float()).all()
    assert l2 <= 1 and mx <= 1, (shape, dt, l2, mx)


def _count_ops(c, bias2=0.0):
    ops = dict(w1=torch.full((c, c), 1.0 / c), bias4=torch.zeros(4, c), w5=torch.full((c, c), 1.0 / c), b5=torch.zeros(c),
               wcat=torch.full((c, 5 * c), 1.0 / c), bcat=torch.zeros(c), ws=torch.zeros(5 * c), wt=torch.zeros(5 * c))
    for i in (2, 3, 4):
        ops[f"w{i}"] = torch.full((c, c, 3, 3), 1.0 / c)
    ops["bias4"][1] = bias2
    return ops


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", [(2, 7, 7, 64), (3, 9, 13, 128), (2, 14, 14, 256)], ids=SID)
def test_padding_contributes_zero(shape, dt):
    """x = 1, every branch weight 1 / c, biases 0, identity BatchNorm, w_s =
    w_t = 0 (so m = max(0, sigmoid(0)) = 0.5) and conv_cat's weight 1 / c: the
    branches are 1, v6, v12, v18 (the pixel's in-map tap counts) and g = 1, so
    every output is 0.5 (2 + v6^2 + v12^2 + v18^2), at most 122.5 and exact in
    both dtypes (the CPU emulation confirms it), compared element by element,
    corners included.  A halo that picked up a neighbouring crop, a wrapped row
    or a bias would count a tap too many.  Then a bias of 3 on the d = 6
    branch alone shows up once per pixel, (v6 + 3)^2, not once per tap."""
    from fac_fake_amd import mdfa
    n, h, w, c = shape
    x = torch.ones(n, h, w, c).to(T16[dt])
    v = [R.in_map_taps(h, w, d) for d in R.DILATIONS]
    assert v[0][0, 0] == 4 and v[0][h // 2, w // 2] == (9 if h >= 13 else 1 if w < 13 else 3) and bool((v[2] == 1).all())
    for bias2 in (0.0, 3.0):
        ops = _count_ops(c, bias2)
        want = (0.5 * (2 + (v[0] + bias2) ** 2 + v[1] ** 2 + v[2] ** 2)).view(1, h, w, 1).expand(n, h, w, c)
        assert float(want.max()) <= 122.5
        with torch.no_grad():
            emu = _nhwc(R.mdfa_block(_nchw(x, torch.float32), R.round_ops(ops, dt), torch.float32, round=dt))
        assert torch.equal(emu.double(), want)
        rc, got = _run(x.to(DEV), mdfa.mdfa_pack(ops, dt, DEV), dt)
        assert rc == 0 and torch.equal(got.cpu().double(), want), bias2


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("side", ["s", "t"])
def test_each_side_of_the_max(side, dt):
    """w_t = 0: t_b = 0 and m = s_p everywhere.  w_s strongly negative: s_p ~ 0
    and m = t_b everywhere.  Each against the float64 reference under the block rule.
    Measured on an MI355X: m = s at 0.286 (fp16) / 0.291 (bf16) of the relative
    L2 allowance, m = t at 0.264 / 0.265; max|d| at 0.250 in all four."""
    shape = (3, 9, 13, 128)
    x = _input(shape, dt)
    ops = _operands(shape, dt, side)
    rc, got = _run(x.to(DEV), _packed(ops, dt), dt)
    assert rc == 0
    ref, emu, share = _reference(shape, dt, side)
    assert share == (0.0 if side == "s" else 1.0)
    l2, mx = _rule1(got.cpu(), ref, emu, dt)
    print(f"m = {side} {dt}: relative L2 at {l2:.3f} of its allowance, max|d| at {mx:.3f}; mean output "
          f"{float(got.float().mean()):.3f}")
    assert float(got.float().mean()) > 0.01 and l2 <= 1 and mx <= 1, (side, dt, l2, mx)


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", [(5, 14, 14, 256), (5, 7, 7, 512)], ids=SID)
def test_a_crop_does_not_depend_on_its_batch(shape, dt):
    x = _input(shape, dt).to(DEV)
    pk = _packed(_operands(shape, dt), dt)
    rc5, five = _run(x, pk, dt)
    assert rc5 == 0
    for i in (0, 3, 4):
        rc1, one = _run(x[i:i + 1].contiguous(), pk, dt)
        assert rc1 == 0 and torch.equal(five[i:i + 1].view(torch.int16), one.view(torch.int16)), i


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_nothing_is_written_outside_out_or_the_scratch(shape, dt):
    """out and the scratch carved from larger device buffers filled with a
    pattern: the guard bytes on both sides of each are unchanged, the result is
    the plain call's and x is unchanged."""
    x = _input(shape, dt).to(DEV)
    keep = x.clone()
    pk = _packed(_operands(shape, dt), dt)
    nb, ns = x.numel() * 2, _lib.load().fac_mdfa_scratch_bytes(*shape)
    assert ns > 0 and ns % 16 == 0
    obuf = torch.full((GUARD + nb + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    sbuf = torch.full((GUARD + ns + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    out = obuf[GUARD:GUARD + nb].view(T16[dt]).view(x.shape)
    rc, got = _run(x, pk, dt, out=out, scratch=sbuf[GUARD:GUARD + ns])
    assert rc == 0
    assert bool((obuf[:GUARD] == 0x5A).all()) and bool((obuf[GUARD + nb:] == 0x5A).all())
    assert bool((sbuf[:GUARD] == 0x5A).all()) and bool((sbuf[GUARD + ns:] == 0x5A).all())
    assert torch.equal(got.view(torch.int16), _run(x, pk, dt)[1].view(torch.int16))
    assert torch.equal(x.view(torch.int16), keep.view(torch.int16))


def test_error_returns():
    """Every rejected call returns before a launch: out keeps its pattern.  Argument checks only."""
    dt = "fp16"
    lib = _lib.load()
    x = torch.zeros(1, 16, 16, 512, dtype=torch.float16, device=DEV)
    out = torch.full_like(x, 7.0)
    pk = _packed(_operands((2, 7, 7, 64), dt), dt)
    scr = _scratch((1, 14, 14, 512))
    run = lambda shape, **kw: _run(x, pk, dt, shape=shape, out=out, scratch=scr, **kw)[0]  # noqa: E731
    for bad in ((1, 6, 7, 64), (1, 15, 7, 64), (1, 7, 6, 64), (1, 7, 15, 64), (1, 7, 7, 96), (1, 7, 7, 32), (1, 7, 7, 1024)):
        assert run(bad) == SHAPE_ERR, bad
        assert lib.fac_mdfa_scratch_bytes(*bad) == 0, bad
    assert run((0, 7, 7, 64)) == ARG_ERR
    assert run((-1, 7, 7, 64)) == ARG_ERR
    assert run((1, 7, 7, 64), dtype_id=2) == ARG_ERR
    assert lib.fac_mdfa_scratch_bytes(0, 7, 7, 64) == 0
    st = torch.cuda.current_stream().cuda_stream
    args = lambda xp, pp, op, sp: (1, xp, 1, 7, 7, 64, pp, op, sp, st)  # noqa: E731
    X, P, O, S = x.data_ptr(), pk.data_ptr(), out.data_ptr(), scr.data_ptr()
    assert lib.fac_mdfa(*args(None, P, O, S)) == ARG_ERR
    assert lib.fac_mdfa(*args(X, None, O, S)) == ARG_ERR
    assert lib.fac_mdfa(*args(X, P, None, S)) == ARG_ERR
    assert lib.fac_mdfa(*args(X, P, O, None)) == ARG_ERR
    # the branch kernel reads halos: not in place, and no partial overlap either
    assert lib.fac_mdfa(*args(O, P, O, S)) == ARG_ERR
    assert lib.fac_mdfa(*args(O + 64, P, O, S)) == ARG_ERR
    # x, the packed blob, out and the scratch must be 16-byte aligned
    assert lib.fac_mdfa(*args(X + 2, P, O, S)) == ARG_ERR
    assert lib.fac_mdfa(*args(X, P + 8, O, S)) == ARG_ERR
    assert lib.fac_mdfa(*args(X, P, O + 2, S)) == ARG_ERR
    assert lib.fac_mdfa(*args(X, P, O, S + 4)) == ARG_ERR
    c = 64
    host = [torch.zeros(n) for n in (c * c, 9 * c * c, 9 * c * c, 9 * c * c, 4 * c, c * c, c, 5 * c * c, c, 5 * c, 5 * c)]
    ptrs = [t.data_ptr() for t in host]
    blob = torch.zeros(lib.fac_mdfa_packed_bytes(c), dtype=torch.uint8)
    assert lib.fac_mdfa_pack(2, c, *ptrs, blob.data_ptr()) == ARG_ERR
    assert lib.fac_mdfa_pack(1, 96, *ptrs, blob.data_ptr()) == SHAPE_ERR
    assert lib.fac_mdfa_pack(1, c, None, *ptrs[1:], blob.data_ptr()) == ARG_ERR
    assert lib.fac_mdfa_pack(1, c, *ptrs, None) == ARG_ERR
    assert lib.fac_mdfa_pack(1, c, *ptrs, blob.data_ptr()) == 0
    sizes = [lib.fac_mdfa_packed_bytes(k) for k in (32, 64, 96, 128, 256, 512, 1024)]
    assert [s > 0 for s in sizes] == [False, True, False, True, True, True, False]
    assert sizes[1] >= (28 + 4) * c * c * 2 + 2 * c * c * 4
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert run((1, 7, 7, 64)) == 0                # and the legal call next to them runs


# ---------------------------------------------------------------- the drop-ins
def _sd_t(name):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in make_mdfa_state_dict(name, 0).items()}


@pytest.fixture(scope="module")
def models():
    """The drop-in per (class, dtype), built on first use, released when the module is done."""
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from fac_fake_amd import mdfa
    built = {}

    def get(name, dt):
        if (name, dt) not in built:
            m = mdfa.CViT(name, dtype=dt)
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
    class and dtype (test_mdfa.py holds the emulation to 1.25x).
    Measured on an MI355X, max|dp| of the allowance: cvit_GGCA4_MDFA5 fp16
    4.8e-4 of 8.0e-4, bf16 1.7e-3 of 2.9e-3; cvit_MDFA_BFM 3.9e-4 of 6.4e-4 and
    3.0e-3 of 8.2e-3; cvit_BFM_MDFA 3.1e-4 of 1.0e-3 and 1.2e-3 of 4.9e-3."""
    g = golden("mdfa_golden.npz")
    tol = 2 * golden("mdfa_envelope.json")[name][dt]
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


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("name", R.NAMES)
def test_mdfa_map_in_the_model_matches_the_block_reference(models, name, dt):
    """The GPU's own map before the mdfa step through mdfa_block on the CPU
    against the GPU's map after it, under the block rule of
    test_mdfa_vs_float64_reference: this isolates the block, with the model's
    weights and activations, from the convs before it.
    Measured on an MI355X over the six cases: relative L2 at 0.239 .. 0.243 of
    its allowance, max|d| at 0.250; t wins on 0.520 .. 0.528 of the pixels."""
    from fac_fake_amd.variants import steps_upto
    crops = torch.from_numpy(make_crops(2, seed=44)).to(DEV)
    m = models(name, dt)
    with torch.no_grad():
        m.forward_u8(crops)   # prepares the packed layers
        plan = [s for s, _run_, _ops in m._steps]
        k = steps_upto(plan, "mdfa")
        f = m._walk(crops, True, m._steps[:k - 1]).cpu()
        got = m.stem_features(crops, u8=True, upto="mdfa").cpu()
    site, c = m.table["mdfa"]
    hw = 14 if site == "features1" else 7
    assert tuple(f.shape) == (2, hw, hw, c) and got.shape == f.shape and plan[k - 1].kind == "mdfa"
    ops = R.round_ops(R.mdfa_fold(make_mdfa_state_dict(name, 0)), dt)
    with torch.no_grad():
        ref, p = R.mdfa_block(_nchw(f, torch.float64), ops, parts=True)
        emu = _nhwc(R.mdfa_block(_nchw(f, torch.float32), ops, torch.float32, round=dt).double())
    share = float((p["t"].view(-1, 1, 1) > p["s"]).double().mean())
    l2, mx = _rule1(got, _nhwc(ref), emu, dt)
    print(f"MDFA in {name} {dt}: t wins on {share:.3f}; relative L2 at {l2:.3f} of its allowance, max|d| at {mx:.3f}")
    assert 0.2 <= share <= 0.8 and l2 <= 1 and mx <= 1, (share, l2, mx)


@pytest.mark.parametrize("name", R.NAMES)
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


def test_graph_replay_matches_eager(models):
    crops = torch.from_numpy(make_crops(8, seed=45)).to(DEV)
    slots = torch.arange(8, dtype=torch.int32, device=DEV) * 3 % 32
    m = models("cvit_BFM_MDFA", "bf16")
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


@pytest.mark.parametrize("name", R.NAMES)
def test_reserve_then_two_forwards_allocate_nothing_new(models, name):
    """After reserve(B) and one forward at that batch, a second forward of B
    crops takes no new memory from the device, and the block's scratch is the
    buffer reserve() made."""
    m = models(name, "fp16")
    m.reserve(8, DEV)
    scratch, outgrown = m._mdfa_scratch, len(m._mdfa_outgrown)
    assert scratch is not None and m._mdfa is not None
    assert scratch.numel() >= _lib.load().fac_mdfa_scratch_bytes(8, *((14, 14, 256) if m.table["mdfa"][1] == 256 else (7, 7, 512)))
    crops = torch.from_numpy(make_crops(8, seed=46)).to(DEV)
    with torch.no_grad():
        first = m.forward_u8(crops)
        torch.cuda.synchronize()
        before = torch.cuda.memory_reserved()
        again = m.forward_u8(crops)
        torch.cuda.synchronize()
    assert torch.cuda.memory_reserved() == before and torch.equal(first, again)
    assert m._mdfa_scratch is scratch and len(m._mdfa_outgrown) == outgrown and m._smfa_scratch is None


def test_predict_video_takes_the_model(models):
    """video.predict_video on a 30-frame synthetic video (3 crops): the logits
    of the model on those crops, and prediction.predict_crops' score up to the
    device sigmoid's last bit."""
    from fac_fake_amd.prediction import chunk_slots, predict_crops
    from fac_fake_amd.video import crop_faces, predict_video, reference_boxes, synthetic_video
    frames, boxes = synthetic_video(30, 360, 640, seed=3, device=DEV)
    m = models("cvit_GGCA4_MDFA5", "fp16")
    score, logits = predict_video(m, frames, boxes, return_logits=True)
    sel = reference_boxes(boxes, 30)
    crops = crop_faces(frames, sel)
    with torch.no_grad():
        want = m.forward_u8(crops, pos_index=torch.from_numpy(chunk_slots(len(sel))))
    assert len(sel) == 3 and torch.equal(logits, want)
    assert abs(score - predict_crops(m, crops)) <= 1e-6
