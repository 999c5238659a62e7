"""fac_ggca, fac_kan_linear, fac_pool_nd's generic routes, fac_pack_input,
fac_pack_input_s2d (fp32 source) and fac_sigmoid on the GPU against the fp64
references of tests/side_ops_ref.py, at the shapes where they can go wrong:
non-square maps, the LDS limits, partial chunks, values on and outside the
knots, padded windows over negative inputs, channel slots, clip batches.

The gates are those test_side_ops_ref.py shows plain fp32 torch meeting on
the same inputs; every output buffer the kernels do not own entirely is
pre-filled with a sentinel that must survive.
"""
import pytest
import torch

import side_ops_ref as R
from fac_fake_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T16 = R.T16
SENT = 77.0           # exactly representable in both 16-bit types
PAD = 64              # sentinel elements on either side of a flat output


def _case_id(c):
    return "x".join(map(str, c))


def _guarded(numel, dtype):
    """(buffer, view): `numel` elements with PAD sentinels before and after."""
    buf = torch.full((PAD + numel + PAD,), SENT, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + numel]


def _guards_intact(buf, numel):
    return bool((buf[:PAD] == SENT).all()) and bool((buf[PAD + numel:] == SENT).all())


# ---------------------------------------------------------------- GGCA
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("case", R.GGCA_CASES, ids=_case_id)
def test_ggca_vs_fp64(case, dt, torch_threads):
    """fac_ggca against the fp64 reference rounded once: <= 1 value of the 16-bit type everywhere, and
    different at all on <= 0.5 % of the outputs (plain fp32 torch: <= 0.1 %, test_side_ops_ref.py).
    Observed on an MI355X, worst of the six cases: fp16 0.091 % (2x1x15x256x1), bf16 0.022 % (2x5x7x64x2),
    never more than 1 value."""
    n, h, w, c, groups = case
    x16, prm = R.ggca_inputs(case, dt)
    ref = R.round16(R.ggca_ref(x16.permute(0, 3, 1, 2), *prm, groups), dt).permute(0, 2, 3, 1)
    xg = x16.contiguous().to(DEV)
    pg = [t.contiguous().to(DEV) for t in prm]
    buf, out = _guarded(x16.numel(), T16[dt])
    rc = _lib.load().fac_ggca(_lib.DTYPES[dt], xg.data_ptr(), n, h, w, c, groups, *(t.data_ptr() for t in pg),
                              out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, None, "fac_ggca")
    torch.cuda.synchronize()
    got = out.cpu().view(n, h, w, c)
    assert not bool(torch.isnan(got.float()).any())
    d = R.ulp_dist(got, ref.contiguous())
    share = float((d > 0).float().mean())
    print(f"ggca {case} {dt}: max {int(d.max())} ulp, share {share:.5f}")
    assert int(d.max()) <= 1 and share <= R.GGCA_FLIP_CAP_GPU, (int(d.max()), share)
    assert _guards_intact(buf, x16.numel())
    assert torch.equal(xg.cpu(), x16)                    # the input is read only


# ---------------------------------------------------------------- KANLinear
def _kan_check(y, y64, a, in_f, what):
    err, bound = (y.double() - y64).abs(), R.kan_bound(a, in_f)
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"kan {what}: max err/bound {ratio:.4f}")
    assert not bool(torch.isnan(y).any())
    assert bool((err <= bound).all()), ratio
    assert bool((y[a == 0] == 0).all())                  # rows whose features are all zero: exactly 0
    return ratio


@pytest.mark.parametrize("case", R.KAN_CASES, ids=_case_id)
def test_kan_linear_vs_fp64(case, torch_threads):
    """KANLinearLayer against fp64 within (9 in_f + 32) 2^-24 A per output (side_ops_ref.kan_bound), with x on
    every knot of a feature, outside the knots, +-0 and +-1e4, and partial row / input / output chunks.
    Observed max err / bound on an MI355X: 0.0037 (1x1x1), 0.0270 (33x40x70), 0.0168 (64x64x128),
    0.0009 (5x500x3)."""
    from fac_fake_amd.ops import KANLinearLayer
    x, grid, bw, sw, ss = R.kan_inputs(case)
    y64, a = R.kan_ref(x, grid, bw, sw, ss)
    layer = KANLinearLayer(grid, bw, sw, ss, DEV)
    y = layer(x.to(DEV))
    torch.cuda.synchronize()
    assert tuple(y.shape) == (case[0], case[2])
    _kan_check(y.cpu(), y64, a, case[1], case)


def test_kan_linear_scratch_reused_for_a_smaller_call(torch_threads):
    """The same layer on 33 rows, then on 1 row: the scratch of the first call serves the second, whose
    partial slabs are [chunk][1][out] inside it."""
    from fac_fake_amd.ops import KANLinearLayer
    case = (33, 40, 70)
    x, grid, bw, sw, ss = R.kan_inputs(case)
    y64, a = R.kan_ref(x, grid, bw, sw, ss)
    layer = KANLinearLayer(grid, bw, sw, ss, DEV)
    y33 = layer(x.to(DEV))
    scratch = layer._scratch
    y1 = layer(x[5:6].to(DEV))
    torch.cuda.synchronize()
    assert layer._scratch is scratch
    _kan_check(y33.cpu(), y64, a, 40, "33 rows")
    _kan_check(y1.cpu(), y64[5:6], a[5:6], 40, "then 1 row")
    assert torch.equal(y1.cpu(), y33.cpu()[5:6])         # a row's sum does not depend on the batch


# ---------------------------------------------------------------- pooling
def _pool_input(shape, dt, negative, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g)
    if negative:
        x = -1.0 - x.abs()
    return x.to(T16[dt])


AVG_CASES = [
    # (shape [n,d,h,w,c], kernel, stride, padding)
    ((2, 3, 5, 7, 24), (3, 3, 3), 1, 1),
    ((2, 3, 5, 7, 24), (2, 3, 3), (1, 2, 2), (1, 1, 1)),
    ((2, 3, 5, 7, 24), (1, 2, 2), 2, 0),                 # floor mode drops the odd edge
    ((2, 3, 5, 7, 8), (3, 3, 3), 1, 1),                  # a single 8-channel piece
]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("shape,k,s,p", AVG_CASES, ids=[f"c{c[0][4]}-k{_case_id(c[1])}" for c in AVG_CASES])
def test_avg_pool_padded_vs_fp64(shape, k, s, p, dt):
    """Average pooling under padding divides by the whole window (count_include_pad=True): <= 1 ulp of the
    rounded fp64 reference, test_pool_nd's criterion."""
    from fac_fake_amd.ops import pool, pool_route
    x = _pool_input(shape, dt, False, 11)
    ref = R.round16(R.pool_ref(x, k, s, p, "avg"), dt)
    xg = x.to(DEV)
    assert pool_route(xg, k, s, p, "avg") == "pool_nd"
    y = pool(xg, k, s, p, "avg")
    torch.cuda.synchronize()
    assert tuple(y.shape) == tuple(ref.shape)
    u = R.ulps_noise(y.cpu(), ref, dt)
    print(f"avg {shape} {k} {dt}: max {float(u.max()):.3f} ulp")
    assert float(u.max()) <= 1.0


MAX_CASES = [
    # (route, shape, kernel, stride, padding)
    ("pool_max_win", (2, 3, 5, 7, 24), (1, 3, 3), (1, 2, 2), (0, 1, 1)),
    ("pool_max_win", (2, 3, 5, 7, 24), (3, 3, 3), 2, 1),
    ("pool_max_win", (2, 3, 5, 7, 24), (2, 2, 2), 2, 0),
    ("pool_nd", (2, 3, 5, 7, 24), (1, 5, 3), (1, 3, 2), (0, 2, 1)),
    ("pool_max_win", (2, 1, 1, 7, 24), (1, 3, 3), (1, 2, 2), (0, 1, 1)),   # a 1-frame, 1-row map
    ("pool_max_win", (2, 1, 1, 7, 24), (3, 3, 3), 2, 1),
    ("pool_nd", (2, 1, 1, 7, 24), (1, 5, 3), (1, 3, 2), (0, 2, 1)),
]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("route,shape,k,s,p", MAX_CASES,
                         ids=[f"{c[0]}-d{c[1][1]}h{c[1][2]}-k{_case_id(c[2])}" for c in MAX_CASES])
def test_max_pool_negative_inputs_bit_exact(route, shape, k, s, p, dt):
    """Padded max pooling of inputs <= -1: a tap read as 0 (instead of ignored, -inf) would win every
    border window.  Bit-exact."""
    from fac_fake_amd.ops import pool, pool_route
    x = _pool_input(shape, dt, True, 12)
    ref = R.pool_ref(x, k, s, p, "max").to(T16[dt])      # a max selects one of its inputs: exact
    xg = x.to(DEV)
    assert pool_route(xg, k, s, p, "max") == route
    y = pool(xg, k, s, p, "max")
    torch.cuda.synchronize()
    assert tuple(y.shape) == tuple(ref.shape) and bool((y.cpu().float() <= -1).all())
    assert torch.equal(y.cpu().view(torch.int16), ref.view(torch.int16))


SLOT_CASES = [
    ("pool_nd", "avg", (2, 3, 3), (1, 2, 2), (1, 1, 1)),
    ("pool_nd", "max", (1, 5, 3), (1, 3, 2), (0, 2, 1)),
    ("pool_max_win", "max", (3, 3, 3), 2, 1),
]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("route,mode,k,s,p", SLOT_CASES, ids=[f"{c[0]}-{c[1]}" for c in SLOT_CASES])
def test_pool_into_channel_slot(route, mode, k, s, p, dt):
    """c_off 8, ldo = c + 24: the 8 channels before the slot and the 16 after keep their sentinel."""
    from fac_fake_amd.ops import pool, pool_route
    shape = (2, 3, 5, 7, 24)
    x = _pool_input(shape, dt, mode == "max", 13)
    ref = R.round16(R.pool_ref(x, k, s, p, mode), dt)
    xg = x.to(DEV)
    big = torch.full((*ref.shape[:4], 24 + 24), SENT, dtype=T16[dt], device=DEV)
    assert pool_route(xg, k, s, p, mode, out=big, c_off=8) == route
    pool(xg, k, s, p, mode, out=big, c_off=8)
    torch.cuda.synchronize()
    b = big.cpu()
    assert bool((b[..., :8] == SENT).all()) and bool((b[..., 32:] == SENT).all())
    got = b[..., 8:32].contiguous()
    if mode == "max":
        assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    else:
        assert float(R.ulps_noise(got, ref, dt).max()) <= 1.0


# ---------------------------------------------------------------- fac_pack_input
PACK_SRC = {
    # 3 * 11 * 13 = 429 and 2 * 3 * 5 * 7 = 210 positions: one above 256, neither a multiple of 256
    "u8": dict(shape=(3, 11, 13, 3), spatial=(11, 13), div=255.0, mean=R.IMAGENET_MEAN, std=R.IMAGENET_STD),
    "f32": dict(shape=(2, 3, 3, 5, 7), spatial=(3, 5, 7), div=1.0, mean=None, std=None),
}


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("c_pad", [8, 24])
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_pack_input_vs_reference(kind, c_pad, dt):
    """fac_pack_input from uint8 NHWC (/255, ImageNet mean / std) and from fp32 planar raw 0..255 values
    (no mean / std): channels 0..2 bit-equal to (x / div - mean) / std in fp32 rounded once, channels
    3..c_pad-1 exactly zero, nothing written outside [n][s][c_pad]."""
    from fac_fake_amd.ops import pack_input
    cfg = PACK_SRC[kind]
    g = torch.Generator().manual_seed(21)
    src = torch.randint(0, 256, cfg["shape"], generator=g, dtype=torch.uint8)
    src = src if kind == "u8" else src.float()
    n = cfg["shape"][0]
    ref = R.pack_input_ref(src, kind == "u8", cfg["div"], cfg["mean"], cfg["std"], c_pad, dt)
    d, h, w = (1,) * (3 - len(cfg["spatial"])) + cfg["spatial"]
    buf, flat = _guarded(ref.numel(), T16[dt])
    out = pack_input(src.to(DEV), dtype=dt, u8=kind == "u8", div=cfg["div"], mean=cfg["mean"], std=cfg["std"],
                     spatial=cfg["spatial"], c_pad=c_pad, out=flat.view(n, d, h, w, c_pad))
    torch.cuda.synchronize()
    got = out.cpu().view(n, -1, c_pad)
    assert bool((got[..., 3:].view(torch.int16) == 0).all())
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    assert _guards_intact(buf, ref.numel())


def test_pack_input_default_is_eight_channels():
    from fac_fake_amd.ops import pack_input
    src = torch.arange(2 * 5 * 3, dtype=torch.uint8).view(2, 5, 1, 3)
    out = pack_input(src.to(DEV), dtype="fp16", u8=True, spatial=(5, 1))
    torch.cuda.synchronize()
    assert tuple(out.shape) == (2, 1, 5, 1, 8)
    assert torch.equal(out.cpu().view(2, 5, 8), R.pack_input_ref(src, True, 1.0, None, None, 8, "fp16"))


# ---------------------------------------------------------------- fac_pack_input_s2d, fp32 source
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("norm", ["meanstd", "null"])
@pytest.mark.parametrize("pb,pa", [(2, 1), (0, 0), (1, 2)])
@pytest.mark.parametrize("shape", [(2, 3, 10, 12), (2, 3, 3, 10, 12)], ids=["image", "clip"])
def test_pack_input_s2d_f32_vs_reference(shape, pb, pa, norm, dt):
    """fac_pack_input_s2d from an fp32 image batch [n][3][h][w] and a clip batch [n][3][frames][h][w]
    (n = 2 clips of 3 frames: image index = clip * frames + frame) against a reference that slices the
    source by (clip, frame): bit-equal, border cells and channel 3 of every pixel zero."""
    from fac_fake_amd.ops import pack_input_s2d
    g = torch.Generator().manual_seed(31)
    src = torch.randint(0, 256, shape, generator=g).float()
    div, mean, std = (255.0, R.IMAGENET_MEAN, R.IMAGENET_STD) if norm == "meanstd" else (1.0, None, None)
    ref = R.pack_s2d_ref(src, pb, pa, div, mean, std, dt)
    buf, flat = _guarded(ref.numel(), T16[dt])
    out = pack_input_s2d(src.to(DEV), dtype=dt, u8=False, div=div, mean=mean, std=std, pad_before=pb, pad_after=pa,
                         out=flat.view(ref.shape))
    torch.cuda.synchronize()
    got = out.cpu()
    h2, w2 = shape[-2] // 2, shape[-1] // 2
    assert tuple(got.shape) == (2, shape[2] if len(shape) == 5 else 1, h2 + pb + pa, w2 + pb + pa, 16)
    gi = got.view(torch.int16)
    assert bool((gi[..., 3::4] == 0).all())                                        # channel 3 of every pixel
    inner = torch.zeros(got.shape[2], got.shape[3], dtype=torch.bool)
    inner[pb:pb + h2, pb:pb + w2] = True
    assert bool((gi[:, :, ~inner] == 0).all())                                     # the border cells
    assert torch.equal(gi, ref.view(torch.int16))
    assert _guards_intact(buf, ref.numel())


# ---------------------------------------------------------------- sigmoid
@pytest.mark.parametrize("n", [1, 257, 1000])
def test_sigmoid_vs_fp64(n):
    """fac_sigmoid over [-104, 104] (expf overflows past 88.7), 0 and +-inf: |y - ref| <= 4 2^-24 ref + 2^-125,
    no NaN, every value in [0, 1], nothing written past n."""
    x = R.sigmoid_inputs(n)
    ref = R.sigmoid_ref(x)
    xg = x.to(DEV)
    buf, y = _guarded(n, torch.float32)
    _lib.check(_lib.load().fac_sigmoid(xg.data_ptr(), y.data_ptr(), n, torch.cuda.current_stream().cuda_stream),
               None, "fac_sigmoid")
    torch.cuda.synchronize()
    got = y.cpu()
    assert not bool(torch.isnan(got).any()) and bool(((got >= 0) & (got <= 1)).all())
    err, bound = (got.double() - ref).abs(), R.sigmoid_bound(ref)
    print(f"sigmoid n={n}: max err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    assert _guards_intact(buf, n)
    if n >= 3:
        assert got[0] == 0.5 and got[1] == 1.0 and got[2] == 0.0
    from fac_fake_amd.ops import sigmoid
    assert torch.equal(sigmoid(xg).cpu(), got)
