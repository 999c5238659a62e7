"""What fac_ggca, fac_kan_linear, fac_pack_input, fac_pack_input_s2d and
fac_sigmoid refuse before they launch anything, pinned without a GPU (as
test_conv_routes.py pins the dispatchers): every row is rejected by the entry
point's own argument checks, so no device is touched.  The pointers are
dummies; the entry points only test them for NULL on these paths.
"""
import pytest

from fac_fake_amd import _lib

ARG, SHAPE = -1, -2
PTR = 64            # a dummy non-NULL pointer
BF16, F16 = 0, 1


@pytest.fixture(scope="module")
def lib(built_lib):
    return _lib.load()


def ggca(lib, *, dtype=F16, x=PTR, n=2, h=7, w=7, c=512, groups=4, w1=PTR, out=PTR):
    return lib.fac_ggca(dtype, x, n, h, w, c, groups, w1, PTR, PTR, PTR, PTR, out, None)


GGCA_ROWS = [
    ("null x", dict(x=None), ARG),
    ("null w1", dict(w1=None), ARG),
    ("null out", dict(out=None), ARG),
    ("c % groups != 0", dict(c=510, groups=4), ARG),
    ("h = 17", dict(h=17, w=1, c=16, groups=1), SHAPE),
    ("w = 17", dict(h=1, w=17, c=16, groups=1), SHAPE),
    ("cg = 24", dict(c=48, groups=2), SHAPE),
    ("cg = 272", dict(h=1, w=1, c=272, groups=1), SHAPE),
    ("16 x 16 x cg 80: 20480 features", dict(h=16, w=16, c=80, groups=1), SHAPE),
    ("1 x 16 x cg 256: 8704 pooled values", dict(h=1, w=16, c=256, groups=1), SHAPE),
    ("dtype 2", dict(dtype=2), ARG),
    ("dtype -1", dict(dtype=-1), ARG),
    ("c = 0", dict(c=0), ARG),
    ("n = 0", dict(n=0), ARG),
    ("groups = 0", dict(groups=0), ARG),
]


@pytest.mark.parametrize("what,kw,status", GGCA_ROWS, ids=[r[0] for r in GGCA_ROWS])
def test_ggca_rejects(lib, what, kw, status):
    assert ggca(lib, **kw) == status


def kan(lib, *, x=PTR, rows=4, in_f=64, out_f=8, grid=PTR, n_knots=12, wcat=PTR, y=PTR, partial=PTR):
    return lib.fac_kan_linear(x, rows, in_f, out_f, grid, n_knots, wcat, y, partial, None)


KAN_ROWS = [
    ("null x", dict(x=None), ARG),
    ("null grid", dict(grid=None), ARG),
    ("null scratch", dict(partial=None), ARG),
    ("rows = 0", dict(rows=0), ARG),
    ("n_knots 11", dict(n_knots=11), SHAPE),
    ("rows * out_f = 2^31", dict(rows=1 << 16, in_f=1, out_f=1 << 15), SHAPE),
    ("rows * out_f > 2^32 (wraps to a small int)", dict(rows=(1 << 16) + 1, in_f=1, out_f=1 << 16), SHAPE),
    ("chunks * rows * out_f = 2^31", dict(rows=1 << 13, in_f=33 + 32 * 6, out_f=1 << 15), SHAPE),
]


@pytest.mark.parametrize("what,kw,status", KAN_ROWS, ids=[r[0] for r in KAN_ROWS])
def test_kan_linear_rejects(lib, what, kw, status):
    assert kan(lib, **kw) == status


def test_kan_scratch_bytes(lib):
    assert lib.fac_kan_scratch_bytes(0, 64, 8) == 0
    assert lib.fac_kan_scratch_bytes(4, 0, 8) == 0 and lib.fac_kan_scratch_bytes(4, 64, -1) == 0
    assert lib.fac_kan_scratch_bytes(33, 40, 70) == 2 * 33 * 70 * 4      # ceil(40 / 32) slabs
    assert lib.fac_kan_scratch_bytes(1, 1, 1) == 4
    assert lib.fac_kan_scratch_bytes(1 << 16, 64, 1 << 15) == 2 * (1 << 31) * 4   # size_t arithmetic


def pack(lib, *, dtype=F16, src=PTR, kind=0, n=2, s=100, div=255.0, out=PTR, c_pad=8):
    return lib.fac_pack_input(dtype, src, kind, n, s, div, None, None, out, c_pad, None)


PACK_ROWS = [
    ("null src", dict(src=None), ARG),
    ("c_pad 4", dict(c_pad=4), ARG),
    ("c_pad 12", dict(c_pad=12), ARG),
    ("src_kind 2", dict(kind=2), ARG),
    ("div 0", dict(div=0.0), ARG),
    ("div nan", dict(div=float("nan")), ARG),
    ("dtype 2", dict(dtype=2), ARG),
    ("s = 0", dict(s=0), ARG),
]


@pytest.mark.parametrize("what,kw,status", PACK_ROWS, ids=[r[0] for r in PACK_ROWS])
def test_pack_input_rejects(lib, what, kw, status):
    assert pack(lib, **kw) == status


def s2d(lib, *, dtype=BF16, src=PTR, kind=1, n=2, frames=1, h=10, w=12, pb=2, pa=1, div=1.0, out=PTR):
    return lib.fac_pack_input_s2d(dtype, src, kind, n, frames, h, w, pb, pa, div, None, None, out, None)


S2D_ROWS = [
    ("null out", dict(out=None), ARG),
    ("odd h", dict(h=11), ARG),
    ("odd w", dict(w=13), ARG),
    ("negative pad_before", dict(pb=-1), ARG),
    ("negative pad_after", dict(pa=-1), ARG),
    ("frames = 0", dict(frames=0), ARG),
    ("dtype 2", dict(dtype=2), ARG),
    ("2^31 cells", dict(n=1 << 15, frames=4, h=250, w=250, pb=2, pa=1), SHAPE),          # 2^17 * 128^2
    ("2^31 - 256 cells", dict(n=(1 << 23) - 1, frames=1, h=28, w=28, pb=1, pa=1), SHAPE),  # (2^23 - 1) * 256
]


@pytest.mark.parametrize("what,kw,status", S2D_ROWS, ids=[r[0] for r in S2D_ROWS])
def test_pack_input_s2d_rejects(lib, what, kw, status):
    assert s2d(lib, **kw) == status


def test_sigmoid_rejects(lib):
    assert lib.fac_sigmoid(PTR, PTR, 0, None) == ARG
    assert lib.fac_sigmoid(PTR, PTR, -5, None) == ARG
    assert lib.fac_sigmoid(None, PTR, 8, None) == ARG and lib.fac_sigmoid(PTR, None, 8, None) == ARG
