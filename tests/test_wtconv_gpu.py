"""cvit_GGCA_ADD_WTConv on the GPU: fac_wtconv (wtconv.hip) against a float64
reference of its own arithmetic (tests/wtconv_ref.py) and against exactly
countable cases, and the drop-in of fac_fake_amd/wtconv.py against the
reference class's recorded outputs (tests/golden/wtconv_*,
tools/make_golden_wtconv.py).
"""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))

import wtconv_ref as R  # noqa: E402
from fac_fake_amd import _lib  # noqa: E402
from fac_fake_amd.weights import db1_filters, make_crops, make_wtconv_state_dict  # noqa: E402
from oracle.cvit_torch import normalize_u8  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
# |got - ref| / max(|ref|, 1e-3): twice the half-ulp of the one output rounding (KERNEL_BOUND of test_variants_gpu.py)
KERNEL_BOUND = {"fp16": 2 ** -10 + 1e-5, "bf16": 2 ** -7 + 1e-5}
CHAIN = 64                       # the longest fp32 chain of an output: 4 + 25 + 4 + 25 + the affine
OK, ARG, SHAPE = 0, -1, -2
# (n, h, w, c).  A workgroup owns 16 x 16 outputs (8 x 8 half-resolution pixels) of 16 channels.  (2, 2): one
# half-resolution pixel, every tap but the centre is padding; (6, 10): narrower than the 4-pixel halo in one direction;
# (18, 22) and (38, 50): no multiple of the tile, so the last tile of a row and of a column is partly empty and
# crops start inside the grid; then one crop of each of the model's four sites.
SHAPES = [(3, 2, 2, 32), (3, 6, 10, 32), (2, 18, 22, 64), (1, 38, 50, 128), (1, 28, 28, 256), (1, 224, 224, 32),
          (1, 112, 112, 64), (1, 56, 56, 128)]
_ids = lambda s: "x".join(map(str, s))  # noqa: E731


@functools.lru_cache(maxsize=None)
def _operands(c):
    """Random operands of one layer in wt_fold's natural order, fp32: NON-Haar 2x2 filters (normal, 0.5), taps in
    +-0.3, scale in +-[0.5, 1] with both signs, shift in +-1."""
    g = torch.Generator().manual_seed(700 + c)
    u = lambda *s, lo=-1.0, hi=1.0: torch.rand(*s, generator=g) * (hi - lo) + lo  # noqa: E731
    sign = torch.where(torch.rand(c, generator=g) < 0.3, -1.0, 1.0)
    return dict(dwt=torch.randn(c, 4, 2, 2, generator=g) * 0.5, wtaps=u(c, 4, 25, lo=-0.3, hi=0.3),
                iwt=torch.randn(c, 4, 2, 2, generator=g) * 0.5, btaps=u(c, 25, lo=-0.3, hi=0.3),
                scale=u(c, lo=0.5, hi=1.0) * sign, shift=u(c))


def _haar(c):
    """The db1 filters with exactly +-0.5 entries, [c, 4, 2, 2] each."""
    d, i = db1_filters(c)
    return (torch.from_numpy(np.sign(d)).reshape(c, 4, 2, 2) * 0.5, torch.from_numpy(np.sign(i)).reshape(c, 4, 2, 2) * 0.5)


@functools.lru_cache(maxsize=None)
def _input(shape, dt):
    n, h, w, c = shape
    g = torch.Generator().manual_seed(13 + h * w + c)
    return (torch.randn(n, h, w, c, generator=g) * 1.5).to(T16[dt])     # signed


@functools.lru_cache(maxsize=None)
def _reference(shape, dt):
    """(ref, mag) of the unpooled layer in float64 from the 16-bit input values and the same fp32 operands, NCHW:
    mag is the same layer on |x| with every filter, tap and scale in absolute value and shift 0.  The pooled
    pair is the 2x2 max of each (the bound of a max of four is at most the largest of the four bounds)."""
    x = _input(shape, dt).double().permute(0, 3, 1, 2)
    ops = _operands(shape[3])
    with torch.no_grad():
        ref = R.wt_layer(x, ops, False, torch.float64)
        mag = R.wt_layer(x.abs(), {k: (torch.zeros_like(v) if k == "shift" else v.abs()) for k, v in ops.items()}, False,
                         torch.float64)
    return ref, mag


def _run(x16, ops, pool, dt, shape=None, out=None):
    """fac_wtconv on a device tensor [n,h,w,c] with operands in wt_fold's natural order; returns (status, out)."""
    from fac_fake_amd.wtconv import wt_pack
    n, h, w, c = shape or x16.shape
    dev_ops = wt_pack(ops, DEV)
    if out is None:
        out = torch.empty(n, h // 2 if pool else h, w // 2 if pool else w, c, dtype=x16.dtype, device=DEV)
    rc = _lib.load().fac_wtconv(_lib.DTYPES[dt], x16.data_ptr(), out.data_ptr(), n, h, w, c,
                                *[t.data_ptr() for t in dev_ops], int(pool), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("pool", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_wtconv_vs_float64_reference(shape, pool, dt):
    """|got - ref| <= KERNEL_BOUND[dt] max(|ref|, 1e-3) + 64 * 2^-24 mag on signed inputs, non-Haar 2x2 filters
    and an affine of both signs: the half-ulp of the one rounding (doubled, the project's bound) plus the derived
    fp32 summation error of the ~425 signed products behind an output, whose longest chain is 64 long.  Unlike
    fac_idwconv's, the plain bound alone is not expected to hold near zeros of the output.
    Measured on an MI355X, the share of the allowance used: 0.42 - 0.49 for fp16 and 0.42 - 0.50 for bf16 over all
    32 cases, i.e. the half-ulp of the one rounding.  Against the plain one-rounding bound alone the same runs use
    0.43 - 0.50 (bf16) and up to 0.70 (fp16, the full-size sites): the summation term shows in fp16 and was not
    needed on these inputs."""
    x = _input(shape, dt)
    rc, got = _run(x.to(DEV), _operands(shape[3]), pool, dt)
    assert rc == OK
    ref, mag = _reference(shape, dt)
    if pool:
        ref, mag = F.max_pool2d(ref, 2, 2), F.max_pool2d(mag, 2, 2)
    ref, mag = ref.permute(0, 2, 3, 1), mag.permute(0, 2, 3, 1)
    assert got.shape == ref.shape
    diff = (got.double().cpu() - ref).abs()
    allow = KERNEL_BOUND[dt] * ref.abs().clamp_min(1e-3) + CHAIN * 2.0 ** -24 * mag
    share = float((diff / allow).max())
    plain = float((diff / (KERNEL_BOUND[dt] * ref.abs().clamp_min(1e-3))).max())
    print(f"{shape} pool {pool} {dt}: {share:.3f} of the allowance used ({plain:.3f} of the plain one-rounding bound); "
          f"max|ref| {float(ref.abs().max()):.3g}, share of zeros {float((ref == 0).double().mean()):.2f}")
    assert float(ref.abs().max()) > 1.0 and float((ref == 0).double().mean()) < 0.95
    assert share <= 1.0, (shape, pool, dt, share)


def _counts(h, w):
    """In-map taps of a 5x5 window centred on each pixel of an h x w map."""
    ys, xs = torch.arange(h).view(h, 1), torch.arange(w).view(1, w)
    rows = torch.clamp(ys + 2, max=h - 1) - torch.clamp(ys - 2, min=0) + 1
    cols = torch.clamp(xs + 2, max=w - 1) - torch.clamp(xs - 2, min=0) + 1
    return (rows * cols).float()


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("pool", [0, 1])
@pytest.mark.parametrize("shape", [(3, 2, 2, 32), (3, 6, 10, 32), (2, 18, 22, 64), (2, 38, 34, 128)], ids=_ids)
def test_exact_counting(shape, pool, dt):
    """All-ones input, the exact +-0.5 filters, all taps 1, scale 0.5, shift 3: the low-pass subband is 2 inside
    the map, the others 0, so the output is 0.5 (n5(y, x) + n5h(y // 2, x // 2)) + 3 with n5 / n5h the in-map
    taps of a 5x5 window at full / half resolution.  Every value is exact in both dtypes.  A padded tap taken as
    `shift`, a subband pixel outside the map that is not 0, or a halo read across a crop or tile boundary changes
    a count."""
    n, h, w, c = shape
    dwt, iwt = _haar(c)
    ops = dict(dwt=dwt, wtaps=torch.ones(c, 4, 25), iwt=iwt, btaps=torch.ones(c, 25), scale=torch.full((c,), 0.5),
               shift=torch.full((c,), 3.0))
    rc, got = _run(torch.ones(n, h, w, c, dtype=T16[dt], device=DEV), ops, pool, dt)
    assert rc == OK
    n5h = _counts(h // 2, w // 2).repeat_interleave(2, 0).repeat_interleave(2, 1)
    want = 0.5 * (_counts(h, w) + n5h) + 3.0
    assert float(want[0, 0]) == 0.5 * (min(3, h) * min(3, w) + min(3, h // 2) * min(3, w // 2)) + 3.0
    if pool:
        want = F.max_pool2d(want.view(1, 1, h, w), 2, 2).view(h // 2, w // 2)
    want = want.view(1, *want.shape, 1).expand(n, -1, -1, c)
    assert torch.equal(want.to(T16[dt]).float(), want)                    # every value is exact in the dtype
    assert torch.equal(got.float().cpu(), want)


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("pool", [0, 1])
@pytest.mark.parametrize("shape", [(3, 2, 2, 32), (2, 18, 22, 64), (1, 28, 28, 256)], ids=_ids)
def test_perfect_reconstruction(shape, pool, dt):
    """The exact +-0.5 filters, wavelet taps that are the centre tap only, base taps 0, scale 1, shift 0, inputs
    that are multiples of 1/8 in +-16 (exact in both dtypes, every fp32 sum exact): the synthesis inverts the
    analysis and the output is relu(x) bit for bit."""
    n, h, w, c = shape
    dwt, iwt = _haar(c)
    wtaps = torch.zeros(c, 4, 25)
    wtaps[:, :, 12] = 1.0
    ops = dict(dwt=dwt, wtaps=wtaps, iwt=iwt, btaps=torch.zeros(c, 25), scale=torch.ones(c), shift=torch.zeros(c))
    g = torch.Generator().manual_seed(h * w + c)
    x = (torch.randint(-128, 129, (n, h, w, c), generator=g).float() / 8).to(T16[dt])
    assert torch.equal(x.float() * 8, (x.float() * 8).round()) and float(x.min()) < -15 and float(x.max()) > 15
    rc, got = _run(x.to(DEV), ops, pool, dt)
    assert rc == OK
    want = torch.relu(x.float())
    if pool:
        want = F.max_pool2d(want.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    want = want.to(T16[dt]).contiguous()
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("pool", [0, 1])
@pytest.mark.parametrize("shape", [(3, 6, 10, 32), (3, 18, 22, 64), (3, 38, 50, 128)], ids=_ids)
def test_a_crop_does_not_depend_on_its_batch(shape, pool):
    x = _input(shape, "fp16").to(DEV)
    ops = _operands(shape[3])
    rc3, three = _run(x, ops, pool, "fp16")
    rc1, one = _run(x[1:2].contiguous(), ops, pool, "fp16")
    assert rc3 == OK and rc1 == OK
    assert torch.equal(three[1:2].view(torch.int16), one.view(torch.int16))
    assert not torch.equal(three[0].view(torch.int16), three[1].view(torch.int16))


def test_error_returns():
    from fac_fake_amd.wtconv import wt_pack
    x = _input((1, 12, 12, 288), "fp16").to(DEV)
    out = torch.empty_like(x)
    ops = _operands(64)
    run = lambda shape, pool=0, dt="fp16": _run(x, ops, pool, dt, shape=shape, out=out)[0]  # noqa: E731
    assert run((1, 12, 12, 48)) == SHAPE            # c no multiple of 32
    assert run((1, 12, 12, 16)) == SHAPE            # c < 32
    assert run((1, 12, 12, 288)) == SHAPE           # c > 256
    assert run((1, 11, 12, 64)) == SHAPE            # odd h, with and without the pool
    assert run((1, 11, 12, 64), 1) == SHAPE
    assert run((1, 12, 11, 64)) == SHAPE            # odd w
    assert run((1, 0, 12, 64)) == SHAPE             # h < 2
    assert run((1, 12, 226, 64)) == SHAPE           # w > 224
    assert run((0, 12, 12, 64)) == ARG              # n <= 0
    assert run((-1, 12, 12, 64)) == ARG
    assert run((1, 12, 12, 64), 2) == ARG           # a pool flag other than 0 / 1
    lib = _lib.load()
    d = wt_pack(ops, DEV)
    ptrs = [t.data_ptr() for t in d]
    call = lambda dt, i, o, p, pool=0: lib.fac_wtconv(dt, i, o, 1, 12, 12, 64, *p, pool, None)  # noqa: E731
    assert call(2, x.data_ptr(), out.data_ptr(), ptrs) == ARG                  # bad dtype
    assert call(1, None, out.data_ptr(), ptrs) == ARG                          # null input
    assert call(1, x.data_ptr(), None, ptrs) == ARG                            # null output
    for k in range(6):                                                         # each operand null, then misaligned
        assert call(1, x.data_ptr(), out.data_ptr(), ptrs[:k] + [None] + ptrs[k + 1:]) == ARG
        assert call(1, x.data_ptr(), out.data_ptr(), ptrs[:k] + [ptrs[k] + 2] + ptrs[k + 1:]) == ARG
    assert call(1, x.data_ptr() + 8, out.data_ptr(), ptrs) == ARG              # maps not 16-byte aligned
    assert call(1, x.data_ptr(), out.data_ptr() + 2, ptrs) == ARG
    torch.cuda.synchronize()
    # and a valid call afterwards: the same bits as a fresh run of that shape
    xin = _input((1, 12, 12, 64), "fp16").to(DEV)
    rc, a = _run(xin, ops, 0, "fp16")
    ref = R.wt_layer(xin.cpu().double().permute(0, 3, 1, 2), ops, False, torch.float64).permute(0, 2, 3, 1)
    assert rc == OK and float((a.double().cpu() - ref).abs().max()) <= 2 ** -9 * float(ref.abs().max())


# ---------------------------------------------------------------- the drop-in
def _sd_t():
    return {k: torch.from_numpy(np.asarray(v)) for k, v in make_wtconv_state_dict(R.NAME, 0).items()}


@pytest.fixture(scope="module")
def models():
    """The drop-in per dtype, built on first use, released when the module is done."""
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from fac_fake_amd import wtconv
    built = {}

    def get(dt):
        if dt not in built:
            m = wtconv.CViT(dtype=dt)
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
    """forward_u8 on the 8 golden crops against the reference class's fp32 probabilities, within 2x the recorded
    16-bit emulation envelope of that dtype (test_wtconv.py holds the emulation to 1.25x)."""
    g = golden("wtconv_golden.npz")
    tol = 2 * golden("wtconv_envelope.json")[dt]
    crops = torch.from_numpy(make_crops(8, seed=int(g["crop_seed"]))).to(DEV)
    with torch.no_grad():
        lg, pr = models(dt).forward_u8(crops, return_probs=True)
        torch.cuda.synchronize()
    lg, pr = lg.cpu().numpy(), pr.cpu().numpy()
    d = float(np.abs(pr - g["probs"]).max())
    print(f"cvit_GGCA_ADD_WTConv {dt}: max|dp| vs reference {d:.3e} (tolerance {tol:.3e})")
    assert np.isfinite(lg).all()
    assert d <= tol, (dt, d, tol)
    assert np.allclose(pr, 1 / (1 + np.exp(-lg)), atol=1e-6)


def test_map_after_the_first_pool_matches_emulation(models, torch_threads):
    """conv 3->32 and two WT layers with the pool, [B,112,112,32], against the emulation of the same rounding
    points by relative L2 <= 5e-3, the project's bound for this comparison
    (test_repbn3_56x56_map_matches_emulation).  The two differ only where fp32 summation order flips a 16-bit
    rounding."""
    crops = make_crops(2, seed=34)
    m = models("fp16")
    with torch.no_grad():
        m.forward_u8(torch.from_numpy(crops).to(DEV))   # prepares the packed layers
        f = m.stem_features(torch.from_numpy(crops).to(DEV), u8=True, upto=3).float().cpu()
    assert tuple(f.shape) == (2, 112, 112, 32)
    _, maps = R.forward_emulated(make_wtconv_state_dict(R.NAME, 0), normalize_u8(crops), dtype="fp16", return_features=True)
    ref = maps["features.6"].permute(0, 2, 3, 1)
    rel = float((f - ref).norm() / ref.norm())
    print(f"WTConv 112x112 map after the first pool: relative L2 {rel:.3e}")
    assert rel <= 5e-3, rel


def test_u8_and_nchw_paths_agree(models):
    crops = make_crops(3, seed=33)
    m = models("fp16")
    with torch.no_grad():
        a = m.forward_u8(torch.from_numpy(crops).to(DEV))
        b = m(normalize_u8(crops).to(DEV))
        torch.cuda.synchronize()
        assert torch.equal(a, b)
        with pytest.raises(RuntimeError):      # the reference's pos_embedding[0:B] past 32 crops
            m.forward_u8(torch.zeros(33, 224, 224, 3, dtype=torch.uint8, device=DEV))


def test_graph_replay_matches_eager(models):
    crops = torch.from_numpy(make_crops(8, seed=35)).to(DEV)
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


def test_predict_video_takes_the_model(models):
    """video.predict_video on a 30-frame synthetic video (3 crops): the logits of the model on those crops, and
    prediction.predict_crops' score up to the device sigmoid's last bit."""
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
