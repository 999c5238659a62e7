"""The eight CViT variants on the GPU: fac_ggca_apply (ggca.hip) against the
CPU reference's GGCA arithmetic (tests/variants_ref.py), and the drop-ins of
fac_fake_amd/variants.py against the reference classes' recorded outputs
(tests/golden/variants_*, tools/make_golden_variants.py).

Models are built and released one at a time.
"""
import contextlib
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import variants_ref as R  # noqa: E402
from fac_fake_amd import _lib  # noqa: E402
from fac_fake_amd.weights import VARIANT_NAMES, make_crops, make_variant_state_dict  # noqa: E402
from oracle.cvit_torch import normalize_u8  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
# |got - ref| / max(|ref|, 1e-3): twice the half-ulp of the one output rounding (fac_ggca's rule, test_repbn8.py)
KERNEL_BOUND = {"fp16": 2 ** -10 + 1e-5, "bf16": 2 ** -7 + 1e-5}
# (h, w, c, groups): RepBn3's map (cr = 1); non-square; just past the LDS route (cr = 2); the LDS route
SHAPES = [(56, 56, 64, 4), (20, 24, 64, 4), (17, 17, 128, 4), (7, 7, 512, 4)]
ROUTES = [2, 2, 2, 1]
REPBN3 = "cvit_GGCA_ADD_DEConv_RepBn3"
N = 3


@functools.lru_cache(maxsize=None)
def _ggca_weights(c, groups):
    """Random GGCA(c, ., ., 16, groups).shared_conv weights, the reference module's shapes."""
    g = torch.Generator().manual_seed(1000 + c)
    cg = c // groups
    cr = cg // 16
    u = lambda *s, lo=-1.0, hi=1.0: torch.rand(*s, generator=g) * (hi - lo) + lo  # noqa: E731
    w1 = u(cr, cg, 1, 1) * (3.0 / cg) ** 0.5
    bn = (u(cr, lo=-0.2, hi=0.2), u(cr, lo=0.5, hi=1.5), u(cr, lo=0.8, hi=1.2), u(cr, lo=-0.2, hi=0.2))
    return w1, u(cr, lo=-0.1, hi=0.1), bn, u(cg, cr, 1, 1), u(cg, lo=-0.1, hi=0.1)


@functools.lru_cache(maxsize=None)
def _input(shape, signed, dt):
    h, w, c, _ = shape
    g = torch.Generator().manual_seed(7 + h * w + c + int(signed))
    x = torch.randn(N, h, w, c, generator=g) * 1.5 if signed else torch.rand(N, h, w, c, generator=g) * 3
    return x.to(T16[dt])


@functools.lru_cache(maxsize=None)
def _reference(shape, signed, dt, op):
    """The reference GGCA arithmetic in fp32 on the 16-bit input values, NHWC."""
    x = _input(shape, signed, dt).float().permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        return R.ggca_combine(_ggca_weights(shape[2], shape[3]), x, op, shape[3]).permute(0, 2, 3, 1).contiguous()


def _dev_weights(c, groups):
    w1, b1, bn, w2, b2 = _ggca_weights(c, groups)
    cr, cg = w1.shape[:2]
    return [t.to(DEV, torch.float32).contiguous() for t in (w1.reshape(cr, cg), b1, torch.stack(bn),
                                                            w2.reshape(cg, cr), b2)]


def _apply(x16, groups, op, dt, entry="fac_ggca_apply", shape=None, weights=None):
    """fac_ggca_apply (or fac_ggca) on a device tensor [n,h,w,c]; returns (status, out)."""
    n, h, w, c = shape or x16.shape
    wts = weights or _dev_weights(c, groups)
    out = torch.empty_like(x16)
    ptrs = [t.data_ptr() for t in wts]
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    if entry == "fac_ggca":
        rc = lib.fac_ggca(_lib.DTYPES[dt], x16.data_ptr(), n, h, w, c, groups, *ptrs, out.data_ptr(), st)
    else:
        rc = lib.fac_ggca_apply(_lib.DTYPES[dt], x16.data_ptr(), n, h, w, c, groups, *ptrs, op, out.data_ptr(), st)
    torch.cuda.synchronize()
    return rc, out


def test_routes_depend_on_the_shape_alone():
    lib = _lib.load()
    assert [lib.fac_ggca_apply_route(h, w, c, g) for h, w, c, g in SHAPES] == ROUTES
    assert lib.fac_ggca_apply_route(64, 64, 64, 4) == 2 and lib.fac_ggca_apply_route(65, 56, 64, 4) == 0


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("op", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ggca_apply_vs_reference(torch_threads, shape, op, dt):
    """x * GGCA(x) / x + GGCA(x) within one 16-bit rounding of the fp32
    reference, on non-negative and on signed inputs (the max and mean pools
    treat signs differently)."""
    for signed in (False, True):
        x = _input(shape, signed, dt)
        rc, got = _apply(x.to(DEV), shape[3], op, dt)
        assert rc == 0
        ref = _reference(shape, signed, dt, op)
        err = float(((got.float().cpu() - ref).abs() / ref.abs().clamp_min(1e-3)).max())
        print(f"{shape} op {op} {dt} signed {signed}: max rel err {err:.3e} (bound {KERNEL_BOUND[dt]:.3e})")
        assert err <= KERNEL_BOUND[dt], (shape, op, dt, signed, err)


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_lds_route_op0_is_fac_ggca_bit_for_bit(dt):
    shape = (7, 7, 512, 4)
    for signed in (False, True):
        x = _input(shape, signed, dt).to(DEV)
        rc0, want = _apply(x, 4, 0, dt, entry="fac_ggca")
        rc1, got = _apply(x, 4, 0, dt)
        assert rc0 == 0 and rc1 == 0
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("op", [0, 1])
@pytest.mark.parametrize("shape", [(56, 56, 64, 4), (7, 7, 512, 4)], ids=["streaming", "lds"])
def test_a_crop_does_not_depend_on_its_batch(shape, op):
    x = _input(shape, True, "fp16").to(DEV)
    rc3, three = _apply(x, shape[3], op, "fp16")
    rc1, one = _apply(x[1:2].contiguous(), shape[3], op, "fp16")
    assert rc3 == 0 and rc1 == 0
    assert torch.equal(three[1:2].view(torch.int16), one.view(torch.int16))


def test_error_returns():
    x = _input((56, 56, 64, 4), False, "fp16").to(DEV)
    wts = _dev_weights(64, 4)
    assert _apply(x, 4, 1, "fp16", shape=(1, 65, 56, 64), weights=wts)[0] == -2      # FAC_ERR_SHAPE: h = 65
    assert _apply(x, 4, 1, "fp16", shape=(1, 56, 65, 64), weights=wts)[0] == -2
    assert _apply(x, 3, 1, "fp16", shape=(1, 56, 56, 64), weights=wts)[0] == -1      # FAC_ERR_ARG: c % groups
    assert _apply(x, 4, 2, "fp16", shape=(1, 56, 56, 64), weights=wts)[0] == -1      # op
    assert _apply(x, 4, 1, "fp16", shape=(1, 56, 56, 96), weights=wts)[0] == -2      # cg = 24, no multiple of 16
    lib = _lib.load()
    assert lib.fac_ggca_apply(1, None, 1, 56, 56, 64, 4, *[t.data_ptr() for t in wts], 1, x.data_ptr(), None) == -1


# ---------------------------------------------------------------- the drop-ins
def _sd_t(name):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in make_variant_state_dict(name, 0).items()}


@contextlib.contextmanager
def _model(name, dt):
    """One variant on the GPU, released on exit."""
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from fac_fake_amd import variants
    m = variants.CViT(name, dtype=dt)
    m.load_state_dict(_sd_t(name))
    m.to(DEV)
    try:
        yield m
    finally:
        torch.cuda.synchronize()
        m._release()


E2E = [(n, "fp16") for n in VARIANT_NAMES] + [("cvit_GGCA_ADD", "bf16"), (REPBN3, "bf16")]


@pytest.mark.parametrize("name,dt", E2E)
def test_variant_matches_reference(golden, name, dt):
    """forward_u8 on the 4 golden crops against the reference class's fp32
    probabilities, within 2x the recorded 16-bit emulation envelope of that
    variant and dtype (test_variants.py holds the emulation to 1x)."""
    g = golden("variants_golden.npz")
    tol = 2 * golden("variants_envelope.json")[name][dt]
    crops = torch.from_numpy(make_crops(4, seed=int(g["crop_seed"]))).to(DEV)
    with _model(name, dt) as m, torch.no_grad():
        lg, pr = m.forward_u8(crops, return_probs=True)
        torch.cuda.synchronize()
        lg, pr = lg.cpu().numpy(), pr.cpu().numpy()
    p_ref = 1 / (1 + np.exp(-g[f"{name}.logits"]))
    d = float(np.abs(pr - p_ref).max())
    print(f"{name} {dt}: max|dp| vs reference {d:.3e} (tolerance {tol:.3e})")
    assert np.isfinite(lg).all()
    assert d <= tol, (name, dt, d, tol)
    assert np.allclose(pr, 1 / (1 + np.exp(-lg)), atol=1e-6)


def test_repbn3_56x56_map_matches_emulation(torch_threads):
    """features1 and x + GGCA(x) on the 64x56x56 map against the emulation of
    the same rounding points (the stem bound of test_repbn8.py)."""
    crops = make_crops(2, seed=34)
    with _model(REPBN3, "fp16") as m, torch.no_grad():
        m.forward_u8(torch.from_numpy(crops).to(DEV))   # prepares the packed layers
        f = m.stem_features(torch.from_numpy(crops).to(DEV), u8=True, upto="ggca").float().cpu()
    assert tuple(f.shape) == (2, 56, 56, 64)
    _, _, ref = R.forward_emulated(REPBN3, make_variant_state_dict(REPBN3, 0), normalize_u8(crops), dtype="fp16",
                                   return_features=True)
    ref = ref.permute(0, 2, 3, 1)
    rel = float((f - ref).norm() / ref.norm())
    print(f"RepBn3 56x56 map after x + GGCA(x): relative L2 {rel:.3e}")
    assert rel <= 5e-3, rel


def test_repbn3_u8_and_nchw_paths_agree():
    crops = make_crops(3, seed=33)
    with _model(REPBN3, "fp16") as m, torch.no_grad():
        a = m.forward_u8(torch.from_numpy(crops).to(DEV))
        b = m(normalize_u8(crops).to(DEV))
        torch.cuda.synchronize()
        assert torch.equal(a, b)
        with pytest.raises(RuntimeError):      # the reference's pos_embedding[0:B] past 32 crops
            m.forward_u8(torch.zeros(33, 224, 224, 3, dtype=torch.uint8, device=DEV))


def test_repbn3_graph_replay_matches_eager():
    crops = torch.from_numpy(make_crops(8, seed=35)).to(DEV)
    slots = torch.arange(8, dtype=torch.int32, device=DEV) * 3 % 32
    with _model(REPBN3, "bf16") as m, torch.no_grad():
        eager = m.forward_u8(crops, pos_index=slots)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            m.forward_u8(crops, pos_index=slots)    # sizes this stream's GGCA workspace before the capture
            with torch.cuda.graph(g, stream=s):
                out = m.forward_u8(crops, pos_index=slots)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
        del g


def test_predict_video_takes_a_variant():
    """video.predict_video on a 30-frame synthetic video (3 crops): the logits
    of the model on those crops, and prediction.predict_crops' score up to the
    device sigmoid's last bit (test_gpu_parity.py's rule for the same pair)."""
    from fac_fake_amd.prediction import chunk_slots, predict_crops
    from fac_fake_amd.video import crop_faces, predict_video, reference_boxes, synthetic_video
    frames, boxes = synthetic_video(30, 360, 640, seed=3, device=DEV)
    with _model("cvit_GGCA_ADD_RepBn", "fp16") as m:
        score, logits = predict_video(m, frames, boxes, return_logits=True)
        sel = reference_boxes(boxes, 30)
        crops = crop_faces(frames, sel)
        with torch.no_grad():
            want = m.forward_u8(crops, pos_index=torch.from_numpy(chunk_slots(len(sel))))
        assert len(sel) == 3 and torch.equal(logits, want)
        assert abs(score - predict_crops(m, crops)) <= 1e-6
