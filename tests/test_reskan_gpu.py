"""ResKan on the GPU: the BasicBlock kernels (csrc/resnet.hip) against fp64,
and the model against outputs of the reference module (tests/golden/reskan_*,
tools/make_golden_reskan.py)."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))

from fac_fake_amd.weights import make_crops, make_reskan_state_dict, reskan_crops_varied  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
MANT = {"fp16": 10, "bf16": 7}
MIN_EXP = {"fp16": -14, "bf16": -126}           # smallest normal exponent: below it the spacing is constant
SHAPES = [(56, 64), (28, 128), (14, 256), (7, 512)]


def _ulp(ref: torch.Tensor, dt: str) -> torch.Tensor:
    """One 16-bit unit in the last place of |ref| (float64)."""
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** MIN_EXP[dt]))).clamp_min(MIN_EXP[dt])
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - MANT[dt])


@functools.lru_cache(maxsize=None)
def _case(h, c, dt, n, variant="random"):
    """Operands already rounded to the dtype (bias fp32), the float64 reference
    relu(conv(x, w) + bias + residual) and its tolerance: one 16-bit ulp of
    |ref| plus the worst-case fp32 accumulation bound K 2^-24 A, K = 9 cin,
    A = conv(|x|, |w|) + |bias| + |residual|.  Computed once per case."""
    g = torch.Generator().manual_seed(h * 1000 + c + 17 * n + (dt == "bf16"))
    x = torch.randn(n, h, h, c, generator=g).to(T16[dt])
    w = (torch.randn(c, c, 3, 3, generator=g) / (9 * c) ** 0.5).to(T16[dt])
    res = torch.randn(n, h, h, c, generator=g).to(T16[dt])
    bias = 0.2 * torch.randn(c, generator=g)
    if variant == "zero_residual":
        res = torch.zeros_like(res)
    elif variant == "zero_weights":
        w = torch.zeros_like(w)
    elif variant == "edge":       # only the last column and the last row of each crop are non-zero
        keep = torch.zeros(1, h, h, 1, dtype=torch.bool)
        keep[:, h - 1, :, :] = True
        keep[:, :, h - 1, :] = True
        x = torch.where(keep, x, torch.zeros_like(x))
    x64, w64 = x.double().permute(0, 3, 1, 2), w.double()
    r64, b64 = res.double().permute(0, 3, 1, 2), bias.double().view(1, -1, 1, 1)
    ref = F.relu(F.conv2d(x64, w64, padding=1) + b64 + r64).permute(0, 2, 3, 1).contiguous()
    a = (F.conv2d(x64.abs(), w64.abs(), padding=1) + b64.abs() + r64.abs()).permute(0, 2, 3, 1)
    tol = _ulp(ref, dt) + 9 * c * 2.0 ** -24 * a
    return x, w, bias, res, ref, tol


def _run_res(h, c, dt, x, w, bias, res):
    from fac_fake_amd.ops import Conv3x3Res
    layer = Conv3x3Res(w.float(), bias, h, dtype=dt, device=DEV)
    # input and residual at exactly their size, the output with nothing around it
    xd, rd = x.to(DEV), res.to(DEV)
    assert xd.numel() == x.shape[0] * h * h * c and rd.numel() == xd.numel()
    out = layer(xd, rd)
    torch.cuda.synchronize()
    assert out.shape == x.shape and out.dtype == T16[dt]
    return out.double().cpu()


def _check(out, ref, tol, what):
    err = (out - ref).abs()
    worst = float((err / tol).max())
    print(f"{what}: max err {float(err.max()):.3e}, max err / tol {worst:.3f}")
    assert torch.isfinite(out).all()
    assert worst <= 1.0, (what, worst)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("h,c", SHAPES)
def test_conv3x3_res_matches_fp64(h, c, dt, n):
    """n = 1: at 7^2 a single partial row tile; n = 3: 147 rows, crop boundaries
    inside tiles and a partial last tile."""
    x, w, bias, res, ref, tol = _case(h, c, dt, n)
    _check(_run_res(h, c, dt, x, w, bias, res), ref, tol, f"conv3x3_res {h} {c} {dt} n={n}")


@pytest.mark.parametrize("variant", ["zero_residual", "zero_weights", "edge"])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("h,c", SHAPES)
def test_conv3x3_res_variants(h, c, dt, variant):
    """Residual all zeros / weights all zeros: a dropped or doubled residual and
    a ReLU before the add show.  Input non-zero only in each crop's last column
    and last row: a pixel that sees the next row's or the next crop's first
    pixel instead of zero padding shows (at 7^2 the row tiles span crops)."""
    x, w, bias, res, ref, tol = _case(h, c, dt, 3, variant)
    out = _run_res(h, c, dt, x, w, bias, res)
    _check(out, ref, tol, f"conv3x3_res {variant} {h} {c} {dt}")
    if variant == "zero_weights":       # relu(bias + residual) exactly, rounded once
        want = F.relu(bias.double().view(1, 1, 1, -1) + res.double()).to(torch.float32).to(T16[dt]).double()
        assert torch.equal(out, want)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("c", [8, 512])
@pytest.mark.parametrize("s", [1, 49])
def test_avgpool_f32_matches_fp64(s, c, n, dt):
    from fac_fake_amd.ops import avgpool_f32
    g = torch.Generator().manual_seed(s * 7 + c + n)
    x = (torch.randn(n, s, c, generator=g) + 0.5).to(T16[dt])
    y = avgpool_f32(x.to(DEV))
    torch.cuda.synchronize()
    assert y.shape == (n, c) and y.dtype == torch.float32
    ref = x.double().mean(1)
    tol = 49 * 2.0 ** -24 * x.double().abs().mean(1)
    err = (y.double().cpu() - ref).abs()
    print(f"avgpool s={s} c={c} n={n} {dt}: max err / tol {float((err / tol).max()):.3f}")
    assert (err <= tol).all()
    assert torch.equal(y, avgpool_f32(x.to(DEV)))       # fixed order, no atomics


def test_error_codes():
    import ctypes
    from fac_fake_amd import _lib
    lib = _lib.load()
    ARG, SHAPE = -1, -2
    for h, c in SHAPES:
        assert lib.fac_conv3x3_res_packed_elems(h, c) == 9 * c * c
    for h, c in [(56, 128), (28, 64), (14, 512), (7, 256), (112, 64), (8, 512), (0, 0), (7, 0), (-7, 512)]:
        assert lib.fac_conv3x3_res_packed_elems(h, c) == 0, (h, c)
    t = torch.zeros(3 * 49 * 512, dtype=torch.float16, device=DEV)
    wpk = torch.zeros(9 * 512 * 512, dtype=torch.float16, device=DEV)
    b = torch.zeros(512, device=DEV)
    o = torch.empty_like(t)
    p = lambda v: v.data_ptr()  # noqa: E731
    good = [1, p(t), p(wpk), p(b), p(t), p(o), 3, 7, 512, None]
    assert lib.fac_conv3x3_res(*good) == 0
    for i in (1, 2, 3, 4, 5):                       # each pointer null
        bad = list(good)
        bad[i] = None
        assert lib.fac_conv3x3_res(*bad) == ARG, i
    for n in (0, -1):
        bad = list(good)
        bad[6] = n
        assert lib.fac_conv3x3_res(*bad) == ARG
    bad = list(good)
    bad[0] = 2
    assert lib.fac_conv3x3_res(*bad) == ARG
    for h, c in [(7, 256), (14, 512), (56, 128), (28, 64), (6, 512), (112, 64)]:
        bad = list(good)
        bad[7], bad[8] = h, c
        assert lib.fac_conv3x3_res(*bad) == SHAPE, (h, c)
    host_w, host_o = torch.zeros(64 * 64 * 9), torch.zeros(64 * 64 * 9, dtype=torch.int16)
    assert lib.fac_conv3x3_res_pack(0, 56, 64, p(host_w), p(host_o)) == 0
    assert lib.fac_conv3x3_res_pack(0, 56, 64, None, p(host_o)) == ARG
    assert lib.fac_conv3x3_res_pack(0, 56, 64, p(host_w), None) == ARG
    assert lib.fac_conv3x3_res_pack(3, 56, 64, p(host_w), p(host_o)) == ARG
    assert lib.fac_conv3x3_res_pack(0, 56, 32, p(host_w), p(host_o)) == SHAPE
    y = torch.empty(3, 512, device=DEV)
    good = [1, p(t), 3, 49, 512, p(y), None]
    assert lib.fac_avgpool_f32(*good) == 0
    for i, v, rc in ((1, None, ARG), (5, None, ARG), (2, 0, ARG), (2, -3, ARG), (0, 7, ARG), (3, 0, SHAPE),
                     (3, -1, SHAPE), (4, 12, SHAPE), (4, 0, SHAPE), (4, 4, SHAPE)):
        bad = list(good)
        bad[i] = v
        assert lib.fac_avgpool_f32(*bad) == rc, (i, v)
    torch.cuda.synchronize()
    assert ctypes.sizeof(ctypes.c_size_t) == 8


# ------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def models():
    from fac_fake_amd.reskan import resnet34
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in make_reskan_state_dict(0).items()}
    out = {}
    for dt in ("fp16", "bf16"):
        m = resnet34(set_device=DEV, num_classes=2, include_top=False, include_top_kan=True, dtype=dt)
        m.load_state_dict(sd)
        out[dt] = m
    return out


@pytest.fixture(scope="module")
def fixture_crops(golden):
    g = golden("reskan_golden_stages.npz")
    return g, torch.from_numpy(reskan_crops_varied(int(g["n_crops"]), seed=int(g["crop_seed"]))).to(DEV)


def _prob_bar(g, dt):
    return 1e-3 if dt == "fp16" else 2 * float(g[f"env_prob_{dt}"])


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_reskan_every_block_matches_reference(models, fixture_crops, dt):
    """8 crops: the per-channel means of the max-pool output, of EVERY BasicBlock
    (downsample and residual included) and the fp32 pooled features against the
    reference module's, within 2x that stage's emulated 16-bit envelope + 1e-4
    (relative to the rms of the reference means); probabilities fp16 within
    1e-3, bf16 within 2x its emulated envelope."""
    g, x = fixture_crops
    n = x.shape[0]
    m = models[dt]
    taps = m.stage_outputs(x)
    torch.cuda.synchronize()
    assert len(taps) == 18
    assert all(t.dtype == T16[dt] for t in taps[:17]) and taps[17].dtype == torch.float32
    env = g[f"env_{dt}"]
    for i, t in enumerate(taps):
        got = t.float().reshape(n, -1, t.shape[-1]).mean(1).double().cpu().numpy()
        ref = g[f"mean_{i}"].astype(np.float64)
        assert got.shape == ref.shape, (i, got.shape, ref.shape)
        err = float(np.abs(got - ref).max() / np.sqrt((ref ** 2).mean()))
        print(f"reskan {dt} tap {i}: err {err:.3e} gate {2 * env[i] + 1e-4:.3e}")
        assert err <= 2 * env[i] + 1e-4, (i, err, env[i])
    lg, pr = m.forward_u8(x, return_probs=True)
    p_ref = 1 / (1 + np.exp(-g["logits"].astype(np.float64)))
    perr = float(np.abs(pr.double().cpu().numpy() - p_ref).max())
    print(f"reskan {dt}: prob err {perr:.3e} bar {_prob_bar(g, dt):.3e}")
    assert lg.shape == (n, 2) and lg.dtype == torch.float32
    assert perr <= _prob_bar(g, dt)
    assert torch.equal(pr, torch.sigmoid(lg)) or float((pr - torch.sigmoid(lg)).abs().max()) <= 1e-6


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_reskan_forward_equals_forward_u8(models, fixture_crops, dt):
    """forward on the normalised fp32 NCHW batch (the reference's call) against
    the reference's probabilities, within the gates of forward_u8."""
    from oracle.cvit_torch import normalize_u8
    g, x = fixture_crops
    m = models[dt]
    img = normalize_u8(x.cpu().numpy()).to(DEV)
    lg = m(img)
    lg8 = m.forward_u8(x, pos_index=torch.arange(x.shape[0], dtype=torch.int32))      # accepted, ignored
    torch.cuda.synchronize()
    p_ref = 1 / (1 + np.exp(-g["logits"].astype(np.float64)))
    for out in (lg, lg8):
        assert out.shape == (x.shape[0], 2) and out.dtype == torch.float32
        assert np.abs(torch.sigmoid(out.double()).cpu().numpy() - p_ref).max() <= _prob_bar(g, dt)
    assert torch.equal(lg8, m.forward_u8(x))


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_reskan_batch_of_33_and_graph_replay(models, fixture_crops, dt):
    """No pos_embedding: a batch of 33 runs, and its first 8 rows are the 8-crop
    result bit for bit (no route of this model depends on the batch size).  A
    captured graph replays the eager forward bit for bit."""
    g, x = fixture_crops
    m = models[dt]
    x33 = torch.cat([x, torch.from_numpy(make_crops(25, seed=3)).to(DEV)])
    lg8 = m.forward_u8(x)
    lg33 = m.forward_u8(x33)
    torch.cuda.synchronize()
    assert lg33.shape == (33, 2) and torch.isfinite(lg33).all()
    assert torch.equal(lg33[:8], lg8)
    static = x33.clone()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.forward_u8(static)
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(graph):
        out = m.forward_u8(static)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, lg33)
    static.copy_(torch.flip(x33, dims=[0]))          # the replay reads its input again
    graph.replay()
    torch.cuda.synchronize()
    flipped = out.clone()
    assert torch.equal(flipped, m.forward_u8(static)) and not torch.equal(flipped, lg33)


def test_reskan_predict_crops(models, fixture_crops):
    """prediction.predict_crops scores a video's crops with this model unchanged
    (it passes pos_index, which the model ignores)."""
    from fac_fake_amd.prediction import pre_process_prediction, pred_sig, predict_crops
    _, x = fixture_crops
    m = models["fp16"]
    want = float(pre_process_prediction(pred_sig(m.forward_u8(x).float().cpu())))
    assert predict_crops(m, x) == want
    assert predict_crops(m, x.cpu()) == want
    assert 0.0 <= want <= 1.0
    # more crops than one batch: video.score_selected's call
    assert torch.equal(m.forward_u8_pipelined(x, torch.arange(8, dtype=torch.int32), chunk=3, equal=False),
                       m.forward_u8(x))
