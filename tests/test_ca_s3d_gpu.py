"""CA_S3D_v3 on the GPU: the context-block kernels (csrc/context.hip) against
the fp64 restatement, and the model against outputs of the reference module
(tests/golden/ca_s3d_*, tools/make_golden_ca_s3d.py)."""
import ctypes
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import ca_s3d_ref as R  # noqa: E402
from fac_fake_amd.weights import make_ca_s3d_state_dict, s3d_clips, s3d_clips_varied  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
ROUTES = {"clip": 1, "split": 2}

# (n, T, H, W, C, P): the six maps of CA_S3D_v3 at 16 x 112^2 and 20 x 224^2
# clips with P = int(C / 16) (P = 33, 52: no multiple of anything; (2,1,5,5,16):
# P = 1, where LayerNorm over one value gives ln_b), then s = 65 (one full
# 64-row chunk of the split route and one row more) at a width whose 16-byte
# column count (3) divides no workgroup size, s = 128 (two full chunks) at the
# widest bottleneck (P = 64), and c = 8 (one column, 512 row groups).
OP_SHAPES = [(3, 2, 3, 3, 832, 52), (2, 4, 7, 7, 528, 33), (2, 8, 14, 14, 256, 16), (2, 5, 14, 14, 512, 32),
             (1, 10, 28, 28, 256, 16), (2, 1, 5, 5, 16, 1), (2, 1, 13, 5, 24, 3), (2, 2, 8, 8, 1024, 64),
             (2, 1, 9, 9, 8, 2)]


def _weights(c, p, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(p, c, generator=g) / c ** 0.5, 0.02 * torch.randn(p, generator=g),
            0.5 + torch.rand(p, generator=g), torch.rand(p, generator=g) - 0.5,
            torch.randn(c, p, generator=g) / p ** 0.5, 0.1 * torch.randn(c, generator=g))


@functools.lru_cache(maxsize=None)
def _case(shape, dt):
    """x16 (clips of independent content and different means), the weights, and
    the CPU restatement's term in fp64 and in fp32: computed once per shape and
    dtype, shared by every test that needs it."""
    n, t, h, w, c, p = shape
    g = torch.Generator().manual_seed(1000 + c + 7 * n + t)
    means = 0.3 * (1 + torch.arange(n, dtype=torch.float32)).view(n, 1, 1, 1, 1)
    x16 = (0.5 * torch.randn(n, t, h, w, c, generator=g) + means * (0.5 + torch.rand(n, 1, 1, 1, c, generator=g))).to(T16[dt])
    wts = _weights(c, p, 17 + c)
    _, term64 = R.context_add_ref(x16, wts, torch.float64)
    _, term32 = R.context_add_ref(x16, wts, torch.float32)
    return x16, wts, term64, term32


def _layer(wts, dt):
    from fac_fake_amd.ops import ContextAdd
    return ContextAdd(*wts, eps=R.LN_EPS, dtype=dt, device=DEV)


@pytest.mark.parametrize("route", ["clip", "split"])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", OP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_context_add_parity(shape, dt, route):
    """term within 4 E of the fp64 restatement, E = the fp32 torch
    restatement's own distance from fp64 on the same inputs + 1e-6 rms(term)
    (the rule of the BlazeFace tests); out bit-equal to round16(float(x) +
    term) of the kernel's own term; in place equal to out of place."""
    n, t, h, w, c, p = shape
    x16, wts, term64, term32 = _case(shape, dt)
    rms = float(term64.pow(2).mean().sqrt())
    E = float((term32.double() - term64).abs().max()) + 1e-6 * rms
    if n > 1 and p > 1:   # (P = 1: LayerNorm of one value is ln_b for every clip, the term cannot differ)
        spread = float((term64[:, None, :] - term64[None, :, :]).abs().max())
        assert spread > 100 * 4 * E, (spread, E)
    layer = _layer(wts, dt)
    x = x16.to(DEV)
    out, term = layer(x, route=ROUTES[route], return_term=True)
    torch.cuda.synchronize()
    err = float((term.double().cpu() - term64).abs().max())
    print(f"context_add {shape} {dt} {route}: |term - fp64| {err:.3e}  E {E:.3e}  rms {rms:.3e}")
    assert torch.equal(x, x16.to(DEV)), "the input was written"
    assert err <= 4 * E, (err, E)
    want = (x.float() + term.view(n, 1, 1, 1, c)).to(T16[dt])
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))
    y = x.clone()
    assert layer(y, inplace=True, route=ROUTES[route]) is y
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int16), out.view(torch.int16))


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_context_add_auto_route_is_one_of_the_two(dt):
    """route 0 gives, bit for bit, what one of the forced routes gives."""
    for shape in (OP_SHAPES[0], OP_SHAPES[2]):
        x16, wts, _, _ = _case(shape, dt)
        layer, x = _layer(wts, dt), x16.to(DEV)
        auto, ta = layer(x, return_term=True)
        forced = [layer(x, route=r, return_term=True) for r in (1, 2)]
        torch.cuda.synchronize()
        assert any(torch.equal(ta, tf) and torch.equal(auto.view(torch.int16), of.view(torch.int16))
                   for of, tf in forced)


@pytest.mark.parametrize("route", ["clip", "split"])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_context_add_batch_independence(dt, route):
    """Clip k run alone is bit-equal to clip k inside a batch of 3."""
    for shape in (OP_SHAPES[0], (3, 4, 7, 7, 528, 33), (3, 3, 14, 14, 256, 16)):
        x16, wts, _, _ = _case(shape, dt)
        layer, x = _layer(wts, dt), x16.to(DEV)
        out, term = layer(x, route=ROUTES[route], return_term=True)
        for k in range(3):
            o1, t1 = layer(x[k:k + 1].contiguous(), route=ROUTES[route], return_term=True)
            torch.cuda.synchronize()
            assert torch.equal(t1[0], term[k]), (shape, k)
            assert torch.equal(o1[0].view(torch.int16), out[k].view(torch.int16)), (shape, k)


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", [(8, 14, 14, 256, 16), (4, 7, 7, 512, 32), (5, 14, 14, 512, 32)],
                         ids=lambda s: "x".join(map(str, s)))
def test_context_add_route0_does_not_depend_on_the_batch(shape, dt):
    """The default route picks per-clip or split from (s, c) alone
    (fac_context_route), never from n: the two routes add the pool in different
    orders, so a choice by n would change a clip's term with its batch.  Clips
    above (0.8 MB, 1 MB) and below (0.2 MB) the 256 KB switch, alone, in a
    batch of 3 and in a batch of 300 (more clips than the GPU has CUs): term
    and output bit-equal."""
    from fac_fake_amd import _lib
    t, h, w, c, p = shape
    s = t * h * w
    assert _lib.load().fac_context_route(s, c) == (1 if s * c * 2 <= 256 * 1024 else 2)
    g = torch.Generator().manual_seed(s + c)
    clips = (0.5 * torch.randn(3, s, c, generator=g) + 0.4).to(T16[dt]).to(DEV)
    layer = _layer(_weights(c, p, 23), dt)
    big = clips.repeat(100, 1, 1)                       # clip k of 300 is clips[k % 3]
    out300, term300 = layer(big, return_term=True)
    out3, term3 = layer(clips, return_term=True)
    torch.cuda.synchronize()
    for k in (0, 1, 2, 151, 299):
        o1, t1 = layer(clips[k % 3:k % 3 + 1].contiguous(), return_term=True)
        torch.cuda.synchronize()
        assert torch.equal(t1[0], term300[k]) and torch.equal(t1[0], term3[k % 3]), k
        assert torch.equal(o1[0].view(torch.int16), out300[k].view(torch.int16)), k
        assert torch.equal(o1[0].view(torch.int16), out3[k % 3].view(torch.int16)), k


def test_context_add_rejects_misaligned_views():
    """The kernels load and store 16-byte vectors: a view 8 bytes into a buffer is refused, by
    ContextAdd and by the C entry point (FAC_ERR_ARG), before anything is launched."""
    from fac_fake_amd import _lib
    c, s = 16, 6
    buf = torch.zeros(4 + s * c, dtype=torch.float16, device=DEV)
    x = buf[4:].view(1, s, c)
    layer = _layer(_weights(c, 1, 2), "fp16")
    with pytest.raises(ValueError, match="16-byte"):
        layer(x)
    rc = _lib.load().fac_context_add(1, x.data_ptr(), 1, s, c, 1, layer.w0.data_ptr(), layer.b0.data_ptr(),
                                     layer.ln_w.data_ptr(), layer.ln_b.data_ptr(), ctypes.c_float(1e-5),
                                     layer.w3t.data_ptr(), layer.b3.data_ptr(), x.data_ptr(), None, None, 1,
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == -1


@pytest.mark.parametrize("route", ["clip", "split"])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("nsc", [(2, 65, 528), (3, 18, 832), (2, 130, 16)], ids=lambda v: "x".join(map(str, v)))
def test_context_add_stays_inside_its_views(nsc, dt, route):
    """x is a view into the middle of a buffer whose other elements are 16-bit
    NaN, out a view into a sentinel-filled buffer; the last chunk (s = 65, 130:
    partly full) and the last clip end exactly where the views end.  A read
    outside x would put NaN into term; a write outside out would break a sentinel."""
    n, s, c = nsc
    p = max(1, c // 16)
    pad = 4096
    g = torch.Generator().manual_seed(5 + s)
    body = (0.5 * torch.randn(n, s, c, generator=g) + 0.4).to(T16[dt])
    xbuf = torch.full((pad + body.numel() + pad,), float("nan"), dtype=T16[dt], device=DEV)
    xbuf[pad:pad + body.numel()] = body.reshape(-1).to(DEV)
    x = xbuf[pad:pad + body.numel()].view(n, s, c)
    sentinel = 0x5A5A
    obuf = torch.full((pad + body.numel() + pad,), sentinel, dtype=torch.int16, device=DEV)
    out = obuf[pad:pad + body.numel()].view(T16[dt]).view(n, s, c)
    wts = _weights(c, p, 3)
    layer = _layer(wts, dt)
    _, term = layer(x, out=out, route=ROUTES[route], return_term=True)
    torch.cuda.synchronize()
    assert torch.isfinite(term).all()
    assert bool((obuf[:pad] == sentinel).all()) and bool((obuf[pad + body.numel():] == sentinel).all())
    assert torch.isnan(xbuf[:pad]).all() and torch.isnan(xbuf[pad + body.numel():]).all()
    want = (body.to(DEV).float() + term.view(n, 1, c)).to(T16[dt])
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))
    _, term64 = R.context_add_ref(body, wts, torch.float64)
    assert (term.double().cpu() - term64).abs().max() <= 1e-4 * float(term64.abs().max())


def test_context_add_abi_errors():
    """Bad c, p, n, s -> FAC_ERR_SHAPE; a null pointer or a bad route ->
    FAC_ERR_ARG; nothing is launched (out keeps its sentinel)."""
    from fac_fake_amd import _lib
    lib = _lib.load()
    n, s, c, p = 2, 10, 32, 2
    x = torch.zeros(n, s, c, dtype=torch.float16, device=DEV)
    out = torch.full((n, s, c), 3.0, dtype=torch.float16, device=DEV)
    w = [t.to(DEV) for t in _weights(c, p, 1)]
    w[4] = w[4].t().contiguous()
    scratch = torch.empty(max(lib.fac_context_scratch_bytes(n, s, c) // 4, 1), dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(x_=x.data_ptr(), n_=n, s_=s, c_=c, p_=p, route=0, w0=w[0].data_ptr(), scratch_=scratch.data_ptr()):
        return lib.fac_context_add(1, x_, n_, s_, c_, p_, w0, w[1].data_ptr(), w[2].data_ptr(), w[3].data_ptr(),
                                   ctypes.c_float(1e-5), w[4].data_ptr(), w[5].data_ptr(), out.data_ptr(), None,
                                   scratch_, route, st)
    SHAPE, ARG = -2, -1
    assert call(c_=12) == SHAPE and call(c_=0) == SHAPE and call(c_=4104) == SHAPE
    assert call(p_=0) == SHAPE and call(p_=65) == SHAPE
    assert call(n_=0) == SHAPE and call(s_=0) == SHAPE
    assert call(route=3) == ARG and call(route=-1) == ARG
    assert call(x_=None) == ARG and call(w0=None) == ARG and call(route=2, scratch_=None) == ARG
    assert lib.fac_context_scratch_bytes(n, s, 12) == 0 and lib.fac_context_scratch_bytes(0, s, c) == 0
    assert lib.fac_context_scratch_bytes(n, 65, c) == (n * 2 * c + n * c) * 4
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    assert call() == 0 and call(route=1, scratch_=None) == 0
    torch.cuda.synchronize()
    assert not bool((out == 3.0).all())


def test_context_block_dropin_forward():
    """ContextBlock3d.forward on the reference's [N, C, T, H, W] layout."""
    from fac_fake_amd.ca_s3d import ContextBlock3d
    torch.manual_seed(3)
    blk = ContextBlock3d(inplanes=64, ratio=1. / 16., pooling_type="avg")
    with torch.no_grad():
        blk.channel_add_conv[1].weight.uniform_(0.5, 1.5)
        blk.channel_add_conv[1].bias.uniform_(-0.5, 0.5)
    x = (torch.randn(2, 64, 3, 5, 5) + 0.5).half().float()
    a = blk.channel_add_conv
    wts = (a[0].weight.detach().reshape(4, 64), a[0].bias.detach(), a[1].weight.detach().reshape(4),
           a[1].bias.detach().reshape(4), a[3].weight.detach().reshape(64, 4), a[3].bias.detach())
    ref, _ = R.context_add_ref(x.permute(0, 2, 3, 4, 1).half(), wts, torch.float64)
    xd = x.to(DEV)
    y = blk(xd)
    torch.cuda.synchronize()
    assert y.shape == x.shape and y.dtype == x.dtype and torch.equal(xd.cpu(), x)
    assert (y.cpu().double() - ref.permute(0, 4, 1, 2, 3)).abs().max() <= 2 ** -10 * float(ref.abs().max())


# ---------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def ca_models():
    from fac_fake_amd.ca_s3d import CA_S3D_v3
    out = {}
    for srm in ("no", "yes"):
        sd = {k: torch.from_numpy(np.asarray(v)) for k, v in make_ca_s3d_state_dict(0, 1, srm == "yes").items()}
        for dt in ("fp16", "bf16"):
            m = CA_S3D_v3(1, srm, dtype=dt)
            m.load_state_dict(sd)
            out[(srm, dt)] = m
    return out


@pytest.fixture(scope="module")
def block_clips(golden):
    g = R.load_blocks(golden)
    return g, torch.from_numpy(s3d_clips_varied(int(g["n_clips"]), 16, 112, int(g["clip_seed"]))).to(DEV)


def _rel_to_rms(got, ref):
    return float(np.abs(got - ref).max() / (np.sqrt((ref.astype(np.float64) ** 2).mean()) + 1e-30))


def _every_block(m, g, x, srm, dt):
    taps = m.base_outputs(x)
    torch.cuda.synchronize()
    assert len(taps) == 22
    env = g[f"env_{srm}_{dt}"]
    for i, t in enumerate(taps):
        got = t.float().mean(dim=(1, 2, 3)).double().cpu().numpy()
        ref = g[f"mean_{srm}_{i}"].astype(np.float64)
        assert got.shape == ref.shape, (i, got.shape, ref.shape)
        err = _rel_to_rms(got, ref)
        print(f"ca_s3d {srm} {dt} route {m.ctx_route} base.{i}: err {err:.3e} gate {2 * env[i] + 1e-4:.3e}")
        assert err <= 2 * env[i] + 1e-4, (i, err, env[i])
    lg, pr = m(x, return_probs=True)
    torch.cuda.synchronize()
    p_ref = 1 / (1 + np.exp(-g[f"logits_{srm}"].astype(np.float64)))
    bar = 1e-3 if dt == "fp16" else 2 * float(g[f"env_prob_{srm}_{dt}"])
    dp = np.abs(pr.double().cpu().numpy() - p_ref).max()
    print(f"ca_s3d {srm} {dt} route {m.ctx_route}: |dp| {dp:.3e} bar {bar:.3e} "
          f"|dlogit| {np.abs(lg.double().cpu().numpy() - g[f'logits_{srm}']).max():.3e}")
    assert dp <= bar, (dp, bar)
    dl = float(np.abs(lg.double().cpu().numpy() - g[f"logits_{srm}"]).max())
    assert dl <= R.logit_gate(g, g, srm, dt), (dl, R.logit_gate(g, g, srm, dt))
    return lg


@pytest.mark.parametrize("srm", ["no", "yes"])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_ca_s3d_every_block_matches_reference(ca_models, block_clips, srm, dt):
    """8 content-varied clips: the per-channel means of all 22 base[i] outputs
    (the six context blocks' among them; a tap of a Mixed block keeps its
    pre-context tensor) within 2 env[i] + 1e-4 of the reference module's;
    probabilities within 1e-3 (fp16), 2 env_prob (bf16)."""
    g, x = block_clips
    _every_block(ca_models[(srm, dt)], g, x, srm, dt)


@pytest.mark.parametrize("route", [1, 2])
@pytest.mark.parametrize("srm,dt", [("no", "fp16"), ("yes", "bf16")])
def test_ca_s3d_forced_routes_pass_the_every_block_gate(ca_models, block_clips, srm, dt, route):
    g, x = block_clips
    m = ca_models[(srm, dt)]
    m.ctx_route = route
    try:
        _every_block(m, g, x, srm, dt)
    finally:
        del m.ctx_route
    assert m.ctx_route == 0


@pytest.mark.parametrize("srm", ["no", "yes"])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_ca_s3d_reference_harness_shape(ca_models, golden, srm, dt):
    """2 clips of 20 x 224 x 224 vs the reference module: fp16 within 1e-3,
    bf16 within bf16_gate(env_prob); and, since probabilities near 0.999 hardly
    move, the logits within ca_s3d_ref.logit_gate (the only pin of the split
    route inside the model at this shape)."""
    from conftest import bf16_gate
    g = golden("ca_s3d_golden_20x224.npz")
    x = torch.from_numpy(s3d_clips_varied(2, int(g["frames"]), int(g["size"]), seed=int(g["clip_seed"]))).to(DEV)
    lg, pr = ca_models[(srm, dt)](x, return_probs=True)
    torch.cuda.synchronize()
    p_ref = 1 / (1 + np.exp(-g[f"logits_{srm}"].astype(np.float64)))
    tol = 1e-3 if dt == "fp16" else bf16_gate(float(g[f"env_prob_{srm}_bf16"]))
    assert lg.shape == (2, 1)
    assert np.abs(pr.cpu().numpy() - p_ref).max() <= tol, (np.abs(pr.cpu().numpy() - p_ref).max(), tol)
    dl, gate = float(np.abs(lg.double().cpu().numpy() - g[f"logits_{srm}"]).max()), R.logit_gate(R.load_blocks(golden), g, srm, dt)
    print(f"ca_s3d 20x224 {srm} {dt}: |dlogit| {dl:.3e} gate {gate:.3e}")
    assert dl <= gate, (dl, gate)


@pytest.mark.parametrize("srm", ["no", "yes"])
def test_ca_s3d_uint8_clip_equals_its_float_copy(ca_models, srm):
    x = torch.from_numpy(s3d_clips(2, 16, 112, seed=9)).to(DEV)
    m = ca_models[(srm, "fp16")]
    lg, lg8 = m(x), m(x.to(torch.uint8))
    torch.cuda.synchronize()
    assert torch.isfinite(lg).all() and torch.equal(lg8, lg)


def test_ca_s3d_graph_replay_matches_eager(ca_models):
    m = ca_models[("yes", "bf16")]
    x = torch.from_numpy(s3d_clips(3, 16, 112, seed=5)).to(DEV)
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


def test_ca_s3d_video_predictions(ca_models, block_clips):
    """S3D-test.py's per-video score for the 8 clips in batches of 3 (ragged
    last batch): the reference's probabilities within 1e-3 (fp16)."""
    from fac_fake_amd.ca_s3d import custom_round, video_predictions
    g, x = block_clips
    preds = video_predictions(ca_models[("no", "fp16")], x, batch=3)
    p_ref = 1 / (1 + np.exp(-g["logits_no"].astype(np.float64)))[:, 0]
    assert len(preds) == 8 and np.abs(np.array(preds) - p_ref).max() <= 1e-3
    assert np.array_equal(custom_round(preds), custom_round(p_ref))
    dl = np.abs(np.log(np.array(preds) / (1 - np.array(preds))) - g["logits_no"][:, 0].astype(np.float64)).max()
    assert dl <= R.logit_gate(g, g, "no", "fp16") + 1e-3, dl   # (+1e-3: the fp32 sigmoid and its inverse at p = 0.998)
