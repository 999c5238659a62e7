"""The BlazeFace layer kernels (csrc/blazeface.hip: bf_stem, the 13 instances of
bf_block behind the 16 BlazeBlocks, bf_heads) one launch at a time, through
fac_bf_debug_stem / _block / _heads, against the float64 references of
tests/blazeface_ref.py; then run_net's second chunk and bf_tiles at the limits
of its two accumulator types.

Weights are seeded state dicts loaded through load_state_dict; anchors come
from the fixture.  Every launch writes into the middle of a buffer of NaN
between two runs of a sentinel, so an unwritten output and a write outside the
output both show.

* exact    inputs integers in [-3, 3] (stem: pixels in {0, 255} = exactly -1 and
           +1), weights in {-1, 0, 1}, integer biases: every partial sum is an
           integer below 2^24 (asserted in test_blazeface_ref.py), so summation
           order and FMA contraction cannot matter and the output must EQUAL the
           reference.  All 16 block indices run: 12..15 share a kernel instance
           but not their weights.
* random   Gaussian weights and signed Gaussian inputs, T = 1 and 3, every output
           within gamma_n A of float64 (blazeface_ref's docstring derives n and
           A; nothing in the gate is measured).  Observed on an MI355X at T = 3,
           max of |err| / (gamma_n A): stem 0.035, blocks 0.019 .. 0.063 (block 2 the
           largest), heads 0.053.

tests/test_blazeface_ref.py shows on the CPU that eleven wrong kernels (padding,
pooling, channel pad, dropped channels, transposed taps, anchor order) miss
both gates at these shapes and seeds.
"""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import blazeface_ref as R  # noqa: E402
from fac_fake_amd import blazeface as bz  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = Path(__file__).resolve().parent / "golden"
GUARD = 4096              # sentinel floats on each side of an output (keeps the 16-byte alignment)
SENTINEL = -12345.5


def _detector(sd):
    d = bz.BlazeFace().to(DEV)
    d.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    d.load_anchors(GOLDEN / "blazeface_weights.npz")
    return d


@pytest.fixture(scope="module")
def dets(built_lib):
    return {"exact": _detector(R.exact_state_dict()), "random": _detector(R.random_state_dict())}


@pytest.fixture(scope="module")
def trained(built_lib):
    d = bz.BlazeFace().to(DEV)
    d.load_weights(GOLDEN / "blazeface_weights.npz")
    d.load_anchors(GOLDEN / "blazeface_weights.npz")
    return d


@pytest.fixture(scope="module")
def video(golden):
    G = golden("blazeface_golden.npz")
    return G, bz.fixture_input("video", golden("golden_real.npz")["crops"], G["video_paste"])


@functools.lru_cache(maxsize=None)
def _sd(kind):
    return R.exact_state_dict() if kind == "exact" else R.random_state_dict()


@functools.lru_cache(maxsize=None)
def _case(kind, kernel):
    """(inputs, float64 outputs, A) at T = 3, computed once; T = 1 is the first tile."""
    inputs = R.case_inputs(kind, kernel)
    out, mags = R.run_ref(_sd(kind), kernel, inputs)
    return inputs, out, mags


def _out_shapes(kernel, T):
    if kernel == "stem":
        return [(T, 64, 64, 24)]
    if kernel == "heads":
        return [(T, 896, 16), (T, 896)]
    return [(T,) + R.block_shapes(int(kernel[5:]))[1]]


def _launch(det, kernel, inputs):
    """One launch of `kernel` on `inputs` (host arrays); outputs as host arrays.
    Nothing but the outputs was written, and all of each output was."""
    T = inputs[0].shape[0]
    bufs, outs = [], []
    for shape in _out_shapes(kernel, T):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
        buf[GUARD:GUARD + n] = float("nan")
        bufs.append(buf)
        outs.append(buf[GUARD:GUARD + n].view(shape))
    dev_in = [torch.from_numpy(x).to(DEV) for x in inputs]
    if kernel == "stem":
        det.debug_stem(dev_in[0], out=outs[0])
    elif kernel == "heads":
        det.debug_heads(dev_in[0], dev_in[1], out_r=outs[0], out_c=outs[1])
    else:
        det.debug_block(int(kernel[5:]), dev_in[0], out=outs[0])
    torch.cuda.synchronize()
    res = []
    for buf, out in zip(bufs, outs):
        host = buf.cpu().numpy()
        n = out.numel()
        assert (host[:GUARD] == SENTINEL).all(), f"{kernel}: wrote before its output"
        assert (host[GUARD + n:] == SENTINEL).all(), f"{kernel}: wrote behind its output"
        got = host[GUARD:GUARD + n].reshape(tuple(out.shape))
        assert np.isfinite(got).all(), f"{kernel}: {int((~np.isfinite(got)).sum())} outputs not written"
        res.append(got)
    return res


def _assert_equal(kernel, got, want):
    for g, w in zip(got, want):
        bad = g != w
        assert not bad.any(), (f"{kernel}: {int(bad.sum())} of {bad.size} outputs differ, first at "
                               f"{tuple(int(i) for i in np.argwhere(bad)[0])}: {g[bad][0]} for {w[bad][0]}")


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_exact(dets, kernel):
    inputs, want, _ = _case("exact", kernel)
    _assert_equal(kernel, _launch(dets["exact"], kernel, inputs), want)


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("kernel", R.KERNELS)
def test_random_vs_float64(dets, kernel, T):
    inputs, want, mags = _case("random", kernel)
    got = _launch(dets["random"], kernel, [x[:T] for x in inputs])
    worst = R.worst_ratio(kernel, got, [w[:T] for w in want], [a[:T] for a in mags])
    print(f"{kernel} T={T}: max |err| / (gamma_n A) = {worst:.4f}")
    assert worst <= 1.0, (kernel, T, worst)
    if kernel != "stem":      # signed inputs: the case has negative values for the residual to carry
        assert all(float(x.min()) < -1 for x in inputs)


def test_stem_edge_tiles(dets):
    """All 0, all 255, and 255 only in the last two rows and columns, exact: a
    padded tap is 0 (not -1, which the all-0 tile's border would show), and the
    pad is (1, 2, 1, 2)."""
    sd, tiles = _sd("exact"), R.stem_edge_tiles()
    want, _ = R.stem_ref(tiles, sd["backbone1.0.weight"], sd["backbone1.0.bias"])
    _assert_equal("stem", _launch(dets["exact"], "stem", [tiles]), [want])


@pytest.mark.parametrize("kernel", ["stem", "block1", "block2", "block11", "heads"])
def test_tile_does_not_depend_on_its_batch(dets, kernel):
    """Tile 2 of a T = 3 launch and the same tile alone: the same bits (block 1 is
    stride 1 with a channel pad; blocks 2 and 11 are stride 2, 4 and 16 waves)."""
    inputs, _, _ = _case("random", kernel)
    full = _launch(dets["random"], kernel, inputs)
    alone = _launch(dets["random"], kernel, [x[2:3] for x in inputs])
    for f, a in zip(full, alone):
        assert np.array_equal(f[2:3], a)


# ------------------------------------------------------------- second chunk
def test_second_chunk_of_the_net(trained, video):
    """513 tiles: run_net's second pass holds one tile, and tiles 510..512 straddle
    the pass boundary.  They equal the same three tiles run alone."""
    G, frames = video
    six = bz.tile_frames_np(frames)
    idx = np.arange(513) % 6
    assert idx[512] == 2 and int(G["video_tile_counts"][2]) > 0
    tiles = torch.from_numpy(six[idx]).to(DEV)
    last = tiles[510:513].clone()
    full = trained.debug_net(tiles)
    alone = trained.debug_net(last)
    for name, f, a in zip(("b1", "b2", "r", "c"), full, alone):
        assert torch.equal(f[510:513], a), name
    # and the pass before it is not disturbed: tile 0 == tile 6 == tile 510 (the same image)
    for f in full:
        assert torch.equal(f[0], f[6]) and torch.equal(f[0], f[510])
    got = trained.predict_on_batch(tiles, apply_nms=False)
    want = trained.predict_on_batch(last, apply_nms=False)
    assert len(got) == 513 and int(got[512].shape[0]) == int(G["video_tile_counts"][2]) > 0
    for g, w in zip(got[510:], want):
        assert torch.equal(g, w)
    assert [int(d.shape[0]) for d in got[:6]] == G["video_tile_counts"].tolist()


def test_detect_across_the_chunk_boundary(trained, video):
    """172 frames = 516 tiles; frame 170's tiles are 510, 511, 512."""
    G, frames = video
    fr = torch.from_numpy(frames).to(DEV)
    many = fr.repeat(86, 1, 1, 1)
    assert many.shape[0] == 172 and 170 * 3 == 510
    dets, boxes, counts, over = trained.detect(many)
    d2, b2, c2, o2 = trained.detect(many[170:172].clone())
    assert torch.equal(counts[170:], c2) and torch.equal(over[170:], o2)
    assert counts[170:].tolist() == G["video_nms_counts"].tolist() == [2, 0]
    for f in range(2):
        n = int(c2[f])
        assert torch.equal(dets[170 + f, :n], d2[f, :n])
        assert torch.equal(boxes[170 + f, :n, 1:], b2[f, :n, 1:])
        assert boxes[170 + f, :n, 0].tolist() == [170 + f] * n and b2[f, :n, 0].tolist() == [f] * n
    assert torch.equal(counts, c2.repeat(86)) and not bool(over.any())


# ------------------------------------------------ tile sums at the limits
@pytest.mark.parametrize("H,Wd", [(2048, 2048), (2049, 2049), (2049, 2051)],
                         ids=["u32-at-2048", "u64-at-2049", "u64-three-windows"])
def test_tile_sums_at_the_accumulator_limit(trained, H, Wd):
    """A frame of 255 with a sparse grid of other values: 2048 px is the uint32_t
    variant at its bound (2 * 255 n^2 + n^2 = 2143289344), 2049 the first
    uint64_t size, 2049 x 2051 three windows one pixel apart."""
    fr = R.limit_frame(H, Wd)
    split, x_step, n = bz.tile_windows(H, Wd)
    assert (split <= 2048) == (H == 2048) and (x_step, n) == ((1, 3) if Wd > H else (0, 1))
    want = R.tile_frames_ref(fr)
    got = trained.tiles(torch.from_numpy(fr).to(DEV)).cpu().numpy()
    assert got.shape == want.shape == (n, 128, 128, 3)
    bad = got != want
    assert not bad.any(), (int(bad.sum()), tuple(int(i) for i in np.argwhere(bad)[0]))
    assert int((want != 255).sum()) > 1000         # the grid reaches the output
