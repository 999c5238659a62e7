"""Float64 references of the BlazeFace layer kernels (csrc/blazeface.hip), written
from the semantics in that file's header comment, plus the operands and the
error bound that tests/test_blazeface_ref.py (CPU) and
tests/test_blazeface_layers_gpu.py share.

Layout is the kernels': activations NHWC, weights as the state_dict holds them
(conv weight [cout, cin / groups, kh, kw]).

    stem    x / 127.5 - 1, zero pad (1, 2, 1, 2) AFTER the normalisation (a padded
            tap is 0, not -1), conv 5x5 stride 2, 3 -> 24, bias, ReLU.
    block   depthwise 3x3 + bias (stride 1: pad 1; stride 2: pad (0, 2, 0, 2), no
            leading pad), pointwise 1x1 + bias, residual (stride 1: the input;
            stride 2: its 2x2 max-pool; channels beyond cin get nothing: the zero
            channel pad is appended at the end), ReLU.
    heads   16x16 map: classifier_8 (2 scores) and regressor_8 (32 coordinates)
            per pixel -> anchors 0..511 (pixel-major, 2 per pixel); 8x8 map:
            classifier_16 (6) and regressor_16 (96) -> anchors 512..895.

Every function returns (out, A).  A is the same computation on the absolute
values of inputs, weights and biases with every subtraction an addition (the
stem's input magnitude is x / 127.5 + 1) and the residual's magnitude added: the
running error bound's magnitude.  A float32 evaluation with n rounded
operations on the path of an output, in ANY summation order and with or
without FMA contraction, is within gamma_n A of the exact value,
gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of
Numerical Algorithms, section 3.1: each rounding multiplies a partial result
by (1 + d), |d| <= u; a term passes through at most n of them).  n per kernel:

    block   9 depthwise FMAs + 1, cin pointwise FMAs + 1, the residual add: 9 + 1 + cin + 1 + 1
    stem    the division and the subtraction of the normalisation, 75 FMAs + 1:  75 + 1 + 2
    heads   cin FMAs + 1:                                                         cin + 1

(the bias starts the accumulator unrounded; the + 1 are slack, ReLU and max are
exact).  The float64 reference's own rounding (u = 2^-53) is 2^-29 of that.

``mutant=`` turns one piece of the arithmetic into a plausible wrong kernel;
tests/test_blazeface_ref.py shows that the checks reject each of them.
"""
import zlib

import numpy as np

from fac_fake_amd import blazeface as bz

U = 2.0 ** -24
BLOCKS = bz.BLOCKS1 + bz.BLOCKS2                       # (cin, cout, stride) of block 0..15
PREFIX = [f"backbone1.{i + 2}" for i in range(11)] + [f"backbone2.{i}" for i in range(5)]
KERNELS = ["stem"] + [f"block{i}" for i in range(16)] + ["heads"]
T_CASE = 3                                             # tiles per launch of the layer cases

MUTANTS = {
    # name: the kernels it applies to
    "dw_s2_pad_1111": [f"block{i}" for i, b in enumerate(BLOCKS) if b[2] == 2],
    "stem_pad_before_norm": ["stem"],
    "stem_pad_2121": ["stem"],
    "pool_top_left": [f"block{i}" for i, b in enumerate(BLOCKS) if b[2] == 2],
    "pool_relu": [f"block{i}" for i, b in enumerate(BLOCKS) if b[2] == 2],
    "channel_pad_front": [f"block{i}" for i, b in enumerate(BLOCKS) if b[1] > b[0]],
    "residual_drops_last_channel": [f"block{i}" for i in range(16)],
    "pw_drops_tail_channels": [f"block{i}" for i, b in enumerate(BLOCKS) if b[1] % 16],
    "dw_taps_transposed": [f"block{i}" for i in range(16)],
    "heads_columns_swapped": ["heads"],
    "heads_8x8_anchors_from_0": ["heads"],
}


def gamma(n: int) -> float:
    return n * U / (1 - n * U)


def bounds(kernel: str, mags):
    """gamma_n A of every output of `kernel`, n the rounded float32 operations on its path."""
    if kernel == "stem":
        return (gamma(75 + 1 + 2) * mags[0],)
    if kernel == "heads":                              # cin is 88 for the anchors of the 16x16 map, 96 for the rest
        out = []
        for a in mags:
            g = np.full(a.shape, gamma(96 + 1))
            g[:, :512] = gamma(88 + 1)
            out.append(g * a)
        return tuple(out)
    return (gamma(9 + 1 + BLOCKS[int(kernel[5:])][0] + 1 + 1) * mags[0],)


def block_shapes(i: int):
    h = 64
    for k, (cin, cout, stride) in enumerate(BLOCKS):
        if k == i:
            return (h, h, cin), (h // stride, h // stride, cout)
        h //= stride


# ------------------------------------------------------------------ the kernels
def stem_ref(tiles, w, b, dt=np.float64, mutant=None):
    """uint8 [T, 128, 128, 3], w [24, 3, 5, 5], b [24] -> (out, A) [T, 64, 64, 24]."""
    w, b = np.asarray(w, dt), np.asarray(b, dt)
    pad = ((0, 0), (2, 1), (2, 1), (0, 0)) if mutant == "stem_pad_2121" else ((0, 0), (1, 2), (1, 2), (0, 0))
    if mutant == "stem_pad_before_norm":
        x = np.pad(tiles.astype(dt), pad) / dt(127.5) - dt(1)
        ax = np.pad(tiles.astype(dt), pad) / dt(127.5) + dt(1)
    else:
        x = np.pad(tiles.astype(dt) / dt(127.5) - dt(1), pad)
        ax = np.pad(tiles.astype(dt) / dt(127.5) + dt(1), pad)
    T = tiles.shape[0]
    acc = np.broadcast_to(b, (T, 64, 64, 24)).copy()
    mag = np.broadcast_to(np.abs(b), (T, 64, 64, 24)).copy()
    for ky in range(5):
        for kx in range(5):
            tap = w[:, :, ky, kx].T                    # [3, 24]
            acc += x[:, ky:ky + 127:2, kx:kx + 127:2] @ tap
            mag += ax[:, ky:ky + 127:2, kx:kx + 127:2] @ np.abs(tap)
    return np.maximum(acc, 0), mag


def block_ref(x, dw_w, dw_b, pw_w, pw_b, stride, dt=np.float64, mutant=None):
    """x [T, h, h, cin], dw_w [cin, 1, 3, 3], pw_w [cout, cin, 1, 1] -> (out, A) [T, h / stride, h / stride, cout]."""
    x = np.asarray(x, dt)
    dw_w, dw_b, pw_w, pw_b = (np.asarray(v, dt) for v in (dw_w, dw_b, pw_w, pw_b))
    T, h, _, cin = x.shape
    cout, ho = pw_w.shape[0], h // stride
    k = dw_w[:, 0]                                     # [cin, ky, kx]
    if mutant == "dw_taps_transposed":
        k = k.transpose(0, 2, 1)
    lead = 1 if (stride == 1 or mutant == "dw_s2_pad_1111") else 0
    pad = ((0, 0), (lead, 2 - lead), (lead, 2 - lead), (0, 0))
    xp = np.pad(x, pad)
    d = np.broadcast_to(dw_b, (T, ho, ho, cin)).copy()
    ad = np.broadcast_to(np.abs(dw_b), (T, ho, ho, cin)).copy()
    span = stride * (ho - 1) + 1
    for ky in range(3):
        for kx in range(3):
            win = xp[:, ky:ky + span:stride, kx:kx + span:stride]
            d += win * k[:, ky, kx]
            ad += np.abs(win) * np.abs(k[:, ky, kx])
    p = d @ pw_w[:, :, 0, 0].T + pw_b
    ap = ad @ np.abs(pw_w[:, :, 0, 0]).T + np.abs(pw_b)
    if mutant == "pw_drops_tail_channels":
        p[..., cout // 16 * 16:] = 0
    if stride == 1:
        res = x
    elif mutant == "pool_top_left":
        res = x[:, ::2, ::2]
    else:
        res = x.reshape(T, ho, 2, ho, 2, cin).max(axis=(2, 4))
        if mutant == "pool_relu":
            res = np.maximum(res, 0)
    if mutant == "residual_drops_last_channel":
        res = res.copy()
        res[..., cin - 1] = 0
    lo = cout - cin if mutant == "channel_pad_front" else 0
    p[..., lo:lo + cin] += res
    ap[..., lo:lo + cin] += np.abs(res)
    return np.maximum(p, 0), ap


def heads_ref(b1, b2, c8w, c8b, r8w, r8b, c16w, c16b, r16w, r16b, dt=np.float64, mutant=None):
    """b1 [T, 16, 16, 88], b2 [T, 8, 8, 96] -> ((r [T, 896, 16], c [T, 896]), (A_r, A_c))."""
    T = b1.shape[0]
    r, c = np.zeros((T, 896, 16), dt), np.zeros((T, 896), dt)
    ar, ac = np.zeros((T, 896, 16), dt), np.zeros((T, 896), dt)
    start = 0
    for x, cw, cb, rw, rb in ((b1, c8w, c8b, r8w, r8b), (b2, c16w, c16b, r16w, r16b)):
        x = np.asarray(x, dt).reshape(T, -1, x.shape[-1])          # [T, pixels, cin]
        wt = np.concatenate([np.asarray(cw, dt)[:, :, 0, 0], np.asarray(rw, dt)[:, :, 0, 0]])   # [ns + 16 ns, cin]
        bias = np.concatenate([np.asarray(cb, dt), np.asarray(rb, dt)])
        ns, npix = cw.shape[0], x.shape[1]
        v = x @ wt.T + bias
        av = np.abs(x) @ np.abs(wt).T + np.abs(bias)
        if mutant == "heads_columns_swapped":          # coordinates taken from the front, scores from the back
            v = np.concatenate([v[..., 16 * ns:], v[..., :16 * ns]], -1)
        n = npix * ns
        at = 0 if (mutant == "heads_8x8_anchors_from_0" and start) else start
        c[:, at:at + n] = v[..., :ns].reshape(T, n)
        r[:, at:at + n] = v[..., ns:].reshape(T, n, 16)
        ac[:, start:start + n] = av[..., :ns].reshape(T, n)
        ar[:, start:start + n] = av[..., ns:].reshape(T, n, 16)
        start += n
    return (r, c), (ar, ac)


def block_weights(sd, i):
    p = PREFIX[i]
    return [np.asarray(sd[f"{p}.convs.{j}.{k}"]) for j in (0, 1) for k in ("weight", "bias")]


def head_weights(sd):
    return [np.asarray(sd[f"{n}.{k}"]) for n in ("classifier_8", "regressor_8", "classifier_16", "regressor_16")
            for k in ("weight", "bias")]


def run_ref(sd, kernel, inputs, dt=np.float64, mutant=None):
    """The reference of one kernel of KERNELS with the weights of state dict `sd`:
    (tuple of outputs, tuple of their A)."""
    if kernel == "stem":
        out, a = stem_ref(inputs[0], sd["backbone1.0.weight"], sd["backbone1.0.bias"], dt, mutant)
        return (out,), (a,)
    if kernel == "heads":
        return heads_ref(*inputs, *head_weights(sd), dt=dt, mutant=mutant)
    i = int(kernel[5:])
    out, a = block_ref(inputs[0], *block_weights(sd, i), BLOCKS[i][2], dt, mutant)
    return (out,), (a,)


def net_ref(sd, tiles):
    """The whole net in float64: (b1 [T, 16, 16, 88], b2 [T, 8, 8, 96], r [T, 896, 16], c [T, 896])."""
    x = stem_ref(tiles, sd["backbone1.0.weight"], sd["backbone1.0.bias"])[0]
    b1 = None
    for i in range(16):
        x = block_ref(x, *block_weights(sd, i), BLOCKS[i][2])[0]
        if i == 10:
            b1 = x
    (r, c), _ = heads_ref(b1, x, *head_weights(sd))
    return b1, x, r, c


# ------------------------------------------------------------------- operands
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _shapes():
    """name -> shape of every state_dict tensor."""
    s = {"backbone1.0.weight": (24, 3, 5, 5), "backbone1.0.bias": (24,)}
    for p, (cin, cout, _) in zip(PREFIX, BLOCKS):
        s[f"{p}.convs.0.weight"], s[f"{p}.convs.0.bias"] = (cin, 1, 3, 3), (cin,)
        s[f"{p}.convs.1.weight"], s[f"{p}.convs.1.bias"] = (cout, cin, 1, 1), (cout,)
    for n, cout, cin in (("classifier_8", 2, 88), ("classifier_16", 6, 96), ("regressor_8", 32, 88),
                         ("regressor_16", 96, 96)):
        s[f"{n}.weight"], s[f"{n}.bias"] = (cout, cin, 1, 1), (cout,)
    return s


def exact_state_dict(seed=0):
    """Weights in {-1, 0, 1}, integer biases in [-2, 2] (float32)."""
    sd = {}
    for k, shape in _shapes().items():
        lo, hi = (-2, 3) if k.endswith("bias") else (-1, 2)
        sd[k] = _rng("exact", seed, k).integers(lo, hi, shape).astype(np.float32)
    return sd


def random_state_dict(seed=0):
    """Signed Gaussian weights scaled by 1 / sqrt(fan in), Gaussian biases, rounded to float32."""
    sd = {}
    for k, shape in _shapes().items():
        fan = int(np.prod(shape[1:])) if len(shape) > 1 else 1
        sd[k] = (_rng("random", seed, k).standard_normal(shape) / np.sqrt(fan)).astype(np.float32)
    return sd


def input_shapes(kernel):
    if kernel == "stem":
        return [(128, 128, 3)]
    if kernel == "heads":
        return [(16, 16, 88), (8, 8, 96)]
    return [block_shapes(int(kernel[5:]))[0]]


def case_inputs(kind, kernel, T=T_CASE):
    """The inputs of one layer case.  exact: integers in [-3, 3] (stem: pixels in
    {0, 255}, which normalise to exactly -1 and +1); random: signed N(0, 1) in
    float32 (stem: uniform uint8)."""
    out = []
    for j, shape in enumerate(input_shapes(kernel)):
        g = _rng(kind, kernel, j)
        full = (T,) + shape
        if kernel == "stem":
            out.append((g.integers(0, 2, full) * 255 if kind == "exact" else g.integers(0, 256, full)).astype(np.uint8))
        elif kind == "exact":
            out.append(g.integers(-3, 4, full).astype(np.float32))
        else:
            out.append(g.standard_normal(full).astype(np.float32))
    return out


def stem_edge_tiles():
    """An all-0 tile, an all-255 tile, and one whose only non-zero pixels (255) are
    the last two rows and columns: the taps that reach the (1, 2, 1, 2) pad."""
    t = np.zeros((3, 128, 128, 3), np.uint8)
    t[1] = 255
    t[2, 126:] = 255
    t[2, :, 126:] = 255
    return t


def worst_ratio(kernel, got, ref, mags):
    """max |got - ref| / (gamma_n A) over every output of `kernel` (0 / 0 counts as 0:
    an output that no operand reaches must be exact)."""
    worst = 0.0
    for g, r, b in zip(got, ref, bounds(kernel, mags)):
        err = np.abs(np.asarray(g, np.float64) - r)
        assert not np.isnan(err).any()
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0, 0.0, err / b)
        worst = max(worst, float(q.max()))
    return worst


# -------------------------------------------------------------------- tiles
def area_resize_ref(src, out=bz.TILE):
    """bz.area_resize_np with float64 matmuls: every product and partial sum is an
    integer <= 255 n^2 < 2^53, so they are exact and BLAS may order them freely."""
    ny, nx = src.shape[:2]
    assert out <= min(ny, nx) and 255 * ny * nx < 2 ** 53
    ry, rx = bz._overlap(ny, out).astype(np.float64), bz._overlap(nx, out).astype(np.float64)
    den = nx * ny
    res = np.empty((out, out, 3), np.uint8)
    for c in range(3):
        num = (ry @ src[:, :, c].astype(np.float64) @ rx.T).astype(np.int64)
        res[:, :, c] = ((2 * num + den) // (2 * den)).astype(np.uint8)
    return res


def tile_frames_ref(frames):
    """bz.tile_frames_np on area_resize_ref."""
    F, H, W, _ = frames.shape
    split, x_step, n = bz.tile_windows(H, W)
    out = np.empty((F * n, bz.TILE, bz.TILE, 3), np.uint8)
    for f in range(F):
        for h in range(n):
            out[f * n + h] = area_resize_ref(frames[f, :split, h * x_step:h * x_step + split])
    return out


def limit_frame(H, W, seed=0):
    """A frame of 255 (the largest sums) with other values on a sparse grid, so a
    dropped or doubled source pixel moves a rounding somewhere."""
    fr = np.full((1, H, W, 3), 255, np.uint8)
    g = _rng("limit", H, W, seed)
    ys, xs = np.arange(3, H, 11), np.arange(5, W, 13)
    fr[0, ys[:, None], xs[None, :]] = g.integers(0, 255, (len(ys), len(xs), 3), dtype=np.uint8)
    return fr
