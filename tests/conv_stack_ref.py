"""Plain CPU references for the conv-stack layer entry points ``fac_conv3x3`` and
``fac_stem224`` (include/fac_ops.h; csrc/conv.hip, csrc/stem224.hip), and the
operand sets their tests use.  Test infrastructure: never shipped or measured.

* ``conv3x3_ref``   - one 3x3 layer in float64 on operands already rounded to the
  16-bit type: conv, + bias, ReLU if asked, 2x2 max if asked.  Un-rounded.
* ``stem_ref``      - the fused 224^2 block, the three convs with the kernel's
  rounding points, accumulated in float64 (the reference) or in float32 (only to
  measure the accumulation-order envelope, tools/conv_stack_envelope.py).
* ``exact_operands`` / ``stem_exact_operands`` - operands in {-1, 0, 1} whose every
  partial sum is a small integer: exact in bf16, fp16 and fp32 in any summation
  order, so a kernel's output must EQUAL the reference.
* ``stem_random_operands`` - the random stem case, shared by the GPU test and the
  envelope tool (same seeds).

Everything is NHWC on the outside, as the kernels are.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

T16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
MEAN = (0.485, 0.456, 0.406)     # stem224.hip kNormMean
STD = (0.229, 0.224, 0.225)      # stem224.hip kNormStd
EXACT_MAX = 256                  # integers up to here are exact in bf16 (8 significant bits)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def conv3x3_ref(x16, w16, bias, pool, relu):
    """x16 [n][h][h][cin] and w16 [cout][cin][3][3] already rounded to the 16-bit
    type, bias fp32 [cout].  Returns (ref, A), float64 NHWC: ref = conv + bias,
    then ReLU, then max_pool2d(2); A = conv(|x|, |w|) + |bias|, the magnitude the
    fp32 accumulation error is relative to, pooled with the same max."""
    x, w = _nchw(x16.double()), w16.double()
    b = bias.double().view(1, -1, 1, 1)
    ref = F.conv2d(x, w, padding=1) + b
    a = F.conv2d(x.abs(), w.abs(), padding=1) + b.abs()
    if relu:
        ref = F.relu(ref)
    if pool:
        ref, a = F.max_pool2d(ref, 2), F.max_pool2d(a, 2)
    return _nhwc(ref), _nhwc(a)


def normalize_u8_f32(u8):
    """uint8 NHWC crops -> fp32 NCHW, fp32((v/255 - mean_c)/std_c) with IEEE fp32
    operations in the kernel's order (stem224.hip's LUT)."""
    x = _nchw(u8.to(torch.float32))
    mean = torch.tensor(MEAN, dtype=torch.float32).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float32).view(1, 3, 1, 1)
    return ((x / torch.tensor(255.0, dtype=torch.float32) - mean) / std).contiguous()


def stem_ref(inp, w1, b1, w2, b2, w3, b3, dt, u8, acc=torch.float64, mutant=None):
    """fac_stem224 on the CPU.  inp: uint8 NHWC [n][224][224][3] (u8) or fp32 NCHW
    [n][3][224][224]; w*: fp32 [cout][cin][3][3] (rounded to the 16-bit type here,
    as the packing does); b*: fp32.  Rounding points: the input once (u8: of the
    fp32 normalised value; padding is zero in normalised space), conv1 and conv2
    outputs round16(relu(. + b)), conv3 + b3, ReLU, 2x2 max, one rounding.  acc:
    the accumulation type.  Returns NHWC [n][112][112][32] in acc (values of the
    16-bit type).

    mutant (tools/conv_stack_envelope.py only): "drop_tap" leaves out conv2's tap
    (ky, kx) = (1, 2); "pad_relu_b1" gives conv2 relu(b1) instead of 0 for
    conv1 pixels outside the image."""
    td = T16[dt]
    r16 = lambda t: t.to(torch.float32).to(td).to(acc)  # noqa: E731
    x = normalize_u8_f32(inp) if u8 else inp.to(torch.float32)
    x = r16(x)
    ws = [w.to(td).to(acc) for w in (w1, w2, w3)]
    bs = [b.to(acc).view(1, -1, 1, 1) for b in (b1, b2, b3)]
    if mutant == "drop_tap":
        ws[1] = ws[1].clone()
        ws[1][:, :, 1, 2] = 0
    c1 = r16(F.relu(F.conv2d(x, ws[0], padding=1) + bs[0]))
    if mutant == "pad_relu_b1":
        pad = r16(F.relu(bs[0])).expand(c1.shape[0], -1, 226, 226).clone()
        pad[:, :, 1:-1, 1:-1] = c1
        c2 = r16(F.relu(F.conv2d(pad, ws[1]) + bs[1]))
    else:
        c2 = r16(F.relu(F.conv2d(c1, ws[1], padding=1) + bs[1]))
    c3 = F.max_pool2d(F.relu(F.conv2d(c2, ws[2], padding=1) + bs[2]), 2)
    return _nhwc(r16(c3))


def stem_stage_maxima(inp, w1, b1, w2, b2, w3, b3):
    """max over every stage of conv(|x|, |w|) + |b| of the exact-integer chain
    (float64; x: fp32 NCHW): what has to stay <= EXACT_MAX."""
    x = inp.double().abs()
    out = []
    for w, b in ((w1, b1), (w2, b2), (w3, b3)):
        a = F.conv2d(x, w.double().abs(), padding=1) + b.double().abs().view(1, -1, 1, 1)
        out.append(float(a.max()))
        x = a
    return out


# ------------------------------------------------------------------ operands
def random_operands(h, cin, cout, n, dt, seed):
    """x ~ N(0,1) signed, w ~ N(0,1)/sqrt(9 cin), bias ~ 0.2 N(0,1); x and w
    rounded to the 16-bit type (w returned as fp32 holding those values)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, h, cin, generator=g).to(T16[dt])
    w = (torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).to(T16[dt]).float()
    bias = 0.2 * torch.randn(cout, generator=g)
    return x, w, bias


def sparse_pm1(cout, cin, per_out, g, group=32):
    """[cout][cin][3][3] weights in {-1, 0, 1}: inside every group of `group`
    consecutive output channels each (tap, input channel) pair is non-zero for
    one channel chosen at random (so every column block of a kernel, a multiple
    of 32 channels, uses every tap of every input channel, each with its own
    channel), plus `per_out` more non-zeros per output channel."""
    pairs = 9 * cin
    w = torch.zeros(cout, pairs)
    sign = lambda shape: (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()  # noqa: E731
    for o0 in range(0, cout, group):
        gs = min(group, cout - o0)
        ch = torch.randint(0, gs, (pairs,), generator=g) + o0
        w[ch, torch.arange(pairs)] = sign((pairs,))
    if per_out:
        cols = torch.randint(0, pairs, (cout, per_out), generator=g)
        w.scatter_(1, cols, sign((cout, per_out)))
    return w.view(cout, cin, 9).reshape(cout, cin, 3, 3).contiguous()


def edge_mask(h):
    """[1][h][h][1]: True on each crop's last row and last column."""
    keep = torch.zeros(1, h, h, 1, dtype=torch.bool)
    keep[:, h - 1, :, :] = True
    keep[:, :, h - 1, :] = True
    return keep


def exact_operands(h, cin, cout, n, dt, seed, edge=False):
    """Inputs in {-1, 0, 1} (edge: non-zero only in each crop's last row and
    last column), weights sparse_pm1, integer biases in -4..4."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randint(0, 3, (n, h, h, cin), generator=g) - 1).float()
    if edge:
        x = torch.where(edge_mask(h), x, torch.zeros_like(x))
    w = sparse_pm1(cout, cin, 8, g)
    bias = (torch.randint(0, 9, (cout,), generator=g) - 4).float()
    return x.to(T16[dt]), w, bias


def stem_exact_operands(n, seed):
    """The exact-integer stem chain: fp32 NCHW input in {0, 1}; conv1 sparse +-1
    with at most 3 non-zeros per output channel, conv2 / conv3 at most 4, every
    tap and every input channel of each conv used by some output channel; integer
    biases, 1..3 on conv1 and conv2 (a conv1 / conv2 pixel outside the image that
    is not stored as 0 leaks relu(b) > 0 into the border), -2..2 on conv3."""
    g = torch.Generator().manual_seed(seed)
    inp = torch.randint(0, 2, (n, 3, 224, 224), generator=g).float()
    sign = lambda k: (torch.randint(0, 2, (k,), generator=g) * 2 - 1).float()  # noqa: E731

    def conv(cin, nnz):
        # the j-th non-zero of output channel o: input channel from a random
        # permutation (cycled when cin < 32), tap from a random order of the nine
        # walked by o * nnz + j, so all taps and all input channels are used
        w = torch.zeros(32, cin, 9)
        tap_order = torch.randperm(9, generator=g)
        for j in range(nnz):
            chan = torch.randperm(32, generator=g) % cin
            tap = tap_order[(torch.arange(32) * nnz + j) % 9]
            w[torch.arange(32), chan, tap] = sign(32)
        return w.reshape(32, cin, 3, 3).contiguous()

    w1, w2, w3 = conv(3, 3), conv(32, 4), conv(32, 4)
    b1 = torch.randint(1, 4, (32,), generator=g).float()
    b2 = torch.randint(1, 4, (32,), generator=g).float()
    b3 = (torch.randint(0, 5, (32,), generator=g) - 2).float()
    return inp, w1, b1, w2, b2, w3, b3


def taps_and_channels_used(w):
    """(every one of the 9 taps, every input channel) is non-zero for some output channel."""
    nz = w != 0
    return bool(nz.any(dim=(0, 1)).all()), bool(nz.any(dim=(0, 2, 3)).all())


STEM_RANDOM_N = 3
STEM_RANDOM_SEED = 4242


def stem_random_operands(dt, u8):
    """The random stem case (n = 3): uint8 crops or N(0,1) fp32 NCHW; He-scaled
    weights; biases 0.5 + 0.25 N(0,1) on conv1 / conv2 (large and mostly positive:
    a border that is not zeroed must show) and 0.2 N(0,1) on conv3."""
    g = torch.Generator().manual_seed(STEM_RANDOM_SEED + (dt == "bf16") + 2 * bool(u8))
    n = STEM_RANDOM_N
    if u8:
        inp = torch.randint(0, 256, (n, 224, 224, 3), generator=g).to(torch.uint8)
    else:
        inp = torch.randn(n, 3, 224, 224, generator=g)
    w1 = torch.randn(32, 3, 3, 3, generator=g) / 27 ** 0.5
    w2 = torch.randn(32, 32, 3, 3, generator=g) / 288 ** 0.5
    w3 = torch.randn(32, 32, 3, 3, generator=g) / 288 ** 0.5
    b1 = 0.5 + 0.25 * torch.randn(32, generator=g)
    b2 = 0.5 + 0.25 * torch.randn(32, generator=g)
    b3 = 0.2 * torch.randn(32, generator=g)
    return inp, w1, b1, w2, b2, w3, b3


ULP_REL = {"fp16": 2.0 ** -10, "bf16": 2.0 ** -7}


def ulp_diff_and_flips(got, ref, dt):
    """(max |got - ref| in 16-bit ulps of max(|ref|, rms(ref)/2) - the unit of
    tests/test_gpu_parity.py::_ulp_diff - and the fraction of unequal outputs)."""
    got, ref = got.double(), ref.double()
    floor = 0.5 * float(ref.pow(2).mean().sqrt())
    worst = float(((got - ref).abs() / (ref.abs().clamp_min(floor) * ULP_REL[dt])).max())
    return worst, float((got != ref).double().mean())
