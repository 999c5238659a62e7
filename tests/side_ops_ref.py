"""fp64 restatements of the side kernels of csrc/ops.hip for the tests: GGCA
(fac_ggca), KANLinear (fac_kan_linear), pooling (fac_pool_nd), the two input
packers (fac_pack_input, fac_pack_input_s2d) and fac_sigmoid; a helper, not
collected as a test.  torch only: nothing here loads the library.

* ``ggca_ref`` / ``kan_ref`` run the oracles' own functions
  (oracle.repbn8_torch.ggca, oracle.resvitkan_torch.kan_linear_fp32) on
  operands of a chosen float type: fp64 is the truth the kernels are measured
  against, fp32 shows how far the reference's own arithmetic sits from it.
* ``round16`` rounds an fp64 tensor ONCE to a 16-bit type (torch's own
  double -> half conversion goes through fp32 and rounds twice) and
  ``ulp_dist`` counts the 16-bit values between two tensors, so "<= 1 ulp" is
  an integer statement without a noise allowance.
* the case lists and input makers are shared by the CPU tests
  (test_side_ops_ref.py: the gates hold for the reference's fp32 arithmetic
  alone) and the GPU tests (test_gpu_side_ops.py).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from oracle import repbn8_torch, resvitkan_torch

T16 = {"bf16": torch.bfloat16, "fp16": torch.float16}
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ---------------------------------------------------------------- 16-bit rounding and distance
def round16(x: torch.Tensor, dt: str) -> torch.Tensor:
    """x (fp64 or fp32) rounded once, to nearest even, to the 16-bit type.
    fp64 goes to fp32 by round-to-odd first (truncate, then set the last bit
    if anything was lost): the second rounding then sees on which side of a
    16-bit midpoint the fp64 value lay."""
    if x.dtype != torch.float64:
        return x.float().to(T16[dt])
    f = x.float()
    d = f.double()
    inexact = d != x
    over = inexact & (d.abs() > x.abs())
    bits = f.view(torch.int32) - over.to(torch.int32)       # one step towards zero (sign-magnitude patterns)
    bits = bits | inexact.to(torch.int32)
    return bits.view(torch.float32).to(T16[dt])


def _key(t16: torch.Tensor) -> torch.Tensor:
    b = t16.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)             # monotonic in the float order, +0 and -0 both 0


def ulp_dist(a16: torch.Tensor, b16: torch.Tensor) -> torch.Tensor:
    """How many 16-bit values lie between a and b (0: equal; same 16-bit type, no NaN)."""
    assert a16.dtype == b16.dtype and a16.dtype in (torch.float16, torch.bfloat16)
    return (_key(a16) - _key(b16)).abs()


def ulps_noise(a: torch.Tensor, b: torch.Tensor, dt: str) -> torch.Tensor:
    """test_gpu_ops._ulps: |a - b| in 16-bit ulps at max(|a|, |b|) after an fp32
    accumulation-noise allowance of 2^-16 of the output scale (sums that
    cancel carry fp32 rounding larger than the ulp of their own size)."""
    a, b = a.float(), b.float()
    m = torch.maximum(a.abs(), b.abs()).clamp_min(1e-30)
    ulp = torch.pow(2.0, torch.floor(torch.log2(m)) - (7 if dt == "bf16" else 10))
    if dt == "fp16":
        ulp = ulp.clamp_min(2.0 ** -24)
    noise = 2.0 ** -16 * torch.maximum(a.abs().max(), b.abs().max())
    return ((a - b).abs() - noise).clamp_min(0) / ulp


# ---------------------------------------------------------------- GGCA
# (n, h, w, c, groups)
GGCA_CASES = [
    (2, 5, 7, 64, 2),      # non-square, cr = 2
    (2, 16, 3, 96, 2),     # tall, cg = 48
    (1, 16, 16, 64, 1),    # h*w*cg = 16384 and 2h + 2w = 64, both at their limits
    (2, 1, 15, 256, 1),    # cg at its maximum, (2h + 2w)*cg = 8192 at its limit, h = 1
    (3, 7, 7, 512, 4),     # the model's shape
    (2, 3, 3, 32, 2),      # cg = 16, cr = 1
]
GGCA_FLIP_CAP_REF = 1e-3   # share of outputs where fp32 torch and fp64 round differently
GGCA_FLIP_CAP_GPU = 5e-3   # the kernel adds its own expf and summation order


def ggca_inputs(case, dt: str, seed: int = 0):
    """(x16 [n][h][w][c], (w1 [cr][cg], b1 [cr], bn4 [4][cr], w2 [cg][cr], b2 [cg])) as fac_ggca takes them:
    x = 2 randn with one image all negative (n == 1: the lower half of the channels), so a pooled maximum
    below zero exists; weights / sqrt(fan_in); BN weight of both signs, running_var in [0.5, 1.5], non-zero
    means and biases."""
    n, h, w, c, groups = case
    cg = c // groups
    cr = cg // 16
    g = torch.Generator().manual_seed(1000 * seed + n * 131 + h * 17 + w * 7 + c)
    x = 2 * torch.randn(n, h, w, c, generator=g)
    if n > 1:
        x[-1] = -x[-1].abs() - 2.0 ** -6
    else:
        x[..., :c // 2] = -x[..., :c // 2].abs() - 2.0 ** -6
    w1 = torch.randn(cr, cg, generator=g) / math.sqrt(cg)
    b1 = 0.5 * torch.randn(cr, generator=g)
    mean = 0.5 * torch.randn(cr, generator=g)
    var = 0.5 + torch.rand(cr, generator=g)
    gamma = torch.randn(cr, generator=g)
    gamma = torch.where(gamma.abs() < 0.1, torch.full_like(gamma, 0.3), gamma)
    if cr > 1:
        gamma[0], gamma[1] = gamma[0].abs(), -gamma[1].abs()
    beta = 0.5 * torch.randn(cr, generator=g)
    w2 = torch.randn(cg, cr, generator=g) / math.sqrt(cr)
    b2 = 0.5 * torch.randn(cg, generator=g)
    return x.to(T16[dt]), (w1, b1, torch.stack([mean, var, gamma, beta]).contiguous(), w2, b2)


def ggca_ref(x16_nchw: torch.Tensor, w1, b1, bn4, w2, b2, groups: int, dtype=torch.float64) -> torch.Tensor:
    """x * ((x * att_h) * att_w) [n][c][h][w] in `dtype`: oracle.repbn8_torch.ggca (GGCA.forward,
    cvit_GGCA_ADD_DEConv_RepBn8.py:172-207) on the eight shared_conv tensors, then the caller's x * GGCA(x)."""
    cr, cg = w1.shape
    q = "ggca.shared_conv."
    sd = {q + "0.weight": w1.reshape(cr, cg, 1, 1), q + "0.bias": b1,
          q + "1.running_mean": bn4[0], q + "1.running_var": bn4[1], q + "1.weight": bn4[2], q + "1.bias": bn4[3],
          q + "3.weight": w2.reshape(cg, cr, 1, 1), q + "3.bias": b2}
    sd = {k: v.to(dtype).contiguous() for k, v in sd.items()}
    x = x16_nchw.to(dtype)
    return x * repbn8_torch.ggca(sd, x, groups)


# ---------------------------------------------------------------- KANLinear
KAN_CASES = [(1, 1, 1), (33, 40, 70), (64, 64, 128), (5, 500, 3)]   # (rows, in_f, out_f)
KAN_NK = 12
U32 = 2.0 ** -24


def kan_inputs(case, seed: int = 0):
    """(x [rows][in], grid [in][12], base_w [out][in], spline_w [out][in][8], spline_scaler [out][in]) fp32.
    Knots: step 0.4 from -2.2, every knot of every feature moved by 0.05 randn (at most 0.15, so they stay
    ordered).  x = 1.5 randn, then planted: features 0, 1 and the last one take each of their own 12 knots
    (rows 0..11; with fewer rows the knots are spread over the first 24 features instead), values below the
    first and above the last knot, +0, -0, 1e4 and -1e4, and one row that is -1e4 throughout (SiLU and every
    basis are zero there)."""
    rows, in_f, out_f = case
    g = torch.Generator().manual_seed(7000 + 100 * seed + rows + in_f + out_f)
    base = -2.2 + 0.4 * torch.arange(KAN_NK, dtype=torch.float64)
    grid = (base + (0.05 * torch.randn(in_f, KAN_NK, generator=g, dtype=torch.float64)).clamp(-0.15, 0.15)).float()
    x = 1.5 * torch.randn(rows, in_f, generator=g)
    if rows >= KAN_NK:
        for i in sorted({0, min(1, in_f - 1), in_f - 1}):
            x[:KAN_NK, i] = grid[i]
    else:
        for i in range(min(in_f, 24)):
            for r in range(rows):
                x[r, i] = grid[i, (r + rows * i) % KAN_NK]
    if in_f >= 12:
        r = rows - 1
        x[r, 2], x[r, 3] = grid[2, 0] - 0.5, grid[3, 0] - 3.0            # below the first knot
        x[r, 4], x[r, 5] = grid[4, -1] + 2.0 ** -20, grid[5, -1] + 4.0   # above the last
        x[r, 6], x[r, 7] = 0.0, -0.0
        x[r, 8], x[r, 9] = 1e4, -1e4
    if rows >= 3:
        x[rows - 2] = -1e4
    bw = torch.randn(out_f, in_f, generator=g) / math.sqrt(in_f)
    sw = torch.randn(out_f, in_f, KAN_NK - 4, generator=g) / math.sqrt(in_f)
    ss = 1.0 + 0.5 * torch.randn(out_f, in_f, generator=g)
    return x, grid, bw, sw, ss


def kan_ref(x, grid, base_w, spline_w, spline_scaler, dtype=torch.float64):
    """(y [rows][out], A [rows][out]) in `dtype`: y = oracle.resvitkan_torch.kan_linear_fp32 (KANLinear.forward,
    kan.py:189-206) on operands cast to `dtype`; A = sum_i |silu(x)| |bw| + sum_{i,k} |B_k(x)| |sw ss|, the sum
    of the absolute values of y's 9 in_f products."""
    p = "k"
    sd = {p + ".grid": grid.to(dtype), p + ".base_weight": base_w.to(dtype), p + ".spline_weight": spline_w.to(dtype),
          p + ".spline_scaler": spline_scaler.to(dtype)}
    xd = x.to(dtype)
    y = resvitkan_torch.kan_linear_fp32(sd, p, xd)
    scaled = (sd[p + ".spline_weight"] * sd[p + ".spline_scaler"].unsqueeze(-1)).abs()
    bases = resvitkan_torch.b_splines(xd, sd[p + ".grid"]).abs()
    a = F.silu(xd).abs() @ sd[p + ".base_weight"].abs().t() + bases.reshape(xd.shape[0], -1) @ scaled.reshape(
        scaled.shape[0], -1).t()
    return y, a


def kan_bound(a: torch.Tensor, in_f: int) -> torch.Tensor:
    """|y - y64| <= (9 in_f + 32) 2^-24 A: 9 in_f u bounds the fp32 recursive sum of the 9 in_f products;
    32 u covers each feature's own roundings (<= ~20 operations of SiLU and the three Cox-de Boor levels,
    every term non-negative, so nothing amplifies them)."""
    return (9 * in_f + 32) * U32 * a.double()


# ---------------------------------------------------------------- pooling
def pool_ref(x16: torch.Tensor, kernel, stride, padding, mode: str) -> torch.Tensor:
    """x16 [n][d][h][w][c] -> fp64 [n][od][oh][ow][c]: MaxPool3d (padding ignored, i.e. -inf) or
    AvgPool3d(count_include_pad=True), floor mode."""
    x = x16.double().permute(0, 4, 1, 2, 3)
    if mode == "max":
        y = F.max_pool3d(x, kernel, stride, padding)
    else:
        y = F.avg_pool3d(x, kernel, stride, padding, count_include_pad=True)
    return y.permute(0, 2, 3, 4, 1).contiguous()


# ---------------------------------------------------------------- input packers
def _normalise(x: torch.Tensor, div: float, mean, std) -> torch.Tensor:
    """(x / div - mean[c]) / std[c] in fp32 on a channels-LAST fp32 tensor [..., 3]."""
    m = torch.tensor(mean if mean is not None else (0.0, 0.0, 0.0), dtype=torch.float32)
    s = torch.tensor(std if std is not None else (1.0, 1.0, 1.0), dtype=torch.float32)
    return (x / torch.tensor(div, dtype=torch.float32) - m) / s


def pack_input_ref(src: torch.Tensor, u8: bool, div: float, mean, std, c_pad: int, dt: str) -> torch.Tensor:
    """fac_pack_input: u8 [n, *spatial, 3] or fp32 planar [n, 3, *spatial] -> 16-bit [n][s][c_pad], channels
    0..2 the fp32 arithmetic rounded once, the rest zero."""
    n = src.shape[0]
    x = src.reshape(n, -1, 3).float() if u8 else src.reshape(n, 3, -1).permute(0, 2, 1).float()
    out = torch.zeros(n, x.shape[1], c_pad, dtype=T16[dt])
    out[..., :3] = _normalise(x, div, mean, std).to(T16[dt])
    return out


def pack_s2d_ref(src: torch.Tensor, pb: int, pa: int, div: float, mean, std, dt: str) -> torch.Tensor:
    """fac_pack_input_s2d on an fp32 image batch [n][3][h][w] or clip batch [n][3][frames][h][w] ->
    16-bit [n][frames][h/2+pb+pa][w/2+pb+pa][16]: cell (Y, X) channel 4(2dy + dx) + c = the normalised pixel
    (2(Y - pb) + dy, 2(X - pb) + dx) of channel c; channel 3 of each pixel and the border cells zero."""
    if src.dim() == 4:
        src = src.unsqueeze(2)
    n, _, fr, h, w = src.shape
    x = _normalise(src.permute(0, 2, 3, 4, 1).float(), div, mean, std).to(T16[dt])   # [n][fr][h][w][3]
    out = torch.zeros(n, fr, h // 2 + pb + pa, w // 2 + pb + pa, 16, dtype=T16[dt])
    for b in range(n):
        for f in range(fr):
            for dy in range(2):
                for dx in range(2):
                    q = 4 * (2 * dy + dx)
                    out[b, f, pb:pb + h // 2, pb:pb + w // 2, q:q + 3] = x[b, f, dy::2, dx::2]
    return out


# ---------------------------------------------------------------- sigmoid
def sigmoid_inputs(n: int) -> torch.Tensor:
    """0, +inf, -inf, then a linspace over [-104, 104] (expf overflows beyond 88.7), n values in all."""
    lin = torch.linspace(-104.0, 104.0, max(n - 3, 1))
    return torch.cat([torch.tensor([0.0, math.inf, -math.inf]), lin])[:n].contiguous()


def sigmoid_ref(x: torch.Tensor) -> torch.Tensor:
    return torch.sigmoid(x.double())


def sigmoid_bound(ref: torch.Tensor) -> torch.Tensor:
    """expf, one add and one divide: <= 3 fp32 ulp, gated at 4 u relative; the floor 2^-125 admits a result
    flushed to zero below the normal range."""
    return 4 * U32 * ref + 2.0 ** -125
