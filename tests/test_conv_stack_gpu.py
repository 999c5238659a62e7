"""fac_conv3x3 and fac_stem224 (include/fac_ops.h; csrc/conv.hip, stem224.hip)
through the C ABI, one launch at a time, against the float64 references of
tests/conv_stack_ref.py.

Every row of CASES runs three operand sets in both dtypes:

* random       x ~ N(0,1) signed, He-scaled weights: |out - ref| within one 16-bit
               ulp of |ref| plus the fp32 accumulation bound 9 cin 2^-24 A,
               A = conv(|x|, |w|) + |bias| (the rule of test_reskan_gpu._case).
* exact        operands in {-1, 0, 1}, integer biases, every partial sum an integer
               of magnitude <= 256 (asserted on the reference): exact in bf16, fp16
               and fp32 in any summation order, so the output must EQUAL the
               reference (compared as values; the 16-bit encodings of those are
               unique but for the sign of zero).  A wrong tap, channel piece, pixel,
               padding source or column block has no tolerance to hide in.
* exact, edge  the same with input only in each crop's last row and last column:
               a halo that reads the next row or the next crop instead of the
               zero page shows exactly.

Which launch_conv_t case (conv.hip) each id reaches; [8] marks gridDim.x % 8 == 0,
the XCD box permutation.  Ids are test_conv3x3_{random,exact,edge}[<dt>-<id>].
"thr" is the largest n on the few-crop side of n (cout/bn) {14: 1, 28: 7} <= 2 CUs,
computed from the device's CU count.

  224032 launch_box 16x16/32, HB 2             224-32-32-p0r1-n2 [8], 224-64-32-p1r0-n1,
                                                224-96-32-p1r1-n1, 224-32-32-p0r0-n1
  112064 pooled, 2 per CU                      112-32-64-p1r0-n8 [8], 112-96-128-p1r1-n3
  112064 unpooled, 4 per CU                    112-32-64-p0r1-n8 [8], 112-96-64-p0r0-n3,
                                                112-64-128-p0r1-n3
  56128  launch_box 8x28/128                   56-32-128-p0r1-n4 [8], 56-96-128-p1r0-n3,
                                                56-64-256-p0r0-n3, 56-64-256-p1r1-n4 [8]
  56064  launch_box 8x28/64                    56-32-64-p0r0-n4 [8], 56-96-64-p1r1-n3,
                                                56-64-192-p0r1-n3, 56-32-192-p1r0-n4 [8]
  28256  launch_db 4x28/256                    28-32-256-p0r1-n8 [8], 28-96-256-p1r0-n5,
                                                28-64-256-p0r0-n5, 28-64-256-p1r1-n8 [8]
  28192  launch_db 4x28/192                    28-64-192-p0r0-n5, 28-32-192-p1r1-n8 [8],
                                                28-96-192-p0r1-n5, 28-96-192-p1r0-n5
  28128  launch_db BR 9 (few crops)            28-96-128-p0r0-n8 [8], 28-64-128-p1r1-n5,
                                                28-32-1280-p0r1-nthr, 28-32-1280-p1r0-nthr
  28128  launch_db 3-slice (above)             28-32-1280-p{0,1}r{0,1}-nthr+1 (four rows;
                                                [8] at 256 CUs, where thr + 1 = 8)
  14128  launch_box 14x14/128                  14-32-128-p0r0-n8 [8], 14-96-128-p1r1-n3,
                                                14-64-384-p0r1-n3, 14-32-384-p1r0-n8 [8]
  14192  launch_box 14x14/192, no pool         14-64-192-p0r1-n8 [8], 14-96-192-p0r0-n3,
                                                14-32-192-p0r1-n3
  14064  PB, WR 9 (few crops; ring9 & 2)       14-96-64-p0r1-n3, 14-64-64-p1r0-n8 [8],
                                                14-32-320-p0r0-nthr, 14-32-320-p1r1-nthr
  14064  plain 3-slice (above)                 14-32-320-p1r1-nthr+1, 14-32-320-p0r0-nthr|8 [8],
                                                14-32-320-p0r1-nthr+1, 14-32-320-p1r0-nthr|8 [8]
  14064  ring9 & 1 arm                         not reachable: the process-wide option is 6
  14032                                        reachable only through a model context's
                                               conv_small14 option; it stays with its
                                               bit-identity test in test_gpu_parity.py
  stem224_fused, one box per workgroup         test_stem_exact_integer_chain[<dt>-one_box]   (n = 1)
  stem224_fused, three boxes per workgroup     test_stem_exact_integer_chain[<dt>-three_boxes]
                                               (the smallest n with 98 n >= 3 CUs)
  stem224_fused, two boxes (n = 3), both       test_stem_random_vs_fp64[<dt>-u8|f32],
    input paths                                test_stem_u8_equals_f32_path, test_stem_batch_independence

The stem's random-operand gate is the one measured number here:
tests/golden/conv_stack_envelope.json, made on the CPU by
tools/conv_stack_envelope.py from the float32-accumulated reference against the
float64 one, on these operands; the kernel is allowed 2x each figure.
"""
import functools
import json
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import conv_stack_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T16 = R.T16
MANT = {"fp16": 10, "bf16": 7}
MIN_EXP = {"fp16": -14, "bf16": -126}
OK, ARG, SHAPE = 0, -1, -2
GUARD = 4096                                    # sentinel elements behind every output
NAN16 = {"fp16": 0x7E00, "bf16": 0x7FC0}        # outputs start as NaN: an unwritten one is not finite
SENTINEL = 0x5A5A


def _ulp(ref, dt):
    """One 16-bit unit in the last place of |ref| (float64); test_reskan_gpu._ulp."""
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** MIN_EXP[dt]))).clamp_min(MIN_EXP[dt])
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - MANT[dt])


# (h, cin, cout, pool, relu, n); n: an int, or relative to the few-crop threshold
CASES = [
    (224, 32, 32, 0, 1, 2), (224, 64, 32, 1, 0, 1), (224, 96, 32, 1, 1, 1), (224, 32, 32, 0, 0, 1),
    (112, 32, 64, 0, 1, 8), (112, 32, 64, 1, 0, 8), (112, 96, 64, 0, 0, 3), (112, 96, 128, 1, 1, 3),
    (112, 64, 128, 0, 1, 3),
    (56, 32, 128, 0, 1, 4), (56, 96, 128, 1, 0, 3), (56, 64, 256, 0, 0, 3), (56, 64, 256, 1, 1, 4),
    (56, 32, 64, 0, 0, 4), (56, 96, 64, 1, 1, 3), (56, 64, 192, 0, 1, 3), (56, 32, 192, 1, 0, 4),
    (28, 32, 256, 0, 1, 8), (28, 96, 256, 1, 0, 5), (28, 64, 256, 0, 0, 5), (28, 64, 256, 1, 1, 8),
    (28, 64, 192, 0, 0, 5), (28, 32, 192, 1, 1, 8), (28, 96, 192, 0, 1, 5), (28, 96, 192, 1, 0, 5),
    (28, 96, 128, 0, 0, 8), (28, 64, 128, 1, 1, 5),
    (28, 32, 1280, 0, 1, "thr"), (28, 32, 1280, 1, 0, "thr"), (28, 32, 1280, 0, 1, "thr+1"), (28, 32, 1280, 1, 0, "thr+1"),
    (28, 32, 1280, 0, 0, "thr+1"), (28, 32, 1280, 1, 1, "thr+1"),
    (14, 32, 128, 0, 0, 8), (14, 96, 128, 1, 1, 3), (14, 64, 384, 0, 1, 3), (14, 32, 384, 1, 0, 8),
    (14, 64, 192, 0, 1, 8), (14, 96, 192, 0, 0, 3), (14, 32, 192, 0, 1, 3),
    (14, 96, 64, 0, 1, 3), (14, 64, 64, 1, 0, 8),
    (14, 32, 320, 0, 0, "thr"), (14, 32, 320, 1, 1, "thr"), (14, 32, 320, 1, 1, "thr+1"), (14, 32, 320, 0, 0, "thr|8"),
    (14, 32, 320, 0, 1, "thr+1"), (14, 32, 320, 1, 0, "thr|8"),
]
BLOCK = {(28, 1280): 128, (14, 320): 64}         # the block of the rows that branch on the threshold


def _id(c):
    return f"{c[0]}-{c[1]}-{c[2]}-p{c[3]}r{c[4]}-n{c[5]}"


def _n(case):
    """The row's crop count; for the threshold rows from the device's CU count:
    few crops <=> n (cout/bn) {14: 1, 28: 7} <= 2 CUs (launch_conv_t)."""
    h, _, cout, _, _, n = case
    if isinstance(n, int):
        return n
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_crop = (cout // BLOCK[(h, cout)]) * {14: 1, 28: 7}[h]
    thr = 2 * cus // per_crop
    assert thr >= 1 and (thr + 1) * per_crop > 2 * cus >= thr * per_crop
    return {"thr": thr, "thr+1": thr + 1, "thr|8": (thr // 8 + 1) * 8}[n]


def test_threshold_rows_straddle_the_threshold():
    """The rows named after the few-crop threshold land on both of its sides on
    this device, and the table has both box orders at every resolution."""
    boxes = {224: 196, 112: 49, 56: 14, 28: 7, 14: 1}
    orders = {h: set() for h in boxes}
    for c in CASES:
        orders[c[0]].add((_n(c) * boxes[c[0]]) % 8 == 0)
    assert all(v == {True, False} for v in orders.values()), orders
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for c in CASES:
        if isinstance(c[5], str):
            per_crop = (c[2] // BLOCK[(c[0], c[2])]) * {14: 1, 28: 7}[c[0]]
            assert (_n(c) * per_crop <= 2 * cus) == (c[5] == "thr"), c


@functools.lru_cache(maxsize=4)
def _case(case, n, dt, kind):
    """Operands, float64 reference and A of one row (a few are kept: the largest
    reference and its A are 50 MB each)."""
    h, cin, cout, pool, relu, _ = case
    seed = h * 100003 + cin * 1009 + cout * 17 + pool * 5 + relu * 3 + n + (dt == "bf16") * 7919
    if kind == "random":
        x, w, bias = R.random_operands(h, cin, cout, n, dt, seed)
    else:
        x, w, bias = R.exact_operands(h, cin, cout, n, dt, seed, edge=(kind == "edge"))
    ref, a = R.conv3x3_ref(x, w.to(T16[dt]), bias, pool, relu)
    return x, w, bias, ref, a


def _lib():
    from fac_fake_amd import _lib as L
    return L, L.load()


def _pack(dt, h, w):
    L, lib = _lib()
    co, ci = w.shape[:2]
    ne = lib.fac_conv3x3_packed_elems(h, ci, co)
    assert ne == co * ci * 9
    pk = torch.empty(ne, dtype=torch.int16)
    wf = w.float().contiguous()
    L.check(lib.fac_conv3x3_pack(L.DTYPES[dt], h, ci, co, wf.data_ptr(), pk.data_ptr()), None, "fac_conv3x3_pack")
    return pk.to(DEV)


def _out_buffer(numel, dt):
    buf = torch.full((numel + GUARD,), NAN16[dt], dtype=torch.int16, device=DEV)
    buf[numel:] = SENTINEL
    return buf


def _take(buf, shape, dt):
    """The output as float64 on the CPU; nothing was written behind it."""
    numel = buf.numel() - GUARD
    assert bool((buf[numel:] == SENTINEL).all()), "the kernel wrote past its output"
    return buf[:numel].view(T16[dt]).view(shape).double().cpu()


def _run_conv(dt, x16, w, bias, h, pool, relu):
    """fac_conv3x3 on input, weights and output of exactly their sizes."""
    from fac_fake_amd.ops import _zero256
    L, lib = _lib()
    n, cin, cout = x16.shape[0], x16.shape[3], w.shape[0]
    xd, bd, pk = x16.contiguous().to(DEV), bias.float().to(DEV), _pack(dt, h, w)
    ho = h // 2 if pool else h
    buf = _out_buffer(n * ho * ho * cout, dt)
    L.check(lib.fac_conv3x3(L.DTYPES[dt], xd.data_ptr(), pk.data_ptr(), bd.data_ptr(), buf.data_ptr(), n, h, cin,
                            cout, pool, relu, _zero256(xd.device).data_ptr(),
                            torch.cuda.current_stream().cuda_stream), None, "fac_conv3x3")
    torch.cuda.synchronize()
    return _take(buf, (n, ho, ho, cout), dt)


@pytest.mark.parametrize("case", CASES, ids=_id)
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_conv3x3_random(case, dt):
    h, cin, cout, pool, relu, _ = case
    x, w, bias, ref, a = _case(case, _n(case), dt, "random")
    out = _run_conv(dt, x, w, bias, h, pool, relu)
    assert torch.isfinite(out).all()
    tol = _ulp(ref, dt) + 9 * cin * 2.0 ** -24 * a
    err = (out - ref).abs()
    worst = float((err / tol).max())
    print(f"conv3x3 random {_id(case)} {dt}: max err {float(err.max()):.3e}, max err / tol {worst:.3f}")
    assert worst <= 1.0, worst
    if not relu:
        assert float(ref.min()) < -0.5 and float(out.min()) < -0.5      # the case has negative outputs to keep


def _check_exact(case, dt, kind):
    h, cin, cout, pool, relu, _ = case
    x, w, bias, ref, a = _case(case, _n(case), dt, kind)
    assert float(a.max()) <= R.EXACT_MAX                          # every partial sum is an exact integer
    assert torch.equal(ref, ref.round()) and ref.abs().max() > 0
    if kind == "exact":     # every (tap, input channel) is used inside every 32 output channels
        assert bool((w.view(cout // 32, 32, cin * 9) != 0).any(1).all())
    out = _run_conv(dt, x, w, bias, h, pool, relu)
    assert torch.isfinite(out).all()
    bad = out != ref
    assert not bool(bad.any()), (f"{int(bad.sum())} of {bad.numel()} outputs differ, first at "
                                 f"(crop, y, x, channel) {tuple(int(i) for i in bad.nonzero()[0])}: "
                                 f"{float(out[bad][0])} for {float(ref[bad][0])}")


@pytest.mark.parametrize("case", CASES, ids=_id)
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_conv3x3_exact(case, dt):
    _check_exact(case, dt, "exact")


@pytest.mark.parametrize("case", CASES, ids=_id)
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_conv3x3_edge(case, dt):
    _check_exact(case, dt, "edge")


@pytest.mark.parametrize("case", [(224, 32, 32, 0, 1, 2), (112, 32, 64, 1, 0, 8), (56, 32, 128, 0, 1, 4),
                                  (28, 32, 256, 0, 1, 8), (14, 32, 128, 0, 0, 8), (14, 32, 320, 1, 0, "thr|8")],
                         ids=_id)
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_conv3x3_batch_independence(case, dt):
    """A crop alone (n = 1: the plain box order) and as the last crop of the
    larger batch (the permuted order) gives the same bits.  The 14/64 row also
    crosses the few-crop threshold: both weight-ring variants give the same bits."""
    h, cin, cout, pool, relu, _ = case
    x, w, bias = R.random_operands(h, cin, cout, _n(case), dt, 31 * h + cout)
    full = _run_conv(dt, x, w, bias, h, pool, relu)
    alone = _run_conv(dt, x[-1:], w, bias, h, pool, relu)
    assert torch.isfinite(full).all()
    assert torch.equal(full[-1:], alone)


def test_conv3x3_argument_and_shape_returns():
    from fac_fake_amd.ops import _zero256
    _, lib = _lib()
    t = torch.zeros(2 * 14 * 14 * 384, dtype=torch.float16, device=DEV)
    o = torch.empty_like(t)
    wpk = torch.zeros(9 * 384 * 384, dtype=torch.float16, device=DEV)
    b = torch.zeros(384, device=DEV)
    z = _zero256(t.device)
    p = lambda v: v.data_ptr()  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    #        dtype in    wpk     bias  out   n  h   cin cout pool relu zero  stream
    good = [1, p(t), p(wpk), p(b), p(o), 2, 14, 64, 128, 0, 1, p(z), st]
    assert lib.fac_conv3x3(*good) == OK
    for i in (1, 2, 3, 4, 11):
        bad = list(good)
        bad[i] = None
        assert lib.fac_conv3x3(*bad) == ARG, i
    for i, v in ((0, 2), (0, -1), (5, 0), (5, -3)):
        bad = list(good)
        bad[i] = v
        assert lib.fac_conv3x3(*bad) == ARG, (i, v)
    shapes = [(7, 64, 128), (14, 48, 128), (112, 64, 96), (56, 64, 32), (14, 0, 128), (14, 64, 0), (28, 64, 64),
              (224, 32, 64)]
    for h, cin, cout in shapes:
        bad = list(good)
        bad[5], bad[6], bad[7], bad[8] = 1, h, cin, cout
        assert lib.fac_conv3x3(*bad) == SHAPE, (h, cin, cout)
        assert lib.fac_conv3x3_packed_elems(h, cin, cout) == 0, (h, cin, cout)
    # the 14x14 / BN 192 tile has no fused pool: a shape error, before any launch
    for cout, pool, rc in ((192, 1, SHAPE), (192, 0, OK), (384, 1, OK), (128, 1, OK), (64, 1, OK)):
        call = list(good)
        call[8], call[9] = cout, pool
        assert lib.fac_conv3x3(*call) == rc, (cout, pool)
    assert lib.fac_conv3x3_packed_elems(14, 64, 192) == 9 * 64 * 192
    hw, ho = torch.zeros(9 * 64 * 64), torch.zeros(9 * 64 * 64, dtype=torch.int16)
    assert lib.fac_conv3x3_pack(0, 112, 64, 64, p(hw), p(ho)) == OK
    assert lib.fac_conv3x3_pack(0, 112, 64, 64, None, p(ho)) == ARG
    assert lib.fac_conv3x3_pack(0, 112, 64, 64, p(hw), None) == ARG
    assert lib.fac_conv3x3_pack(2, 112, 64, 64, p(hw), p(ho)) == ARG
    assert lib.fac_conv3x3_pack(0, 112, 48, 64, p(hw), p(ho)) == SHAPE
    torch.cuda.synchronize()


# ------------------------------------------------------------------ fac_stem224
def _stem_weights(dt, w1, b1, w2, b2, w3, b3):
    L, lib = _lib()
    w1p = torch.empty(32 * 64, dtype=torch.int16)
    wf = w1.float().reshape(32, 3, 9).contiguous()
    L.check(lib.fac_stem224_pack_conv1(L.DTYPES[dt], wf.data_ptr(), w1p.data_ptr()), None, "fac_stem224_pack_conv1")
    return (w1p.to(DEV), b1.float().to(DEV), _pack(dt, 224, w2), b2.float().to(DEV), _pack(dt, 224, w3),
            b3.float().to(DEV))


def _run_stem(dt, u8, inp, weights):
    L, lib = _lib()
    n = inp.shape[0]
    assert inp.dtype == (torch.uint8 if u8 else torch.float32)
    assert tuple(inp.shape) == ((n, 224, 224, 3) if u8 else (n, 3, 224, 224))
    src = inp.contiguous().to(DEV)
    buf = _out_buffer(n * 112 * 112 * 32, dt)
    L.check(lib.fac_stem224(L.DTYPES[dt], int(u8), src.data_ptr(), *[t.data_ptr() for t in weights], buf.data_ptr(),
                            n, torch.cuda.current_stream().cuda_stream), None, "fac_stem224")
    torch.cuda.synchronize()
    return _take(buf, (n, 112, 112, 32), dt)


@functools.lru_cache(maxsize=None)
def _stem_exact(n):
    ops = R.stem_exact_operands(n, 977 + n)
    ref = R.stem_ref(*ops, "fp16", False)          # exact: the same in either type
    return ops, ref


@pytest.mark.parametrize("schedule", ["one_box", "three_boxes"])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_stem_exact_integer_chain(dt, schedule):
    """Inputs in {0, 1}, sparse +-1 weights, integer biases (positive on conv1 and
    conv2), every stage an integer <= 256: the output EQUALS stem_ref.  n = 1:
    98 boxes, fewer than workgroups, the deferred store leaves only after the
    loop; three_boxes: the smallest n with 98 n >= 3 CUs."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 1 if schedule == "one_box" else -(-3 * cus // 98)
    assert (98 * n <= cus) if schedule == "one_box" else (98 * n >= 3 * cus)
    ops, ref = _stem_exact(n)
    inp, w1, b1, w2, b2, w3, b3 = ops
    assert max(R.stem_stage_maxima(*ops)) <= R.EXACT_MAX
    assert all(R.taps_and_channels_used(w) == (True, True) for w in (w1, w2, w3))
    assert int((w1 != 0).sum(dim=(1, 2, 3)).max()) <= 3
    assert max(int((w != 0).sum(dim=(1, 2, 3)).max()) for w in (w2, w3)) <= 4
    assert float(b1.min()) > 0 and float(b2.min()) > 0
    assert torch.equal(ref, ref.round()) and float(ref.max()) > 0
    assert torch.equal(ref, R.stem_ref(*ops, "bf16", False))
    out = _run_stem(dt, False, inp, _stem_weights(dt, *ops[1:]))
    assert torch.isfinite(out).all()
    bad = out != ref
    assert not bool(bad.any()), (f"{int(bad.sum())} of {bad.numel()} outputs differ, first at "
                                 f"(crop, y, x, channel) {tuple(int(i) for i in bad.nonzero()[0])}")


@functools.lru_cache(maxsize=None)
def _stem_random(dt, u8):
    ops = R.stem_random_operands(dt, u8)
    return ops, R.stem_ref(*ops, dt, u8, acc=torch.float64)


@functools.lru_cache(maxsize=None)
def _stem_random_out(dt, u8):
    ops, _ = _stem_random(dt, u8)
    return _run_stem(dt, u8, ops[0], _stem_weights(dt, *ops[1:]))


@pytest.mark.parametrize("path", ["u8", "f32"])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_stem_random_vs_fp64(dt, path):
    """Random operands, n = 3, against stem_ref accumulated in float64, inside 2x
    the measured float32-against-float64 envelope of the same operands
    (tests/golden/conv_stack_envelope.json, tools/conv_stack_envelope.py)."""
    env = json.loads((Path(__file__).resolve().parent / "golden" / "conv_stack_envelope.json").read_text())
    assert env["n"] == R.STEM_RANDOM_N and env["seed"] == R.STEM_RANDOM_SEED
    _, ref = _stem_random(dt, path == "u8")
    out = _stem_random_out(dt, path == "u8")
    assert torch.isfinite(out).all()
    ulp, flips = R.ulp_diff_and_flips(out, ref, dt)
    e = env[dt][path]
    print(f"stem random {dt} {path}: {ulp:.3f} ulp (gate {2 * e['ulp']:.3f}), "
          f"{flips:.3e} unequal (gate {2 * e['flips']:.3e})")
    assert ulp <= 2 * e["ulp"], (ulp, e["ulp"])
    assert flips <= 2 * e["flips"], (flips, e["flips"])


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_stem_u8_equals_f32_path(dt):
    """The fp32 path fed the host's fp32((v/255 - mean)/std) of the same uint8
    crops: both paths round the same fp32 value once, so the same bits."""
    ops, _ = _stem_random(dt, True)
    weights = _stem_weights(dt, *ops[1:])
    out_u8 = _stem_random_out(dt, True)
    out_f32 = _run_stem(dt, False, R.normalize_u8_f32(ops[0]), weights)
    assert torch.equal(out_u8, out_f32), int((out_u8 != out_f32).sum())


@pytest.mark.parametrize("path", ["u8", "f32"])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_stem_batch_independence(dt, path):
    """Crop 0 alone (98 boxes, one per workgroup) and as the last crop of a batch
    of three (two boxes for some workgroups): the same bits."""
    u8 = path == "u8"
    ops, _ = _stem_random(dt, u8)
    weights = _stem_weights(dt, *ops[1:])
    inp = ops[0]
    alone = _run_stem(dt, u8, inp[:1], weights)
    last = _run_stem(dt, u8, torch.cat([inp[1:], inp[:1]]), weights)
    assert torch.equal(last[-1:], alone)
    assert torch.equal(last[:2], _stem_random_out(dt, u8)[1:])


def test_stem_argument_returns():
    _, lib = _lib()
    ops = R.stem_exact_operands(1, 1)
    weights = _stem_weights("fp16", *ops[1:])
    src = ops[0].to(DEV)
    out = torch.empty(112 * 112 * 32, dtype=torch.float16, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    good = [1, 0, src.data_ptr(), *[t.data_ptr() for t in weights], out.data_ptr(), 1, st]
    assert lib.fac_stem224(*good) == OK
    for i in range(2, 10):
        bad = list(good)
        bad[i] = None
        assert lib.fac_stem224(*bad) == ARG, i
    for i, v in ((0, 2), (0, -1), (10, 0), (10, -1)):
        bad = list(good)
        bad[i] = v
        assert lib.fac_stem224(*bad) == ARG, (i, v)
    hw, ho = torch.zeros(32 * 27), torch.zeros(32 * 64, dtype=torch.int16)
    assert lib.fac_stem224_pack_conv1(0, hw.data_ptr(), ho.data_ptr()) == OK
    assert lib.fac_stem224_pack_conv1(0, None, ho.data_ptr()) == ARG
    assert lib.fac_stem224_pack_conv1(0, hw.data_ptr(), None) == ARG
    assert lib.fac_stem224_pack_conv1(2, hw.data_ptr(), ho.data_ptr()) == ARG
    torch.cuda.synchronize()
