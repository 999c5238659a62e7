"""Cost of the BFM block (bfm.hip) and of cvit_GGCA4_BFM5 (fac_fake_amd/bfm.py)
on the GPU; writes profiles/bfm_bench.txt.

  python tools/bench_bfm.py [--reps 20] [--out profiles/bfm_bench.txt] [--no-model]

* ``fac_bfm`` (one launch) alternating, call by call in one process, with
  ``bfm.ComposedBFM`` (three fac_conv_nd / fac_conv3x3 launches, fac_ew add3,
  fac_ew affine) on the same random input and weights, at the two model shapes
  (C, H) = (512, 7) and (256, 14), at B = 256 and B = 29, fp16 and bf16: device
  events around each call, medians after warm-up, with min and max.  Next to
  each figure its two floors, computed from the shapes: 2 * 83 * C^2 * H^2 FLOP
  per crop over the 16-bit dense MFMA peak, and one read of the packed weights
  (83 * C^2 * 2 bytes) at the HBM rate.  The outputs of the two routes are
  compared on those inputs (relative L2).
* ``forward_u8`` of ``cvit_GGCA4_BFM5`` alternating with ``cvit_GGCA4``
  (other.py: the same forward minus the block) at B = 256, both dtypes: the
  difference is the block's end-to-end cost.
Nothing is gated on these figures; bfm.MODEL_ROUTE is set by hand from them.

There is no CPU path: without a GPU the tool fails.
"""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fac_fake_amd.prediction import dense_slots  # noqa: E402
from fac_fake_amd.weights import make_bfm_state_dict, make_crops, make_other_state_dict  # noqa: E402

DEV = "cuda:0"
T16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
PEAK_16BIT_FLOPS = 2.5e15        # MI355X dense fp16 / bf16 MFMA peak
HBM_BYTES_PER_S = 8.0e12         # MI355X HBM3E peak
SHAPES = [(512, 7), (256, 14)]
BATCHES = [256, 29]


def events_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternating(fa, fb, warmup, reps):
    ta, tb = [], []
    for i in range(warmup + reps):
        a, b = events_ms(fa), events_ms(fb)
        if i >= warmup:
            ta.append(a)
            tb.append(b)
    return ta, tb


def fmt(t):
    return f"{statistics.median(t) * 1e3:9.1f} us [{min(t) * 1e3:9.1f} .. {max(t) * 1e3:9.1f}]"


def build(make, sd):
    m = make()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.to(DEV)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-model", action="store_true", help="skip the two models' forwards")
    ap.add_argument("--out", default=str(REPO / "profiles" / "bfm_bench.txt"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_bfm.py needs a GPU: nothing is measured without one")
    from fac_fake_amd import bfm, other
    lines = [f"device: {torch.cuda.get_device_name(0)}; medians of {args.reps} after {args.warmup} warm-up calls, "
             "[min .. max]; device events; the two routes alternate call by call", ""]
    g = torch.Generator().manual_seed(11)
    u = lambda *s, a=1.0: (torch.rand(*s, generator=g) * 2 - 1) * a  # noqa: E731
    faster = {}
    for c, h in SHAPES:
        ops = {f"w{k}": u(c, c, k, k, a=(3.0 / (c * k * k)) ** 0.5) for k in (3, 5, 7)}
        ops["bias3"] = u(3, c, a=0.3)
        wbytes = 83 * c * c * 2
        for dt in ("fp16", "bf16"):
            fused, comp = bfm.FusedBFM(ops, dt, DEV), bfm.ComposedBFM(ops, dt, DEV)
            for B in BATCHES:
                x = (torch.randn(B, h, h, c, generator=g) * 1.5).to(T16[dt]).to(DEV)
                flops = 2.0 * 83 * c * c * h * h * B
                with torch.no_grad():
                    ya, yb = fused(x), comp(x)
                    torch.cuda.synchronize()
                    rel = float((ya.double() - yb.double()).norm() / yb.double().norm())
                    ta, tb = alternating(lambda: fused(x), lambda: comp(x), args.warmup, args.reps)
                ma, mb = statistics.median(ta), statistics.median(tb)
                f_flop, f_w = flops / PEAK_16BIT_FLOPS * 1e3, wbytes / HBM_BYTES_PER_S * 1e3
                faster[c, h, dt, B] = ma < mb
                lines += [f"BFM({c}) on [{B},{h},{h},{c}] {dt}: {flops / 1e9:.1f} GFLOP, packed weights {wbytes / 1e6:.1f} MB",
                          f"  fac_bfm (1 launch)          {fmt(ta)}  {flops / ma / 1e9:7.1f} TFLOP/s",
                          f"  bfm16_composed (5 launches) {fmt(tb)}  {flops / mb / 1e9:7.1f} TFLOP/s",
                          f"  fused / composed = {ma / mb:.3f}; outputs differ by {rel:.2e} relative L2",
                          f"  floors: FLOP at {PEAK_16BIT_FLOPS / 1e15:.1f} PFLOP/s {f_flop * 1e3:8.1f} us (fused is "
                          f"{ma / f_flop:.1f}x above it); one weight read at {HBM_BYTES_PER_S / 1e12:.0f} TB/s "
                          f"{f_w * 1e3:8.1f} us ({ma / f_w:.1f}x)"]
                del x, ya, yb
            del fused, comp
            lines.append("")
            torch.cuda.synchronize()
    ok = all(v for (c, h, dt, B), v in faster.items() if B == 256)
    lines += [f"fused faster than composed at B = 256 in every shape and dtype: {ok}", ""]

    if not args.no_model:
        B = 256
        crops = torch.from_numpy(make_crops(32, seed=41)).to(DEV).repeat(B // 32, 1, 1, 1).contiguous()
        slots = torch.from_numpy(dense_slots(B)).to(DEV)
        for dt in ("fp16", "bf16"):
            a = build(lambda: bfm.CViT("cvit_GGCA4_BFM5", dtype=dt), make_bfm_state_dict("cvit_GGCA4_BFM5", 0))
            b = build(lambda: other.CViT("cvit_GGCA4", dtype=dt), make_other_state_dict("cvit_GGCA4", 0))
            with torch.no_grad():
                ta, tb = alternating(lambda: a.forward_u8(crops, pos_index=slots),
                                     lambda: b.forward_u8(crops, pos_index=slots), args.warmup, max(args.reps // 2, 5))
            ma, mb = statistics.median(ta), statistics.median(tb)
            lines += [f"{dt}: forward_u8 at B = {B}, alternating (bfm step: {bfm.MODEL_ROUTE})",
                      f"  cvit_GGCA4_BFM5 (bfm.py)   {fmt(ta)}  {B / ma * 1e3:9.0f} crops/s",
                      f"  cvit_GGCA4      (other.py) {fmt(tb)}  {B / mb * 1e3:9.0f} crops/s",
                      f"  difference {1e3 * (ma - mb):8.1f} us = {100 * (ma - mb) / ma:4.1f} % of cvit_GGCA4_BFM5's forward", ""]
            torch.cuda.synchronize()
            a._release()
            b._release()
    text = "\n".join(lines) + "\n"
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
