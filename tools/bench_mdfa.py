"""Cost of the MDFA block (mdfa.hip) and of the three MDFA CViT classes
(fac_fake_amd/mdfa.py) on the GPU; writes profiles/mdfa_bench.txt.

  python tools/bench_mdfa.py [--reps 20] [--out profiles/mdfa_bench.txt] [--no-model]

* ``fac_mdfa`` (one call, four launches) on random input and weights at the two
  model shapes (C, H) = (256, 14) and (512, 7), at B = 256 and B = 29, fp16 and
  bf16: device events around each call, medians after warm-up, with min and
  max.  Next to each figure its FLOP floor from the kept-tap count: per pixel
  the in-map taps of the 20 (14x14) or 12 (7x7) kept ones, C x C each, plus the
  conv_cat GEMM's 4C x C, over the 16-bit dense MFMA peak; and one read of the
  packed 16-bit weights that the shape uses at the HBM rate.
* ``forward_u8`` of each MDFA class alternating, call by call, with
  ``cvit_GGCA4`` (other.py: the same stem and tail with GGCA(256) alone) at
  B = 256, both dtypes.
Nothing is gated on these figures.

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
from fac_fake_amd.weights import MDFA_NAMES, make_crops, make_mdfa_state_dict, make_other_state_dict  # noqa: E402

DEV = "cuda:0"
T16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
PEAK_16BIT_FLOPS = 2.5e15        # MI355X dense fp16 / bf16 MFMA peak
HBM_BYTES_PER_S = 8.0e12         # MI355X HBM3E peak
SHAPES = [(256, 14), (512, 7)]
BATCHES = [256, 29]
DILATIONS = (6, 12, 18)


def in_map_products(h: int) -> tuple:
    """(C x C products per crop over the in-map taps of the four branches, kept taps of the 28) on an h x h map."""
    total, kept = h * h, 1
    for d in DILATIONS:
        axis = [sum(1 for k in (-1, 0, 1) if 0 <= p + k * d < h) for p in range(h)]
        total += sum(axis) ** 2
        kept += sum(1 for k in (-1, 0, 1) if abs(k) * d < h) ** 2
    return total, kept


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
    ap.add_argument("--no-model", action="store_true", help="skip the models' forwards")
    ap.add_argument("--out", default=str(REPO / "profiles" / "mdfa_bench.txt"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_mdfa.py needs a GPU: nothing is measured without one")
    from fac_fake_amd import mdfa, other
    lines = [f"device: {torch.cuda.get_device_name(0)}; medians of {args.reps} after {args.warmup} warm-up calls, "
             "[min .. max]; device events", ""]
    g = torch.Generator().manual_seed(11)
    u = lambda *s, a=1.0: (torch.rand(*s, generator=g) * 2 - 1) * a  # noqa: E731
    for c, h in SHAPES:
        ops = {"w1": u(c, c, a=(3.0 / c) ** 0.5)}
        for i in (2, 3, 4):
            ops[f"w{i}"] = u(c, c, 3, 3, a=(3.0 / (c * 4)) ** 0.5)
        ops.update(bias4=u(4, c, a=0.3), w5=u(c, c, a=(3.0 / c) ** 0.5), b5=u(c, a=0.3),
                   wcat=u(c, 5 * c, a=(3.0 / (5 * c)) ** 0.5) * 0.5, bcat=u(c, a=0.3),
                   ws=u(5 * c, a=(3.0 / (5 * c)) ** 0.5), wt=torch.rand(5 * c, generator=g) / (5 * c))
        prods, kept = in_map_products(h)
        wbytes = (kept + 4) * c * c * 2
        for dt in ("fp16", "bf16"):
            block = mdfa.FusedMDFA(ops, dt, DEV)
            for B in BATCHES:
                x = (torch.randn(B, h, h, c, generator=g) * 1.5).to(T16[dt]).to(DEV)
                flops = 2.0 * c * c * (prods + 4 * h * h) * B
                with torch.no_grad():
                    block(x)
                    torch.cuda.synchronize()
                    ta = [events_ms(lambda: block(x)) for _ in range(args.warmup + args.reps)][args.warmup:]
                ma = statistics.median(ta)
                f_flop, f_w = flops / PEAK_16BIT_FLOPS * 1e3, wbytes / HBM_BYTES_PER_S * 1e3
                lines += [f"MDFA({c}) on [{B},{h},{h},{c}] {dt}: {kept} of 28 taps kept, {prods / (h * h):.2f} in-map C x C "
                          f"products per pixel + 4 for conv_cat, {flops / 1e9:.1f} GFLOP, 16-bit weights in use {wbytes / 1e6:.1f} MB",
                          f"  fac_mdfa (4 launches) {fmt(ta)}  {flops / ma / 1e9:7.1f} TFLOP/s",
                          f"  floors: FLOP at {PEAK_16BIT_FLOPS / 1e15:.1f} PFLOP/s {f_flop * 1e3:8.1f} us (fac_mdfa is "
                          f"{ma / f_flop:.1f}x above it); one weight read at {HBM_BYTES_PER_S / 1e12:.0f} TB/s "
                          f"{f_w * 1e3:8.1f} us ({ma / f_w:.1f}x)"]
                del x
            del block
            lines.append("")
            torch.cuda.synchronize()

    if not args.no_model:
        B = 256
        crops = torch.from_numpy(make_crops(32, seed=41)).to(DEV).repeat(B // 32, 1, 1, 1).contiguous()
        slots = torch.from_numpy(dense_slots(B)).to(DEV)
        for dt in ("fp16", "bf16"):
            b = build(lambda: other.CViT("cvit_GGCA4", dtype=dt), make_other_state_dict("cvit_GGCA4", 0))
            for name in MDFA_NAMES:
                a = build(lambda: mdfa.CViT(name, dtype=dt), make_mdfa_state_dict(name, 0))
                a.reserve(B, DEV)
                with torch.no_grad():
                    ta, tb = alternating(lambda: a.forward_u8(crops, pos_index=slots),
                                         lambda: b.forward_u8(crops, pos_index=slots), args.warmup, max(args.reps // 2, 5))
                ma, mb = statistics.median(ta), statistics.median(tb)
                lines += [f"{dt}: forward_u8 at B = {B}, alternating",
                          f"  {name:<17} (mdfa.py)  {fmt(ta)}  {B / ma * 1e3:9.0f} crops/s",
                          f"  cvit_GGCA4        (other.py) {fmt(tb)}  {B / mb * 1e3:9.0f} crops/s",
                          f"  difference {1e3 * (ma - mb):8.1f} us = {100 * (ma - mb) / ma:4.1f} % of {name}'s forward", ""]
                torch.cuda.synchronize()
                a._release()
            b._release()
    text = "\n".join(lines) + "\n"
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
