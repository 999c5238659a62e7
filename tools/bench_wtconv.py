"""Cost of the WTConv block (wtconv.hip) and of cvit_GGCA_ADD_WTConv
(fac_fake_amd/wtconv.py) on the GPU; writes profiles/wtconv_bench.txt.

  python tools/bench_wtconv.py [--reps 20] [--batch 256] [--out profiles/wtconv_bench.txt] [--no-model]

* Per WT site shape (32 x 224^2, 64 x 112^2, 128 x 56^2, 256 x 28^2; without and
  with the fused pool) at B crops, fp16 and bf16, on the model's own folded
  operands and a post-ReLU random map: device events around one ``fac_wtconv``
  call, medians after warm-up with min and max, alternating call by call with
  two yardsticks from the same run:
    - the plain 3x3 conv C -> C the site replaces (``fac_conv3x3`` on random
      weights through the model's own packer, the same pool flag);
    - a plain device copy of the 16-bit input map (``Tensor.copy_``), whose
      read + write bytes over its time is the copy bandwidth; the site's
      read-once / write-once bytes over fac_wtconv's time is given as a
      fraction of it.
* ``forward_u8`` of the class at B crops, alternating with ``cvit_GGCA_ADD`` (the
  plain stem the class replaces nine convs of).
Nothing is gated on these figures: compare lines from one box only.

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

from fac_fake_amd import _lib  # noqa: E402
from fac_fake_amd.prediction import dense_slots  # noqa: E402
from fac_fake_amd.weights import make_crops, make_variant_state_dict, make_wtconv_state_dict  # noqa: E402

DEV = "cuda:0"
T16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
NAME, BASE = "cvit_GGCA_ADD_WTConv", "cvit_GGCA_ADD"
SITES = (2, 3, 5, 6, 8, 9, 12, 13)    # stem_plan labels: each site shape without and with the pool
FMA_PER_OUT = (16 + 100 + 16 + 100 + 4) / 4      # per output element and channel, halo recompute not counted


def events_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternating(fns, warmup, reps):
    ts = [[] for _ in fns]
    for i in range(warmup + reps):
        for t, fn in zip(ts, fns):
            v = events_ms(fn)
            if i >= warmup:
                t.append(v)
    return ts


def fmt(t):
    return f"{statistics.median(t) * 1e3:9.1f} us [{min(t) * 1e3:9.1f} .. {max(t) * 1e3:9.1f}]"


def build(make, sd):
    m = make()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.to(DEV)


def plain_conv(m, H, c, pool):
    """fac_conv3x3 c -> c at H x H on random weights through the model's own packer, or None where it has no such shape."""
    if _lib.load().fac_conv3x3_packed_elems(H, c, c) == 0:
        return None
    from fac_fake_amd.variants import Step
    g = torch.Generator().manual_seed(5)
    w = (torch.rand(c, c, 3, 3, generator=g) * 2 - 1) * (6.0 / (9 * c)) ** 0.5
    ops = (m._packed_conv(w, H, DEV), torch.zeros(c, device=DEV))
    s = Step("conv", (0,), H, c, c, pool, True)
    return lambda x, st: type(m)._step_conv(m, x, s, ops, True, st)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--no-model", action="store_true", help="skip the models' forwards")
    ap.add_argument("--out", default=str(REPO / "profiles" / "wtconv_bench.txt"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_wtconv.py needs a GPU: nothing is measured without one")
    from fac_fake_amd import variants, wtconv
    B = args.batch
    lines = [f"device: {torch.cuda.get_device_name(0)}; B = {B}; medians of {args.reps} after {args.warmup} warm-up calls, "
             "[min .. max]; device events; fac_wtconv, fac_conv3x3 and the copy alternate call by call", ""]
    g = torch.Generator(device=DEV).manual_seed(11)
    st = torch.cuda.current_stream().cuda_stream
    slots = torch.from_numpy(dense_slots(B)).to(DEV)
    crops = torch.from_numpy(make_crops(32, seed=41)).to(DEV).repeat((B + 31) // 32, 1, 1, 1)[:B].contiguous()
    for dt in ("fp16", "bf16"):
        a = build(lambda: wtconv.CViT(dtype=dt), make_wtconv_state_dict(NAME, 0))
        b = build(lambda: variants.CViT(BASE, dtype=dt), make_variant_state_dict(BASE, 0))
        for m in (a, b):
            m.reserve(B, DEV)
        for label in SITES:
            s, run, ops = [t for t in a._steps if label in t[0].labels][0]
            assert s.kind == "wt"
            x = torch.relu(torch.randn(B, s.H, s.H, s.co, generator=g, device=DEV) * 1.5 + 0.5).to(T16[dt])
            y = torch.empty_like(x)
            conv = plain_conv(b, s.H, s.co, s.pool)
            fns = [lambda: run(a, x, s, ops, True, st), lambda: y.copy_(x)] + ([lambda: conv(x, st)] if conv else [])
            with torch.no_grad():
                ts = alternating(fns, args.warmup, args.reps)
            t_wt, t_cp = statistics.median(ts[0]) * 1e-3, statistics.median(ts[1]) * 1e-3
            n_in = B * s.H * s.H * s.co
            n_out = n_in // 4 if s.pool else n_in
            bw_cp, bw_wt = 4 * n_in / t_cp, 2 * (n_in + n_out) / t_wt
            lines += [f"WTConv({s.co}) on [{B},{s.H},{s.H},{s.co}] {dt}{' + pool' if s.pool else ''}: the map is {2 * n_in / 1e6:.0f} MB",
                      f"  fac_wtconv (1 launch)      {fmt(ts[0])}  {bw_wt / 1e12:5.2f} TB/s read-once / write-once = "
                      f"{100 * bw_wt / bw_cp:4.1f} % of the copy's; {FMA_PER_OUT * n_in / t_wt / 1e12:5.2f} T fp32 fma/s",
                      f"  copy of the input map      {fmt(ts[1])}  {bw_cp / 1e12:5.2f} TB/s read + write"]
            if conv:
                lines.append(f"  fac_conv3x3 {s.co} -> {s.co}       {fmt(ts[2])}  WTConv / conv = {t_wt / (statistics.median(ts[2]) * 1e-3):.2f}")
            else:
                lines.append(f"  fac_conv3x3 has no {s.co} -> {s.co} shape at {s.H}x{s.H}: no plain conv beside it")
            del x, y
            torch.cuda.synchronize()
        lines.append("")
        if not args.no_model:
            with torch.no_grad():
                ta, tb = alternating([lambda: a.forward_u8(crops, pos_index=slots), lambda: b.forward_u8(crops, pos_index=slots)],
                                     args.warmup, max(args.reps // 2, 5))
            ma, mb = statistics.median(ta), statistics.median(tb)
            lines += [f"{dt}: forward_u8 at B = {B}, alternating",
                      f"  {NAME:<22} (wtconv.py)   {fmt(ta)}  {B / ma * 1e3:9.0f} crops/s",
                      f"  {BASE:<22} (variants.py) {fmt(tb)}  {B / mb * 1e3:9.0f} crops/s", ""]
        torch.cuda.synchronize()
        for m in (a, b):
            m._release()
    text = "\n".join(lines) + "\n"
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
