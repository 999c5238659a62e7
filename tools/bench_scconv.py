"""Cost of the ScConv block (scconv.hip) and of cvit_GGCA_ADD_ScConv
(fac_fake_amd/scconv.py) on the GPU; writes profiles/scconv_bench.txt.

  python tools/bench_scconv.py [--reps 20] [--batch 256] [--out profiles/scconv_bench.txt] [--no-model]

* Per ScConv site of the class (64 x 112^2, 128 x 56^2, 256 x 28^2, 256 x 28^2 +
  pool) at B crops, fp16 and bf16, on the model's own packed weights and a
  post-ReLU random map: device events around the model's ``scconv`` step (one
  ``fac_scconv`` call, six launches), medians after warm-up with min and max;
  the bytes the built route has to move at least (x read twice, u | l written
  once and read twice, the output written once) and the rate that makes; and
  beside it the plain ``fac_conv3x3`` C -> C step of ``cvit_GGCA4`` at the same
  site, the layer ScConv replaces.
* ``forward_u8`` of the class alternating, call by call, with ``cvit_GGCA4``
  (the same stem with plain convs, GGCA(256) and the same tail) at B crops.
* ``--accuracy LOG``: append the tau, excluded-share and error lines that
  tests/test_scconv_gpu.py printed (``pytest -s``) into the same file.
Nothing is gated on these figures: compare lines from one box only.

There is no CPU path: without a GPU the tool fails.
"""
from __future__ import annotations

import argparse
import re
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fac_fake_amd.prediction import dense_slots  # noqa: E402
from fac_fake_amd.weights import make_crops, make_other_state_dict, make_scconv_state_dict  # noqa: E402

DEV = "cuda:0"
T16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
NAME, BASE = "cvit_GGCA_ADD_ScConv", "cvit_GGCA4"
SITES = (5, 8, 11, 13)            # the stem_plan labels of the four ScConv steps


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


def route_bytes(B, h, c, pool):
    M = B * h * h
    return 2 * M * c * 2 + 3 * M * (c // 2) * 2 + M * c * 2 // (4 if pool else 1)


def accuracy_lines(log: Path):
    """Per dtype the ranges of tau, the excluded share and the errors of test_block_vs_float64_reference, from a pytest -s log."""
    pat = re.compile(r"\((\d+), (\d+), (\d+), (\d+)\) (\w+) pool (\d) (fp16|bf16): tau ([0-9.e+-]+), excluded ([0-9.]+); relative L2 "
                     r"([0-9.e+-]+) at ([0-9.]+) of its allowance, max\|d\| ([0-9.e+-]+) at ([0-9.]+)")
    stat = re.compile(r"(fp16|bf16): tau ([0-9.e+-]+), max\|t_stats - t_float64\| ([0-9.e+-]+) \(([0-9.]+) tau\)")
    rows, srows = {"fp16": [], "bf16": []}, {"fp16": [], "bf16": []}
    for ln in log.read_text().splitlines():
        m = pat.search(ln)
        if m:
            rows[m.group(7)].append([float(v) for v in m.group(8, 9, 10, 11, 12, 13)])
        m = stat.search(ln)
        if m:
            srows[m.group(1)].append([float(v) for v in m.group(2, 3, 4)])
    out = ["accuracy, from tests/test_scconv_gpu.py on the same box (test_statistics, test_block_vs_float64_reference):"]
    for dt in ("fp16", "bf16"):
        r, s = np.array(rows[dt]), np.array(srows[dt])
        if not len(r) or not len(s):
            continue
        out += [f"  {dt}: {len(r)} block cases: tau {r[:, 0].min():.2e} .. {r[:, 0].max():.2e}; excluded share up to {r[:, 1].max():.4f}; "
                f"relative L2 up to {r[:, 2].max():.3e} ({r[:, 3].max():.3f} of its allowance); max|d| up to {r[:, 4].max():.3e} "
                f"({r[:, 5].max():.3f} of its allowance)",
                f"  {dt}: {len(s)} statistics cases: max|t_stats - t_float64| up to {s[:, 1].max():.3e} = {s[:, 2].max():.3f} tau "
                f"(the bound is tau / 4)"]
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--no-model", action="store_true", help="skip the models' forwards")
    ap.add_argument("--accuracy", default=None, help="a pytest -s log of tests/test_scconv_gpu.py to summarise")
    ap.add_argument("--out", default=str(REPO / "profiles" / "scconv_bench.txt"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_scconv.py needs a GPU: nothing is measured without one")
    from fac_fake_amd import other, scconv
    B = args.batch
    lines = [f"device: {torch.cuda.get_device_name(0)}; B = {B}; medians of {args.reps} after {args.warmup} warm-up calls, "
             "[min .. max]; device events", ""]
    g = torch.Generator().manual_seed(11)
    st = torch.cuda.current_stream().cuda_stream
    slots = torch.from_numpy(dense_slots(B)).to(DEV)
    crops = torch.from_numpy(make_crops(32, seed=41)).to(DEV).repeat((B + 31) // 32, 1, 1, 1)[:B].contiguous()
    for dt in ("fp16", "bf16"):
        a = build(lambda: scconv.CViT(NAME, dtype=dt), make_scconv_state_dict(NAME, 0))
        b = build(lambda: other.CViT(BASE, dtype=dt), make_other_state_dict(BASE, 0))
        a.reserve(B, DEV)
        b.reserve(B, DEV)
        for label in SITES:
            sa, ra, oa = [t for t in a._steps if label in t[0].labels][0]
            sb, rb, ob = [t for t in b._steps if label in t[0].labels][0]
            assert sa.kind == "scconv" and sb.kind == "conv" and (sa.H, sa.co, sa.pool) == (sb.H, sb.co, sb.pool) and sb.ci == sb.co
            x = torch.relu(torch.randn(B, sa.H, sa.H, sa.co, generator=g) * 1.5 + 0.5).to(T16[dt]).to(DEV)
            with torch.no_grad():
                ta, tb = alternating(lambda: ra(a, x, sa, oa, True, st), lambda: rb(b, x, sb, ob, True, st), args.warmup, args.reps)
            ma, mb = statistics.median(ta), statistics.median(tb)
            nbytes = route_bytes(B, sa.H, sa.co, sa.pool)
            lines += [f"ScConv({sa.co}) on [{B},{sa.H},{sa.H},{sa.co}] {dt}{' + pool' if sa.pool else ''}: the map is "
                      f"{B * sa.H * sa.H * sa.co * 2 / 1e6:.0f} MB; the route moves at least {nbytes / 1e6:.0f} MB",
                      f"  fac_scconv (6 launches)       {fmt(ta)}  {nbytes / ma / 1e9:7.2f} TB/s of that minimum",
                      f"  fac_conv3x3 {sb.ci} -> {sb.co} ({BASE})  {fmt(tb)}  ScConv / conv = {ma / mb:.2f}"]
            del x
            torch.cuda.synchronize()
        lines.append("")
        if not args.no_model:
            with torch.no_grad():
                ta, tb = alternating(lambda: a.forward_u8(crops, pos_index=slots), lambda: b.forward_u8(crops, pos_index=slots),
                                     args.warmup, max(args.reps // 2, 5))
            ma, mb = statistics.median(ta), statistics.median(tb)
            lines += [f"{dt}: forward_u8 at B = {B}, alternating",
                      f"  {NAME:<22} (scconv.py) {fmt(ta)}  {B / ma * 1e3:9.0f} crops/s",
                      f"  {BASE:<22} (other.py)  {fmt(tb)}  {B / mb * 1e3:9.0f} crops/s",
                      f"  difference {1e3 * (ma - mb):8.1f} us = {100 * (ma - mb) / ma:4.1f} % of {NAME}'s forward", ""]
        torch.cuda.synchronize()
        a._release()
        b._release()
    if args.accuracy:
        lines += accuracy_lines(Path(args.accuracy)) + [""]
    text = "\n".join(lines) + "\n"
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
