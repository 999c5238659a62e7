"""Cost of the ODConv block (odconv.hip) and of the two ODConv CViT classes
(fac_fake_amd/odconv.py) on the GPU; writes profiles/odconv_bench.txt.

  python tools/bench_odconv.py [--reps 20] [--batch 256] [--out profiles/odconv_bench.txt] [--no-model]

* Per ODConv site (64 x 112^2, 128 x 56^2, 256 x 28^2, 256 x 28^2 + pool of
  cvit_GGCA_ADD_ODConv; the bare 256 x 14^2 of cvit_GGCA_ODConv) at B crops, fp16
  and bf16, on the model's own packed weights and a post-ReLU random map: device
  events around the model's ``odconv`` step (one ``fac_odconv`` call), medians
  after warm-up with min and max, alternating call by call with the plain
  ``fac_conv3x3`` C -> C at the same shape in the same run (for the four stem
  sites the step of ``cvit_GGCA4`` that ODConv replaces; for 14^2 a conv packed
  here, where fac_conv3x3 has that shape); and the aggregated-weight traffic
  of the built route (9 c^2 16-bit values per crop, written once and read once).
* ``forward_u8`` of both classes alternating with ``cvit_GGCA4`` at B crops.
* ``--split CSV``: append the per-site, per-kernel split of fac_odconv from a
  per-dispatch kernel trace (csv) of a run of this tool, made in a run of its
  own with ``--no-model``.
* ``--append``: measure nothing; append the ``--split`` / ``--accuracy`` summaries
  to the existing ``--out`` file (needs no GPU).
* ``--accuracy LOG``: append the ranges of the figures tests/test_odconv_gpu.py
  printed (``pytest -s``).
Nothing is gated on these figures: compare lines from one box only.

There is no CPU path: without a GPU the tool fails.
"""
from __future__ import annotations

import argparse
import csv
import re
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fac_fake_amd import _lib  # noqa: E402
from fac_fake_amd.prediction import dense_slots  # noqa: E402
from fac_fake_amd.weights import make_crops, make_odconv_state_dict, make_other_state_dict  # noqa: E402

DEV = "cuda:0"
T16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
ADD, BARE, BASE = "cvit_GGCA_ADD_ODConv", "cvit_GGCA_ODConv", "cvit_GGCA4"
SITES = (5, 8, 11, 13)            # the stem_plan labels of the four ODConv steps of cvit_GGCA_ADD_ODConv


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
        a, b = events_ms(fa), (events_ms(fb) if fb is not None else 0.0)
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


def plain_conv_14(m, dt, B):
    """A fac_conv3x3 256 -> 256 at 14x14 on random weights through the model's own packer, or None where
    fac_conv3x3 has no such shape."""
    if _lib.load().fac_conv3x3_packed_elems(14, 256, 256) == 0:
        return None
    from fac_fake_amd.variants import Step
    g = torch.Generator().manual_seed(5)
    w = (torch.rand(256, 256, 3, 3, generator=g) * 2 - 1) * (6.0 / 2304) ** 0.5
    ops = (m._packed_conv(w, 14, DEV), torch.zeros(256, device=DEV))
    s = Step("conv", (0,), 14, 256, 256, False, True)
    return lambda x, st: type(m)._step_conv(m, x, s, ops, True, st)


def _col(header, *wants):
    low = [h.strip().lower() for h in header]
    for w in wants:
        if w in low:
            return low.index(w)
    raise SystemExit(f"the kernel trace has no column {wants[0]!r}; it has {header}")


def split_lines(path: Path):
    """Per ODConv site the time of each kernel of fac_odconv, from a per-dispatch
    kernel trace (csv: one row per dispatch with its name, start, end and grid)
    of a run of this tool.  A call is the dispatches from one odconv_mean_k to
    the next; its site is the conv kernel's width (in its name) and row tiles
    (its grid's x / 256 workgroups of 128 rows)."""
    with path.open() as f:
        rows = list(csv.reader(f))
    header, rows = rows[0], rows[1:]
    cn, cs, ce = _col(header, "kernel_name", "name"), _col(header, "start_timestamp"), _col(header, "end_timestamp")
    cg = _col(header, "grid_size_x", "grid_size")
    disp = sorted((int(r[cs]), int(r[ce]), r[cn], int(r[cg])) for r in rows if len(r) > max(cn, cs, ce, cg) and "odconv_" in r[cn])
    calls, cur = [], None
    for t0, t1, name, gx in disp:
        kind = re.search(r"odconv_(mean|att|agg|conv)_k", name).group(1)
        if kind == "mean":
            cur = {"mean": 0.0, "att": 0.0, "agg": 0.0, "conv": 0.0, "site": None}
            calls.append(cur)
        if cur is None:
            continue
        cur[kind] += (t1 - t0) / 1e3
        if kind == "conv":
            c = int(re.search(r"(\d+)\s*>", name).group(1))
            cur["site"] = (c, gx // 256)
    sites = {}
    for call in calls:
        if call["site"] is not None:
            sites.setdefault(call["site"], []).append(call)
    out = ["per-launch split, from a per-dispatch kernel trace of a run of this tool (--no-model; every call of both dtypes; "
           "medians over the calls of a site, the kernels of a call summed; pool and no pool at 256 x 28^2 together):"]
    for (c, tiles), cl in sorted(sites.items(), key=lambda kv: (kv[0][0], -kv[0][1])):
        med = {k: statistics.median(x[k] for x in cl) for k in ("mean", "att", "agg", "conv")}
        tot = sum(med.values())
        out.append(f"  ODConv({c}), {tiles} row tiles of 128 per crop, {len(cl)} calls: " +
                   ", ".join(f"odconv_{k}_k {med[k]:7.1f} us ({100 * med[k] / tot:4.1f} %)" for k in med) +
                   f"; sum {tot:7.1f} us; dominant: odconv_{max(med, key=med.get)}_k")
    return out


def accuracy_lines(log: Path):
    blk = re.compile(r"pool (\d) relu (\d) (fp16|bf16): relative L2 ([0-9.e+-]+) at ([0-9.]+) of its allowance, max\|d\| ([0-9.e+-]+) at ([0-9.]+)")
    att = re.compile(r"att \(.*\) \w+ (fp16|bf16): max\|d\| ([0-9.e+-]+), bound ([0-9.e+-]+), ratio ([0-9.]+)")
    site = re.compile(r"(cvit_\w+) (\S+) (fp16|bf16): relative L2 ([0-9.e+-]+) at ([0-9.]+) of its allowance, max\|d\| ([0-9.e+-]+) at ([0-9.]+)")
    mod = re.compile(r"(cvit_\w+) (fp16|bf16): max\|dp\| vs reference ([0-9.e+-]+) \(tolerance ([0-9.e+-]+)\)")
    rows, arows, extra = {"fp16": [], "bf16": []}, {"fp16": [], "bf16": []}, []
    for ln in log.read_text().splitlines():
        m = blk.search(ln)
        if m and not site.search(ln):
            rows[m.group(3)].append([float(v) for v in m.group(4, 5, 6, 7)])
        m = att.search(ln)
        if m:
            arows[m.group(1)].append([float(v) for v in m.group(2, 3, 4)])
        m = site.search(ln)
        if m:
            extra.append(f"  site {m.group(1)} {m.group(2)} {m.group(3)}: relative L2 {m.group(4)} at {m.group(5)} of its allowance, "
                         f"max|d| {m.group(6)} at {m.group(7)}")
        m = mod.search(ln)
        if m:
            extra.append(f"  model {m.group(1)} {m.group(2)}: max|dp| {m.group(3)} of {m.group(4)} allowed")
    out = ["accuracy, from tests/test_odconv_gpu.py on the same box:"]
    for dt in ("fp16", "bf16"):
        r, a = np.array(rows[dt]), np.array(arows[dt])
        if len(r):
            out.append(f"  {dt}: {len(r)} block cases: relative L2 up to {r[:, 0].max():.3e} (at most {r[:, 1].max():.3f} of its allowance); "
                       f"max|d| up to {r[:, 2].max():.3e} (at most {r[:, 3].max():.3f} of its allowance)")
        if len(a):
            out.append(f"  {dt}: {len(a)} attention cases: max|d| up to {a[:, 0].max():.3e}; bounds {a[:, 1].min():.3e} .. {a[:, 1].max():.3e}; "
                       f"ratio up to {a[:, 2].max():.3f}")
    return out + extra


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--no-model", action="store_true", help="skip the models' forwards")
    ap.add_argument("--split", default=None, help="a per-dispatch kernel trace (csv) of a run of this tool to summarise")
    ap.add_argument("--append", action="store_true", help="measure nothing: append the summaries to the existing --out file")
    ap.add_argument("--accuracy", default=None, help="a pytest -s log of tests/test_odconv_gpu.py to summarise")
    ap.add_argument("--out", default=str(REPO / "profiles" / "odconv_bench.txt"))
    args = ap.parse_args(argv)
    if args.append:
        extra = (split_lines(Path(args.split)) + [""] if args.split else []) + \
            (accuracy_lines(Path(args.accuracy)) + [""] if args.accuracy else [])
        text = Path(args.out).read_text() + "\n".join(extra) + "\n"
        print("\n".join(extra))
        Path(args.out).write_text(text)
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_odconv.py needs a GPU: nothing is measured without one")
    from fac_fake_amd import odconv, other
    B = args.batch
    lines = [f"device: {torch.cuda.get_device_name(0)}; B = {B}; medians of {args.reps} after {args.warmup} warm-up calls, "
             "[min .. max]; device events", ""]
    g = torch.Generator().manual_seed(11)
    st = torch.cuda.current_stream().cuda_stream
    slots = torch.from_numpy(dense_slots(B)).to(DEV)
    crops = torch.from_numpy(make_crops(32, seed=41)).to(DEV).repeat((B + 31) // 32, 1, 1, 1)[:B].contiguous()
    lib = _lib.load()
    for dt in ("fp16", "bf16"):
        a = build(lambda: odconv.CViT(ADD, dtype=dt), make_odconv_state_dict(ADD, 0))
        c = build(lambda: odconv.CViT(BARE, dtype=dt), make_odconv_state_dict(BARE, 0))
        b = build(lambda: other.CViT(BASE, dtype=dt), make_other_state_dict(BASE, 0))
        for m in (a, b, c):
            m.reserve(B, DEV)
        cases = []
        for label in SITES:
            sa, ra, oa = [t for t in a._steps if label in t[0].labels][0]
            sb, rb, ob = [t for t in b._steps if label in t[0].labels][0]
            assert sa.kind == "odconv" and sb.kind == "conv" and (sa.H, sa.co, sa.pool) == (sb.H, sb.co, sb.pool) and sb.ci == sb.co
            cases.append((sa, (lambda x, ra=ra, sa=sa, oa=oa: ra(a, x, sa, oa, True, st)),
                          (lambda x, rb=rb, sb=sb, ob=ob: rb(b, x, sb, ob, True, st)), f"{BASE}'s step"))
        sc, rc, oc = [t for t in c._steps if "odconv" in t[0].labels][0]
        plain = plain_conv_14(b, dt, B)
        cases.append((sc, (lambda x: rc(c, x, sc, oc, True, st)), (lambda x: plain(x, st)) if plain else None, "packed here"))
        for s, fa, fb, what in cases:
            x = torch.relu(torch.randn(B, s.H, s.H, s.co, generator=g) * 1.5 + 0.5).to(T16[dt]).to(DEV)
            with torch.no_grad():
                ta, tb = alternating(lambda: fa(x), (lambda: fb(x)) if fb else None, args.warmup, args.reps)
            ma = statistics.median(ta)
            wbytes = 2 * B * 9 * s.co * s.co * 2
            chunk = lib.fac_odconv_chunk(B, s.co)
            launches = 2 + 2 * ((B + chunk - 1) // chunk)
            tag = f"{' + pool' if s.pool else ''}{'' if s.relu else ', bare (no BatchNorm, no ReLU)'}"
            lines += [f"ODConv({s.co}) on [{B},{s.H},{s.H},{s.co}] {dt}{tag}: the map is {B * s.H * s.H * s.co * 2 / 1e6:.0f} MB; the "
                      f"aggregated weights are {wbytes / 2e6:.0f} MB, written once and read once; scratch "
                      f"{lib.fac_odconv_scratch_bytes(B, s.H, s.H, s.co) / 1e6:.0f} MB",
                      f"  fac_odconv ({launches} launches)          {fmt(ta)}"]
            if fb:
                lines.append(f"  fac_conv3x3 {s.co} -> {s.co} ({what})  {fmt(tb)}  ODConv / conv = {ma / statistics.median(tb):.2f}")
            else:
                lines.append(f"  fac_conv3x3 has no {s.co} -> {s.co} shape at {s.H}x{s.H}: no plain conv beside it")
            del x
            torch.cuda.synchronize()
        lines.append("")
        if not args.no_model:
            for m, name in ((a, ADD), (c, BARE)):
                with torch.no_grad():
                    ta, tb = alternating(lambda: m.forward_u8(crops, pos_index=slots), lambda: b.forward_u8(crops, pos_index=slots),
                                         args.warmup, max(args.reps // 2, 5))
                ma, mb = statistics.median(ta), statistics.median(tb)
                lines += [f"{dt}: forward_u8 at B = {B}, alternating",
                          f"  {name:<22} (odconv.py) {fmt(ta)}  {B / ma * 1e3:9.0f} crops/s",
                          f"  {BASE:<22} (other.py)  {fmt(tb)}  {B / mb * 1e3:9.0f} crops/s",
                          f"  difference {1e3 * (ma - mb):8.1f} us = {100 * (ma - mb) / ma:4.1f} % of {name}'s forward", ""]
        torch.cuda.synchronize()
        for m in (a, b, c):
            m._release()
    if args.split:
        lines += split_lines(Path(args.split)) + [""]
    if args.accuracy:
        lines += accuracy_lines(Path(args.accuracy)) + [""]
    text = "\n".join(lines) + "\n"
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
