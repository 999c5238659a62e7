"""Throughput of cvit_GGCA_ADD_DConv (fac_fake_amd/dconv.py) and the cost of
each fac_idwconv launch, on the GPU; writes profiles/dconv_bench.txt.

  python tools/bench_dconv.py [--batch 256] [--out profiles/dconv_bench.txt]

* crops/s of ``forward_u8`` at the batch size, fp16 and bf16, synthetic
  weights, next to the base ``cvit.CViT`` in the same process (device events
  around each stream-ordered forward, median after warm-up; models built and
  released one at a time).
* each of the model's nine ``fac_idwconv`` launches alone: time, the bytes/s it
  achieves on the bytes the layer has to move (the input map read once, the
  output map written once; halo re-reads are its own overhead and not counted),
  and a plain device copy of the input tensor (one read, one write) for scale.
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

from fac_fake_amd import _lib  # noqa: E402
from fac_fake_amd.prediction import dense_slots  # noqa: E402
from fac_fake_amd.weights import DCONV_LAYERS, make_crops, make_dconv_state_dict, make_state_dict  # noqa: E402

DEV = "cuda:0"
T16 = {"fp16": torch.float16, "bf16": torch.bfloat16}


def timed_ms(fn, warmup: int, reps: int):
    """Median and spread (min, max) of `reps` device-event timings of fn() after `warmup` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def bench_model(make, sd, crops, slots, warmup, reps):
    m = make()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    m.to(DEV)
    with torch.no_grad():
        t = timed_ms(lambda: m.forward_u8(crops, pos_index=slots), warmup, reps)
    torch.cuda.synchronize()
    m._release()
    return t


def idw_shapes():
    """(h, c, pool) of the model's nine InceptionDWConv2d layers, in order."""
    out, h = [], 224
    for _idx, kind, _ci, co, _bn, pool in DCONV_LAYERS:
        if kind == "idw":
            out.append((h, co, pool))
        if pool:
            h //= 2
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=str(REPO / "profiles" / "dconv_bench.txt"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_dconv.py needs a GPU: nothing is measured without one")
    from fac_fake_amd import cvit, dconv
    B = args.batch
    lines = [f"device: {torch.cuda.get_device_name(0)}; batch {B}; medians of {args.reps} after {args.warmup} warm-up "
             "calls; device events", ""]
    crops = torch.from_numpy(make_crops(min(B, 32), seed=41)).to(DEV)
    crops = crops.repeat((B + crops.shape[0] - 1) // crops.shape[0], 1, 1, 1)[:B].contiguous()
    slots = torch.from_numpy(dense_slots(B)).to(DEV)

    lines.append("forward_u8, ms per batch [min .. max] and crops/s")
    for dt in ("fp16", "bf16"):
        base = bench_model(lambda: cvit.CViT(dtype=dt), make_state_dict(0), crops, slots, args.warmup, args.reps)
        mine = bench_model(lambda: dconv.CViT(dtype=dt), make_dconv_state_dict(0), crops, slots, args.warmup, args.reps)
        for name, (med, lo, hi) in (("cvit (cvit.CViT)", base), ("cvit_GGCA_ADD_DConv (dconv.CViT)", mine)):
            lines.append(f"  {dt} {name:36s} {med:8.3f} [{lo:8.3f} .. {hi:8.3f}]  {B / med * 1e3:9.0f} crops/s  "
                         f"{base[0] / med:5.2f}x cvit")
    del crops

    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    reps = max(args.reps, 20)
    g = torch.Generator().manual_seed(9)
    for dt in ("fp16", "bf16"):
        lines += ["", f"fac_idwconv alone, {dt}, batch {B}, medians of {reps}: us [min .. max], TB/s on input + output "
                      "bytes; a device copy of the input (1 read + 1 write) beside it"]
        for h, c, pool in idw_shapes():
            gc = c // 8
            x = (torch.rand(B, h, h, c, generator=g) * 3).to(T16[dt]).to(DEV)
            ho = h // 2 if pool else h
            out = torch.empty(B, ho, ho, c, dtype=T16[dt], device=DEV)
            cp = torch.empty_like(x)
            ops = [t.to(DEV) for t in (torch.rand(gc, 9, generator=g) - 0.5, torch.rand(gc, 11, generator=g) - 0.5,
                                       torch.rand(gc, 11, generator=g) - 0.5, torch.rand(c, generator=g) + 0.5,
                                       torch.rand(c, generator=g) - 0.5)]

            def idw():
                _lib.check(lib.fac_idwconv(_lib.DTYPES[dt], x.data_ptr(), out.data_ptr(), B, h, h, c,
                                           *[t.data_ptr() for t in ops], int(pool), st), None, "fac_idwconv")

            ti = timed_ms(idw, args.warmup, reps)
            tc = timed_ms(lambda: cp.copy_(x), args.warmup, reps)
            moved = (x.numel() + out.numel()) * 2
            lines.append(f"  [{B},{h},{h},{c}] pool {int(pool)}  {ti[0] * 1e3:8.1f} us [{ti[1] * 1e3:8.1f} .. "
                         f"{ti[2] * 1e3:8.1f}]  {moved / ti[0] / 1e9:5.2f} TB/s on {moved / 1e6:7.1f} MB   copy "
                         f"{tc[0] * 1e3:8.1f} us  {2 * x.numel() * 2 / tc[0] / 1e9:5.2f} TB/s   idwconv / copy = "
                         f"{ti[0] / tc[0]:.2f}x")
            del x, out, cp
    text = "\n".join(lines) + "\n"
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
