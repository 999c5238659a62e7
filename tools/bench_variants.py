"""Throughput of the CViT variants (fac_fake_amd/variants.py) and the cost of the
streaming GGCA kernel, on the GPU; writes profiles/variants_bench.txt.

  python tools/bench_variants.py [--batch 256] [--out profiles/variants_bench.txt]

* crops/s of ``forward_u8`` at the batch size per variant, fp16, synthetic
  weights, next to ``repbn8.CViT`` in the same process (device events around
  each stream-ordered forward, median after warm-up; models built and released
  one at a time).
* ``fac_ggca_apply`` (op 1) on RepBn3's [batch,56,56,64] map alone: time, the
  bytes/s it achieves on the bytes the operation has to move (the map read
  twice - pooling and apply - and written once; the fp32 partials it keeps in
  its workspace are its own overhead and not counted), and a plain device copy
  of the same tensor (one read, one write) for scale.  The ratio of the two
  times is reported, not gated on.

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
from fac_fake_amd.weights import (VARIANT_NAMES, make_crops, make_repbn8_state_dict,  # noqa: E402
                                  make_variant_state_dict)

DEV = "cuda:0"


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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=str(REPO / "profiles" / "variants_bench.txt"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_variants.py needs a GPU: nothing is measured without one")
    from fac_fake_amd import repbn8, variants
    B = args.batch
    lines = [f"device: {torch.cuda.get_device_name(0)}; fp16; batch {B}; medians of {args.reps} after "
             f"{args.warmup} warm-up calls; device events", ""]
    crops = torch.from_numpy(make_crops(min(B, 32), seed=41)).to(DEV)
    crops = crops.repeat((B + crops.shape[0] - 1) // crops.shape[0], 1, 1, 1)[:B].contiguous()
    slots = torch.from_numpy(dense_slots(B)).to(DEV)

    lines.append("forward_u8, ms per batch [min .. max] and crops/s")
    base = bench_model(lambda: repbn8.CViT(dtype="fp16"), make_repbn8_state_dict(0), crops, slots, args.warmup,
                       args.reps)
    rows = [("cvit_GGCA_ADD_DEConv_RepBn8 (repbn8.CViT)", base)]
    for name in VARIANT_NAMES:
        rows.append((name, bench_model(lambda: variants.CViT(name, dtype="fp16"), make_variant_state_dict(name, 0),
                                       crops, slots, args.warmup, args.reps)))
    for name, (med, lo, hi) in rows:
        lines.append(f"  {name:44s} {med:8.3f} [{lo:8.3f} .. {hi:8.3f}]  {B / med * 1e3:9.0f} crops/s  "
                     f"{base[0] / med:5.2f}x RepBn8")
    del crops

    # fac_ggca_apply alone on RepBn3's map
    lib = _lib.load()
    h = w = 56
    c, groups, cg = 64, 4, 16
    g = torch.Generator().manual_seed(9)
    x = (torch.rand(B, h, w, c, generator=g) * 3).to(torch.float16).to(DEV)
    out = torch.empty_like(x)
    wts = [t.to(DEV) for t in (torch.rand(1, cg, generator=g) - 0.5, torch.zeros(1),
                               torch.tensor([[0.0], [1.0], [1.0], [0.0]]), torch.rand(cg, 1, generator=g) - 0.5,
                               torch.zeros(cg))]
    st = torch.cuda.current_stream().cuda_stream

    def ggca():
        _lib.check(lib.fac_ggca_apply(_lib.DTYPES["fp16"], x.data_ptr(), B, h, w, c, groups,
                                      *[t.data_ptr() for t in wts], 1, out.data_ptr(), st), None, "fac_ggca_apply")

    reps = max(args.reps, 20)
    tg = timed_ms(ggca, args.warmup, reps)
    tc = timed_ms(lambda: out.copy_(x), args.warmup, reps)
    map_bytes = x.numel() * 2
    lines += ["", f"fac_ggca_apply, op 1 (x + GGCA(x)), [{B},{h},{w},{c}] fp16, {map_bytes / 1e6:.1f} MB map, "
                  f"route {lib.fac_ggca_apply_route(h, w, c, groups)} (streaming), medians of {reps}",
              f"  fac_ggca_apply   {tg[0] * 1e3:8.1f} us [{tg[1] * 1e3:8.1f} .. {tg[2] * 1e3:8.1f}]  "
              f"{3 * map_bytes / tg[0] / 1e9:6.2f} TB/s on 3 x map (2 reads + 1 write)",
              f"  device copy      {tc[0] * 1e3:8.1f} us [{tc[1] * 1e3:8.1f} .. {tc[2] * 1e3:8.1f}]  "
              f"{2 * map_bytes / tc[0] / 1e9:6.2f} TB/s on 2 x map (1 read + 1 write)",
              f"  fac_ggca_apply / copy = {tg[0] / tc[0]:.2f}x the time for 1.5x the bytes"]
    text = "\n".join(lines) + "\n"
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
