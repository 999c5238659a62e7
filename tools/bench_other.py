"""Cost of the SMFA block (smfa.hip) in cvit_GGCA_SMFA (fac_fake_amd/other.py),
on the GPU; writes profiles/smfa_bench.txt.

  python tools/bench_other.py [--batch 256] [--out profiles/smfa_bench.txt]

* ``forward_u8`` of ``cvit_GGCA_SMFA`` alternating with ``cvit_GGCA_ADD``
  (variants.py: the same stem and a 7x7 GGCA combine, no SMFA) in one process,
  call by call, fp16 and bf16, synthetic weights: device events around each
  stream-ordered forward, medians after warm-up.  The difference is the
  block's end-to-end cost.
* ``fac_smfa`` alone at [B,14,14,256], next to two floors computed from the
  shapes: its FLOPs (2 * 196 * (256*512 + 512*512 + 768*256) per crop) over the
  fp16 dense MFMA peak, and its input + output bytes at the rate of a device
  copy of the same bytes timed beside it.
* for scale, the model's own 7x7 GGCA combine and its four 14x14 convs, each
  alone on the same batch.
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
from fac_fake_amd.weights import make_crops, make_other_state_dict, make_variant_state_dict  # noqa: E402

DEV = "cuda:0"
T16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
PEAK_16BIT_FLOPS = 2.5e15        # MI355X dense fp16 / bf16 MFMA peak
SMFA_C, SMFA_HW = 256, 14


def events_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed_ms(fn, warmup: int, reps: int):
    """Median and spread (min, max) of `reps` device-event timings of fn() after `warmup` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = [events_ms(fn) for _ in range(reps)]
    return statistics.median(out), min(out), max(out)


def build(make, sd):
    m = make()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.to(DEV)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=str(REPO / "profiles" / "smfa_bench.txt"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_other.py needs a GPU: nothing is measured without one")
    from fac_fake_amd import other, variants
    B = args.batch
    lines = [f"device: {torch.cuda.get_device_name(0)}; batch {B}; medians of {args.reps} after {args.warmup} warm-up "
             "calls; device events", ""]
    crops = torch.from_numpy(make_crops(min(B, 32), seed=41)).to(DEV)
    crops = crops.repeat((B + crops.shape[0] - 1) // crops.shape[0], 1, 1, 1)[:B].contiguous()
    slots = torch.from_numpy(dense_slots(B)).to(DEV)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    flops = 2.0 * B * SMFA_HW * SMFA_HW * (SMFA_C * 2 * SMFA_C + 4 * SMFA_C * SMFA_C + 3 * SMFA_C * SMFA_C)
    g = torch.Generator().manual_seed(9)

    for dt in ("fp16", "bf16"):
        dti = _lib.DTYPES[dt]
        smfa = build(lambda: other.CViT("cvit_GGCA_SMFA", dtype=dt), make_other_state_dict("cvit_GGCA_SMFA", 0))
        base = build(lambda: variants.CViT("cvit_GGCA_ADD", dtype=dt), make_variant_state_dict("cvit_GGCA_ADD", 0))
        ta, tb = [], []
        with torch.no_grad():
            for i in range(args.warmup + args.reps):            # alternating, call by call
                a = events_ms(lambda: smfa.forward_u8(crops, pos_index=slots))
                b = events_ms(lambda: base.forward_u8(crops, pos_index=slots))
                if i >= args.warmup:
                    ta.append(a)
                    tb.append(b)
        fa, fb = statistics.median(ta), statistics.median(tb)
        lines.append(f"{dt}: forward_u8, alternating, ms per batch [min .. max] and crops/s")
        for name, t, med in (("cvit_GGCA_SMFA (other.py)", ta, fa), ("cvit_GGCA_ADD  (variants.py)", tb, fb)):
            lines.append(f"  {name:30s} {med:8.3f} [{min(t):8.3f} .. {max(t):8.3f}]  {B / med * 1e3:9.0f} crops/s")
        lines.append(f"  difference {1e3 * (fa - fb):8.1f} us = {100 * (fa - fb) / fa:4.1f} % of cvit_GGCA_SMFA's forward")

        x = (torch.randn(B, SMFA_HW, SMFA_HW, SMFA_C, generator=g) * 1.5).to(T16[dt]).to(DEV)
        out, cp = torch.empty_like(x), torch.empty_like(x)
        scratch = torch.empty(lib.fac_smfa_scratch_bytes(B, SMFA_HW, SMFA_HW, SMFA_C), dtype=torch.uint8, device=DEV)
        wpk = smfa._smfa

        def block():
            _lib.check(lib.fac_smfa(dti, x.data_ptr(), B, SMFA_HW, SMFA_HW, SMFA_C, wpk.data_ptr(), 1, out.data_ptr(),
                                    None, scratch.data_ptr(), st), None, "fac_smfa")

        reps = max(args.reps, 20)
        tk = timed_ms(block, args.warmup, reps)
        tc = timed_ms(lambda: cp.copy_(x), args.warmup, reps)
        f_flop, f_copy = flops / PEAK_16BIT_FLOPS * 1e3, tc[0]
        lines += [f"  fac_smfa alone [{B},{SMFA_HW},{SMFA_HW},{SMFA_C}], x + SMFA(x), medians of {reps}:",
                  f"    {tk[0] * 1e3:8.1f} us [{tk[1] * 1e3:8.1f} .. {tk[2] * 1e3:8.1f}]  = {100 * tk[0] / fa:4.1f} % of the "
                  f"forward; scratch {scratch.numel() / 1e6:.1f} MB",
                  f"    floor 1, {flops / 1e9:.1f} GFLOP at {PEAK_16BIT_FLOPS / 1e15:.1f} PFLOP/s: {f_flop * 1e3:8.1f} us "
                  f"({tk[0] / f_flop:5.1f}x above it; {flops / tk[0] / 1e9:6.1f} TFLOP/s achieved)",
                  f"    floor 2, a device copy of the input (1 read + 1 write of {x.numel() * 2 / 1e6:.1f} MB): "
                  f"{f_copy * 1e3:8.1f} us ({tk[0] / f_copy:5.1f}x above it)",
                  f"    the nearer floor is the {'copy' if f_copy > f_flop else 'FLOP'} floor"]
        del out, cp, scratch

        # for scale: the model's 7x7 GGCA combine and its four 14x14 convs, each alone
        f7 = (torch.rand(B, 7, 7, 512, generator=g) * 3).to(T16[dt]).to(DEV)
        with torch.no_grad():
            tg = timed_ms(lambda: smfa.ggca_combine16(f7), args.warmup, reps)
        lines.append(f"  for scale: x + GGCA(x) on [{B},7,7,512] {tg[0] * 1e3:8.1f} us")
        convs = []
        for s, _run, ops in smfa._steps:
            if s.kind != "conv" or s.H != SMFA_HW:
                continue
            (wp, b), H, ci, co, pl, relu = ops, s.H, s.ci, s.co, s.pool, s.relu
            xi = (torch.rand(B, H, H, ci, generator=g) * 3).to(T16[dt]).to(DEV)
            yo = torch.empty(B, H // 2 if pl else H, H // 2 if pl else H, co, dtype=T16[dt], device=DEV)

            def conv():
                _lib.check(lib.fac_conv3x3(dti, xi.data_ptr(), wp.data_ptr(), b.data_ptr(), yo.data_ptr(), B, H, ci, co,
                                           int(pl), int(relu), smfa._zero.data_ptr(), st), None, "fac_conv3x3")

            t = timed_ms(conv, args.warmup, reps)
            convs.append(t[0])
            lines.append(f"  for scale: conv3x3 {ci:3d}->{co:3d} at 14x14{' + pool' if pl else '       '} {t[0] * 1e3:8.1f} us")
            del xi, yo
        three = sum(sorted(convs)[:3])
        lines.append(f"  the block is {tk[0] / (tg[0] + three):.2f}x the 7x7 GGCA plus the three cheapest 14x14 convs "
                     f"({(tg[0] + three) * 1e3:.1f} us)")
        lines.append("")
        torch.cuda.synchronize()
        smfa._release()
        base._release()
        del x, f7
    text = "\n".join(lines) + "\n"
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
