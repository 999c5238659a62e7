"""Time ResKan (ResNet-34 + KAN) and the BasicBlock kernel against the route a
block would otherwise take.

  python tools/bench_reskan.py [--batch 256] [--reps 20] [--out profiles/reskan_bench.txt]

One GPU, one process, device events, medians over ``--reps`` calls after
warm-up; the variants of one shape alternate inside each repetition.

  model    ResKan forward_u8 at --batch crops, bf16 and fp16, replayed from its
           captured graph: ms per forward and crops/s
  conv2    for each of the four maps, at --batch crops and both dtypes:
           fac_conv3x3_res against fac_conv_nd with FAC_CONV_RESID |
           FAC_CONV_RELU2 (no first ReLU) on the same input, weights, bias and
           residual; the largest difference between the two outputs; TFLOP/s
           of each
  avgpool  fac_avgpool_f32 on [batch, 49, 512]

Routing rule (fac_fake_amd/reskan.py RES_KERNEL_MAPS): a map where
fac_conv3x3_res is not faster than fac_conv_nd keeps fac_conv_nd.
"""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

SHAPES = [(56, 64), (28, 128), (14, 256), (7, 512)]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from fac_fake_amd.ops import TORCH16, Conv3x3Res, ConvLayer, avgpool_f32
    from fac_fake_amd.reskan import resnet34
    from fac_fake_amd.weights import make_reskan_state_dict, reskan_crops_varied

    if not torch.cuda.is_available():
        raise SystemExit("bench_reskan needs a GPU (there is no CPU fallback)")
    dev = "cuda:0"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(fns, reps, warm=3):
        """median ms of each callable, alternating them inside each repetition"""
        for _ in range(warm):
            for f in fns:
                f()
        torch.cuda.synchronize()
        ts = [[] for _ in fns]
        for _ in range(reps):
            for i, f in enumerate(fns):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                b.synchronize()
                ts[i].append(a.elapsed_time(b))
        return [statistics.median(t) for t in ts]

    n = args.batch
    say(f"device: {torch.cuda.get_device_name(0)}; batch {n}; medians of {args.reps} after 3 warm-up calls; "
        "device events")

    # ---- model
    say("\nmodel: ResKan forward_u8 (graph replay)")
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in make_reskan_state_dict(0).items()}
    x = torch.from_numpy(reskan_crops_varied(min(n, 16), seed=47))
    x = x.repeat((n + x.shape[0] - 1) // x.shape[0], 1, 1, 1)[:n].contiguous().to(dev)
    for dt in ("bf16", "fp16"):
        m = resnet34(set_device=dev, num_classes=2, dtype=dt)
        m.load_state_dict(sd)
        m.forward_u8(x)
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                m.forward_u8(x)
        torch.cuda.synchronize()
        (ms,) = timed([g.replay], args.reps)
        say(f"  {dt}: {ms:8.3f} ms per forward, {n / ms * 1e3:9.0f} crops/s")
        del g, m
        torch.cuda.empty_cache()

    # ---- conv2 of a BasicBlock: the new kernel vs the generic route
    say("\nconv2 + bn2 + identity + ReLU alone: us per call")
    say(f"  {'map':>10} {'dtype':>5} | {'fac_conv3x3_res':>15} {'TFLOP/s':>8} | {'fac_conv_nd':>11} {'TFLOP/s':>8} | "
        f"{'nd / res':>8} | max |diff|")
    for h, c in SHAPES:
        for dt in ("bf16", "fp16"):
            gen = torch.Generator().manual_seed(h + c)
            w = torch.randn(c, c, 3, 3, generator=gen) / (9 * c) ** 0.5
            b = 0.2 * torch.randn(c, generator=gen)
            xin = torch.randn(n, 1, h, h, c, generator=gen).to(TORCH16[dt]).to(dev)
            res = torch.randn(n, 1, h, h, c, generator=gen).to(TORCH16[dt]).to(dev)
            new = Conv3x3Res(w, b, h, dtype=dt, device=dev)
            old = ConvLayer(w, b, 1, 1, dtype=dt, device=dev)
            o1, o2 = torch.empty_like(xin), torch.empty_like(xin)
            new(xin, res, out=o1)
            old(xin, relu=False, residual=res, relu2=True, out=o2)
            torch.cuda.synchronize()
            diff = float((o1.float() - o2.float()).abs().max())
            t1, t2 = timed([lambda: new(xin, res, out=o1),
                            lambda: old(xin, relu=False, residual=res, relu2=True, out=o2)], args.reps)
            fl = 2.0 * n * h * h * c * c * 9
            say(f"  {f'{h}x{h}x{c}':>10} {dt:>5} | {t1 * 1e3:15.1f} {fl / t1 / 1e9:8.1f} | {t2 * 1e3:11.1f} "
                f"{fl / t2 / 1e9:8.1f} | {t2 / t1:8.2f} | {diff:.2e}")
            del xin, res, o1, o2, new, old
            torch.cuda.empty_cache()

    # ---- pool
    f = torch.randn(n, 49, 512, device=dev).half()
    (ms,) = timed([lambda: avgpool_f32(f)], args.reps)
    say(f"\navgpool: fac_avgpool_f32 [{n}, 49, 512] fp16 -> fp32: {ms * 1e3:.1f} us "
        f"({f.numel() * 2 / ms / 1e9:.2f} TB/s read)")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
