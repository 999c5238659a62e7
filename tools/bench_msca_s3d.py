"""Time msca_S3D's new kernels (csrc/msca.hip), the host-side choices around
them, and the model, on one GPU in one process.

  python tools/bench_msca_s3d.py [--batch 64] [--reps 20] [--out profiles/msca_s3d_bench.txt]

Device events, medians over ``--reps`` calls after warm-up; the variants of one
shape alternate inside each repetition.

  ops      every new op on the model's own maps at 20 x 224^2 clips (10 x 28^2
           at 64, 128 and 768 channels; 5 x 14^2 at 48 .. 224 and 1280), --batch
           clips, fp16, against the same arithmetic as eager torch ops on the
           same tensors (channels-last views).  "bytes" is the traffic no
           implementation can avoid (each operand read once, the result written
           once); "GB/s" is that traffic over the measured time
  choices  a 1x1x1 conv on a channel slice: zero weight columns over the full
           width (what the model does) against a slice copy + the narrow conv;
           the MSCA sum: three launches (what the model does; a fused launch
           was not built) against eager torch
  models   msca_S3D against fac_fake_amd's S3D (both fp16, SRM_net 'no', float
           clips, replayed from captured graphs) and against the eager torch
           fp16 run of the test restatement (tests/msca_s3d_ref.py), all at
           --batch clips of 16 x 112^2

The parent commit has no such model, so eager torch on the same box is the
only baseline for the ops.
"""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

# (T, H, W, C, kt) of the depthwise convs at the harness shape
DW_MAPS = [(10, 28, 28, 64, 1), (10, 28, 28, 128, 1), (10, 28, 28, 768, 3), (5, 14, 14, 48, 3), (5, 14, 14, 96, 3),
           (5, 14, 14, 160, 3), (5, 14, 14, 224, 3), (5, 14, 14, 1280, 3)]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.nn.functional as F

    import msca_s3d_ref as R
    from fac_fake_amd import ops
    from fac_fake_amd.msca_s3d import msca_S3D
    from fac_fake_amd.s3d import S3D
    from fac_fake_amd.weights import make_msca_s3d_state_dict, make_s3d_state_dict, s3d_clips

    if not torch.cuda.is_available():
        raise SystemExit("bench_msca_s3d needs a GPU (there is no CPU fallback)")
    dev, n = "cuda:0", args.batch
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(fns, reps=args.reps, warm=3):
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

    def row(name, shape, nbytes, hip_ms, torch_ms):
        say(f"| {name} | {'x'.join(map(str, shape))} | {nbytes / 1e6:.1f} | {hip_ms * 1e3:.1f} | "
            f"{nbytes / hip_ms / 1e6:.0f} | {torch_ms * 1e3:.1f} | {torch_ms / hip_ms:.2f} |")

    g = torch.Generator().manual_seed(0)
    say(f"# msca_S3D kernels, {n} clips, fp16, {torch.cuda.get_device_name(0)}")
    say()
    say("## ops (bytes: operands read once + result written once, MB; GB/s over that)")
    say("| op | map TxHxWxC | MB | HIP us | GB/s | torch us | torch / HIP |")
    say("|---|---|---|---|---|---|---|")
    for (t, h, w, c, kt) in DW_MAPS:
        x = torch.randn(n, t, h, w, c, generator=g).half().to(dev)
        xn = x.permute(0, 4, 1, 2, 3)                       # NCDHW view, channels-last memory
        for k in ((3,) if c in (768, 1280) else (3, 5, 7)):
            ws = torch.randn(c, 1, 1, k, k, generator=g) / k
            wt = torch.randn(c, 1, kt, 1, 1, generator=g)
            sc, sh = 1 + torch.rand(c, generator=g), torch.rand(c, generator=g)
            act = "gelu" if c in (768, 1280) else "none"
            layer = ops.DWSepLayer(ws, wt, sc, sh, act=act, dtype="fp16", device=dev)
            wsd, wtd = ws.half().to(dev), wt.half().to(dev)
            scd, shd = sc.half().to(dev).view(1, -1, 1, 1, 1), sh.half().to(dev).view(1, -1, 1, 1, 1)

            def eager():
                y = F.conv3d(F.conv3d(xn, wsd, padding=(0, k // 2, k // 2), groups=c), wtd, padding=(kt // 2, 0, 0), groups=c)
                y = (y * scd + shd).clamp(0, 6)
                return F.gelu(y) if act == "gelu" else y
            a, b = timed([lambda: layer(x), eager])
            row(f"dwsep3d k={k} kt={kt} {act}", (t, h, w, c), 2 * x.numel() * 2, a, b)
    for (t, h, w, c, kt) in [(10, 28, 28, 64, 1), (5, 14, 14, 112, 3), (5, 14, 14, 48, 3)]:
        full = torch.randn(n, t, h, w, 192 if c == 64 else 320, generator=g).half().to(dev)
        sc, sh = torch.randn(c, generator=g).to(dev), torch.randn(c, generator=g).to(dev)
        a, b = timed([lambda: ops.bn_max_pool(full, sc, sh, kt, c=c),
                      lambda: F.max_pool3d((full[..., :c] * sc.half() + sh.half()).permute(0, 4, 1, 2, 3), (kt, 3, 3), 1,
                                           (kt // 2, 1, 1))])
        row(f"bn_max_pool kt={kt}", (t, h, w, c), 2 * n * t * h * w * c * 2, a, b)
    for (t, h, w, c) in [(10, 28, 28, 192), (5, 14, 14, 320)]:
        x, y = (torch.randn(n, t, h, w, c, generator=g).half().to(dev) for _ in range(2))
        for op, fn, k in (("gelu", lambda: F.gelu(x), 2), ("clamp6", lambda: x.clamp(0, 6), 2), ("mul", lambda: x * y, 3),
                          ("add", lambda: x + y, 3), ("add_gelu", lambda: F.gelu(x + y), 3)):
            operands = (x,) if k == 2 else (x, y)
            a, b = timed([lambda: ops.ew(op, *operands), fn])
            row(f"ew {op}", (t, h, w, c), k * x.numel() * 2, a, b)

    say()
    say("## choices")
    for (t, h, w, cfull, lo, ci) in [(10, 28, 28, 192, 128, 64), (5, 14, 14, 320, 224, 96), (5, 14, 14, 320, 96, 224)]:
        x = torch.randn(n, t, h, w, cfull, generator=g).half().to(dev)
        wn = torch.randn(ci, ci, 1, 1, 1, generator=g) / ci ** 0.5
        wf = torch.zeros(ci, cfull, 1, 1, 1)
        wf[:, lo:lo + ci] = wn
        full = ops.ConvLayer(wf, torch.zeros(ci), 1, 0, dtype="fp16", device=dev)
        narrow = ops.ConvLayer(wn, torch.zeros(ci), 1, 0, dtype="fp16", device=dev)
        a, b = timed([lambda: full(x, relu=False), lambda: narrow(x[..., lo:lo + ci].contiguous(), relu=False)])
        say(f"1x1x1 conv on channels [{lo}, {lo + ci}) of {cfull} at {t}x{h}x{w}: zero columns over the full width "
            f"{a * 1e3:.1f} us, slice copy + narrow conv {b * 1e3:.1f} us")
    for (t, h, w, c, kt) in [(10, 28, 28, 64, 1), (5, 14, 14, 160, 3)]:
        x = torch.rand(n, t, h, w, c, generator=g).mul(6).half().to(dev)
        mk = lambda k: ops.DWSepLayer(torch.randn(c, 1, 1, k, k, generator=g) / k, torch.randn(c, 1, kt, 1, 1, generator=g),  # noqa: E731
                                      torch.ones(c), torch.zeros(c), dtype="fp16", device=dev)
        l5, l7 = mk(5), mk(7)
        xn = x.permute(0, 4, 1, 2, 3)
        w5s, w5t, w7s, w7t = (v.permute(1, 0).reshape(c, 1, *s).half() for v, s in
                              ((l5.ws, (1, 5, 5)), (l5.wt if kt == 3 else torch.ones(1, c, device=dev), (kt, 1, 1)),
                               (l7.ws, (1, 7, 7)), (l7.wt if kt == 3 else torch.ones(1, c, device=dev), (kt, 1, 1))))

        def eager():
            t5 = F.conv3d(F.conv3d(xn, w5s, padding=(0, 2, 2), groups=c), w5t, padding=(kt // 2, 0, 0), groups=c).clamp(0, 6)
            t7 = F.conv3d(F.conv3d(xn, w7s, padding=(0, 3, 3), groups=c), w7t, padding=(kt // 2, 0, 0), groups=c).clamp(0, 6)
            return xn + t5 + t7
        a, b = timed([lambda: ops.msca_sum(x, l5, l7), eager])
        moved, floor = 8 * x.numel() * 2, 2 * x.numel() * 2   # a x3, t5 and t7 written and read, the sum written
        say(f"MSCA sum at {t}x{h}x{w}x{c}: three launches {a * 1e3:.1f} us ({moved / a / 1e6:.0f} GB/s over the "
            f"{moved / 1e6:.1f} MB they move; a fused launch would move {floor / 1e6:.1f} MB), eager torch {b * 1e3:.1f} us")

    say()
    say(f"## models, {n} clips of 16 x 112^2 (fp16, SRM_net 'no')")

    def load(cls, make):
        m = cls(1, "no", dtype="fp16")
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in make(0, 1, False).items()})
        return m

    clips = torch.from_numpy(s3d_clips(n, 16, 112, seed=50)).to(dev)

    def graphed(m):
        m(clips)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=s):
                m(clips)
        torch.cuda.current_stream().wait_stream(s)
        return gr.replay

    msca, s3d = load(msca_S3D, make_msca_s3d_state_dict), load(S3D, make_s3d_state_dict)
    sd16 = {k: v.to(dev) for k, v in R.cast_sd(make_msca_s3d_state_dict(0, 1, False), torch.float16).items()}
    a, e, b, c = timed([graphed(msca), lambda: msca(clips), graphed(s3d), lambda: R.forward(sd16, clips, False)], reps=max(5, args.reps // 2))
    say(f"msca_S3D (graph replay)  {a:.2f} ms  {n / a * 1e3:.0f} clips/s   (eager launches: {e:.2f} ms)")
    say(f"S3D      (graph replay)  {b:.2f} ms  {n / b * 1e3:.0f} clips/s")
    say(f"eager torch fp16 restatement of msca_S3D  {c:.2f} ms  {n / c * 1e3:.0f} clips/s  ({c / a:.2f}x msca_S3D)")
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
