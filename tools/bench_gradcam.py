"""Time Grad-CAM (fac_fake_amd/gradcam.py) against the plain forward.

  python tools/bench_gradcam.py [--reps 30] [--out profiles/gradcam_bench.txt]

One GPU, one process, device events, medians over ``--reps`` calls after
warm-up; the variants of one shape alternate inside each repetition.  For
both models (fp16) at B = 1 and B = 32 uint8 crops:

  forward   model.forward_u8 (the base CViT replays its captured graph)
  compute   GradCAM.compute: conv stack with the last conv run twice,
            recording tail forward, backward to the 14x14 map, CAM kernel
  fwd half  the same without the backward and the CAM (gradcam_features +
            fac_forward_features): compute - fwd half is the backward's cost,
            its share is that over compute
  dgrad     the backward's 38 dgrad GEMMs alone on the context-free entry
            point, with the tail's shapes (M = 2B rows; B for the head and the
            patch embedding): the tail's 78.1 M 16-bit weights are each needed
            once, 156 MB, and "weight GB/s" is that over the time.  The kernel
            re-reads a weight tile once per 8 rows of dY (from L2 / Infinity
            Cache), so at B = 32 the traffic it generates is up to 8x that.

There is no speed bar: the path is new and the parent commit has nothing to
compare it with.
"""
from __future__ import annotations

import argparse
import statistics
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

# (rows: 2 = 2B, 1 = B; N; K; count) of the backward's dgrad GEMMs
DGRADS = [(1, 2048, 1024, 1), (2, 1024, 2048, 6), (2, 2048, 1024, 6), (2, 1024, 1024, 6), (2, 3072, 1024, 6),
          (1, 1024, 25088, 1)]
WEIGHTS = sum(n * k * c for _, n, k, c in DGRADS)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="commit id to name in the report (default: git rev-parse)")
    args = ap.parse_args()

    import numpy as np
    import torch

    from fac_fake_amd import _lib
    from fac_fake_amd import cvit as cvit_mod
    from fac_fake_amd import repbn8 as repbn8_mod
    from fac_fake_amd.gradcam import GradCAM
    from fac_fake_amd.weights import make_crops, make_repbn8_state_dict, make_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("bench_gradcam needs a GPU (there is no CPU fallback)")
    lib = _lib.load()
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

    commit = args.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", str(REPO), "rev-parse", "--short", "HEAD"], capture_output=True,
                                    text=True).stdout.strip() or "unknown"
        except OSError:
            commit = "unknown"
    say(f"device: {torch.cuda.get_device_name(0)}; parent commit {commit} + this change; fp16; medians of {args.reps} "
        f"after 3 warm-up calls; device events")
    say(f"dgrad weights: {WEIGHTS / 1e6:.1f} M x 2 B = {WEIGHTS * 2 / 1e6:.0f} MB per Grad-CAM call")
    st = torch.cuda.current_stream().cuda_stream
    for name, mod, make in (("cvit", cvit_mod, make_state_dict), ("repbn8", repbn8_mod, make_repbn8_state_dict)):
        m = mod.CViT(dtype="fp16")
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in make(0).items()})
        m.to("cuda")
        cam = GradCAM(m)
        for B in (1, 32):
            x = torch.from_numpy(make_crops(B, seed=3)).cuda()
            pidx = torch.arange(B, dtype=torch.int32, device="cuda")
            logits = torch.empty(B, 2, device="cuda")

            def fwd_half():
                a, feat = m.gradcam_features(x, True)
                tin = m.weighted_features16(feat) if name == "repbn8" else feat
                _lib.check(lib.fac_forward_features(m._ctx, tin.data_ptr(), B, pidx.data_ptr(), None,
                                                    logits.data_ptr(), None, st), m._ctx, "fac_forward_features")

            # the dgrad GEMMs alone, on buffers of the tail's shapes
            bufs = []
            for rows, n, k, cnt in DGRADS:
                M = rows * B
                w = (torch.randn(n, k, device="cuda") * 0.02).half()
                dy = torch.randn(M, n, device="cuda") * 1e-3
                scr = torch.empty(lib.fac_gradcam_dgrad_scratch_floats(M, n, k), device="cuda")
                dx = torch.empty(M, k, device="cuda")
                bufs.append((M, n, k, cnt, w, dy, scr, dx))

            def dgrads():
                for M, n, k, cnt, w, dy, scr, dx in bufs:
                    for _ in range(cnt):
                        _lib.check(lib.fac_gradcam_dgrad(1, dy.data_ptr(), n, w.data_ptr(), scr.data_ptr(), dx.data_ptr(),
                                                         M, n, k, st), None, "fac_gradcam_dgrad")

            t_fwd, t_cam, t_half, t_dg = timed([lambda: m.forward_u8(x), lambda: cam.compute(x, 0), fwd_half, dgrads],
                                               args.reps)
            say(f"  {name:>6} B={B:>2}: forward {t_fwd:7.3f} ms  compute {t_cam:7.3f} ms ({t_cam / t_fwd:5.2f}x)  fwd half "
                f"{t_half:7.3f} ms  backward + CAM {t_cam - t_half:7.3f} ms ({(t_cam - t_half) / t_cam * 100:4.1f} %)  "
                f"dgrad GEMMs {t_dg:7.3f} ms = {WEIGHTS * 2 / t_dg / 1e6:7.1f} weight GB/s")
            del bufs
        del cam, m
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
