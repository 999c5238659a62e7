"""Time the GPU BlazeFace detector against the same network in eager torch.

  python tools/bench_blazeface.py [--frames 300 30] [--reps 20] [--out profiles/blazeface_bench.txt]

For each frame count F (1080 x 1920 frames, 3 tiles each: 900 tiles is a
300-frame video searched densely, 90 tiles the 30 frames the reference
schedule reads) it reports medians over ``--reps`` timed calls after warm-up,
all on one GPU in one process:

  tiles       fac_bf_debug_tiles alone (device events), with the traffic floor:
              each 1080^2 window reads 1080 * 1080 * 3 B = 3.5 MB
  net hip     tiles -> backbone -> raw r, c through the HIP kernels (device events)
  net eager   the same network as torch-ROCm eager ops (F.conv2d, fp32, NCHW)
              on the same tiles and weights (device events)
  detect      frames -> int boxes on the host, the whole ``detect_faces`` call
              (host clock around a call that ends in the device->host read)

and the largest difference between the two networks' raw outputs.  There is
no detector in the parent commit, so eager torch is the only baseline.
"""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from fac_fake_amd import blazeface as bz  # noqa: E402
from fac_fake_amd.video import detect_faces  # noqa: E402

WEIGHTS = REPO / "tests" / "golden" / "blazeface_weights.npz"
HBM_BYTES_PER_S = 8e12   # MI355X peak HBM3E bandwidth


class EagerBlazeFace:
    """The reference network as eager torch ops on a state_dict (fp32, NCHW)."""

    def __init__(self, sd):
        self.sd = sd

    def block(self, x, p, stride):
        sd = self.sd
        cin, cout = sd[p + ".convs.0.weight"].shape[0], sd[p + ".convs.1.weight"].shape[0]
        if stride == 2:
            h = F.pad(x, (0, 2, 0, 2))
            x = F.max_pool2d(x, 2, 2)
            h = F.conv2d(h, sd[p + ".convs.0.weight"], sd[p + ".convs.0.bias"], stride=2, groups=cin)
        else:
            h = F.conv2d(x, sd[p + ".convs.0.weight"], sd[p + ".convs.0.bias"], padding=1, groups=cin)
        h = F.conv2d(h, sd[p + ".convs.1.weight"], sd[p + ".convs.1.bias"])
        if cout > cin:
            x = F.pad(x, (0, 0, 0, 0, 0, cout - cin))
        return F.relu(h + x)

    def __call__(self, tiles_u8):
        sd = self.sd
        x = tiles_u8.permute(0, 3, 1, 2).float() / 127.5 - 1.0
        x = F.pad(x, (1, 2, 1, 2))
        x = F.relu(F.conv2d(x, sd["backbone1.0.weight"], sd["backbone1.0.bias"], stride=2))
        for i, (_, _, s) in enumerate(bz.BLOCKS1):
            x = self.block(x, f"backbone1.{i + 2}", s)
        h = x
        for i, (_, _, s) in enumerate(bz.BLOCKS2):
            h = self.block(h, f"backbone2.{i}", s)
        b = x.shape[0]

        def head(name, t, k):
            return F.conv2d(t, sd[name + ".weight"], sd[name + ".bias"]).permute(0, 2, 3, 1).reshape(b, -1, k)
        c = torch.cat((head("classifier_8", x, 1), head("classifier_16", h, 1)), 1)
        r = torch.cat((head("regressor_8", x, 16), head("regressor_16", h, 16)), 1)
        return r, c


def device_ms(fn, reps, warmup):
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


def host_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()            # ends in a device->host read
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out), min(out), max(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, nargs="+", default=[300, 30])
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--out", default=str(REPO / "profiles" / "blazeface_bench.txt"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_blazeface needs a GPU (a CPU run cannot give a time)")
    dev = torch.device("cuda", 0)
    det = bz.BlazeFace().to(dev)
    det.load_weights(WEIGHTS)
    eager = EagerBlazeFace({k: v.to(dev) for k, v in det.state_dict().items()})
    lines = [f"BlazeFace detector, {torch.cuda.get_device_name(0)}, torch {torch.__version__}, fp32; "
             f"median [min .. max] of {args.reps} calls after {args.warmup} warm-up calls"]
    for nf in args.frames:
        g = torch.Generator(device=dev).manual_seed(nf)
        frames = torch.randint(0, 256, (nf, args.height, args.width, 3), dtype=torch.uint8, device=dev, generator=g)
        split, _, n = bz.tile_windows(args.height, args.width)
        T = nf * n
        tiles = det.tiles(frames)
        fmt = lambda t: f"{t[0]:9.3f} ms [{t[1]:.3f} .. {t[2]:.3f}]"  # noqa: E731
        t_tiles = device_ms(lambda: det.tiles(frames), args.reps, args.warmup)
        t_hip = device_ms(lambda: det.debug_net(tiles), args.reps, args.warmup)
        t_det = host_ms(lambda: detect_faces(det, frames), args.reps, args.warmup)
        floor_bytes = T * split * split * 3 + T * 128 * 128 * 3
        lines.append(f"-- {nf} frames of {args.height} x {args.width}: {T} tiles")
        lines.append(f"tiles      {fmt(t_tiles)}   reads {T * split * split * 3 / 1e6:.0f} MB "
                     f"({split * split * 3 / 1e6:.2f} MB per window): floor {floor_bytes / HBM_BYTES_PER_S * 1e3:.3f} ms "
                     f"at 8 TB/s, achieved {floor_bytes / t_tiles[0] / 1e9 * 1e3:.0f} GB/s")
        lines.append(f"net hip    {fmt(t_hip)}   {t_hip[0] / T * 1e3:.2f} us per tile")
        if not args.no_eager:
            with torch.no_grad():
                t_eager = device_ms(lambda: eager(tiles), args.reps, args.warmup)
                r0, c0 = eager(tiles)
            _, _, r1, c1 = det.debug_net(tiles)
            lines.append(f"net eager  {fmt(t_eager)}   {t_eager[0] / T * 1e3:.2f} us per tile; "
                         f"hip / eager = {t_hip[0] / t_eager[0]:.2f}; max|r_hip - r_eager| = "
                         f"{float((r1 - r0).abs().max()):.2e}, max|c_hip - c_eager| = {float((c1 - c0).abs().max()):.2e}")
        lines.append(f"detect     {fmt(t_det)}   frames -> host boxes ({t_det[0] / nf * 1e3:.1f} us per frame)")
        del frames, tiles
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
