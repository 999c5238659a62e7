"""Time the S3D clip staging kernel against the S3D forward it feeds.

  python tools/clip_stage_bench.py [--clips 256] [--reps 20] [--out profiles/clip_stage_bench.txt]

Stages ``--clips`` clips' worth of face boxes (20 per clip) from 1080 x 1920
frames in one ``fac_clip_stage_u8`` launch (fac_fake_amd/clip.py
``stage_clips``: box table on the host, upload, kernel), for three box
populations of ``video.synthetic_video``:

  mixed   square boxes of 112..559 px (about a quarter upscale)
  down    240..559 px: every box takes the area branch
  up      112..223 px: every box takes the bicubic branch

Per variant, medians over ``--reps`` timed calls after warm-up, device events
on one GPU in one process:

  kernel   the launch alone, table already on the device, per clip, with the
           HBM floor of its traffic: every source box read once plus
           3 * 20 * 224 * 224 bytes written per clip, at 8 TB/s
  stage    ``stage_clips`` as called (table + upload + launch), per clip
  forward  fp16 ``S3D(1, "no")`` on the staged clips, ``--batch`` clips per
           call, per clip; and kernel / forward
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

from fac_fake_amd import _lib, clip  # noqa: E402
from fac_fake_amd.s3d import S3D  # noqa: E402
from fac_fake_amd.video import synthetic_video  # noqa: E402
from fac_fake_amd.weights import make_s3d_state_dict  # noqa: E402

HBM_BYTES_PER_S = 8e12   # MI355X peak HBM3E bandwidth
VARIANTS = (("mixed", 112, 448), ("down", 240, 320), ("up", 112, 112))


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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--frames", type=int, default=64, help="distinct 1080p frames the boxes are spread over")
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--batch", type=int, default=32, help="clips per S3D forward")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(REPO / "profiles" / "clip_stage_bench.txt"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("clip_stage_bench needs a GPU (a CPU run cannot give a time)")
    dev = torch.device("cuda", 0)
    T = clip.CLIP_FRAMES
    n = args.clips * T
    per_frame = -(-n // args.frames)
    model = S3D(1, "no", dtype="fp16")
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in make_s3d_state_dict(0, 1, False).items()})
    lib = _lib.load()
    fmt = lambda t, k: f"{t[0] / k * 1e3:9.2f} us [{t[1] / k * 1e3:.2f} .. {t[2] / k * 1e3:.2f}]"  # noqa: E731
    lines = [f"S3D clip staging (fac_clip_stage_u8), {torch.cuda.get_device_name(0)}, torch {torch.__version__}; "
             f"{args.clips} clips x {T} boxes from {args.frames} frames of {args.height} x {args.width}; per clip, "
             f"median [min .. max] of {args.reps} calls after {args.warmup} warm-up calls"]
    for name, box_min, box_span in VARIANTS:
        frames, boxes = synthetic_video(args.frames, args.height, args.width, seed=3, device=dev,
                                        faces_per_frame=per_frame, box_min=box_min, box_span=box_span)
        boxes = boxes[:n]
        table = clip.box_table(boxes, args.height, args.width)
        side = boxes[:, 3] - boxes[:, 1]
        branch = {"copy": int((side == 224).sum()), "area": int((side > 224).sum()), "cubic": int((side < 224).sum())}
        d_table = torch.from_numpy(table).to(dev)
        clips = torch.empty(args.clips, 3, T, clip.CLIP, clip.CLIP, dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream

        def kernel():
            _lib.check(lib.fac_clip_stage_u8(frames.data_ptr(), args.frames, args.height, args.width,
                                             d_table.data_ptr(), n, T, clips.data_ptr(), st), None, "fac_clip_stage_u8")

        t_kernel = device_ms(kernel, args.reps, args.warmup)
        t_stage = device_ms(lambda: clip.stage_clips(frames, boxes, out=clips), args.reps, args.warmup)
        nb = min(args.batch, args.clips)
        with torch.no_grad():
            t_fwd = device_ms(lambda: model(clips[:nb]), args.reps, args.warmup)
        read = int((side.astype(np.int64) ** 2).sum()) * 3
        moved = read + args.clips * 3 * T * clip.CLIP * clip.CLIP
        floor_us = moved / HBM_BYTES_PER_S / args.clips * 1e6
        lines.append(f"-- {name}: box sides {box_min}..{box_min + box_span - 1} px (mean {side.mean():.0f}); "
                     f"{branch['area']} area, {branch['cubic']} cubic, {branch['copy']} copy")
        lines.append(f"kernel   {fmt(t_kernel, args.clips)}   moves {moved / args.clips / 1e6:.2f} MB per clip "
                     f"({read / args.clips / 1e6:.2f} read + {3 * T * clip.CLIP * clip.CLIP / 1e6:.2f} written): "
                     f"floor {floor_us:.2f} us at 8 TB/s, achieved {moved / t_kernel[0] / 1e9 * 1e3:.0f} GB/s")
        lines.append(f"stage    {fmt(t_stage, args.clips)}   box table on the host + upload + launch")
        lines.append(f"forward  {fmt(t_fwd, nb)}   fp16 S3D(1, 'no'), {nb} clips of {T} x 224 x 224 per call; "
                     f"kernel / forward = {t_kernel[0] / args.clips / (t_fwd[0] / nb) * 100:.2f} %")
        del frames, clips
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
