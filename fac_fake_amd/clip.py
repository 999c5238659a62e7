"""One decoded video through face boxes -> clip -> S3D / CA_S3D_v3 / msca_S3D score.

The S3D harness builds a model's input clip on the CPU in three steps, and
``s3d.video_predictions`` starts after them.  This module is those steps:

* crop: ``preprocessing/extract_crops.py:51-71`` pads each face box to a
  square (``int((long - short) / 2)`` on both sides of the short axis) and
  slices the frame, which clips the box (``square_boxes``, host numpy);
* select: ``S3D/S3D-test.py:165-191`` keeps face 0 of every frame that has
  one, skips a video with fewer than 200 such frames, and takes every 10th of
  the first 200: 20 frames (``clip_schedule``);
* resize: each crop through ``IsotropicResize(224, INTER_AREA down /
  INTER_CUBIC up)`` and ``PadIfNeeded(224, 224, BORDER_CONSTANT)``
  (``S3D-test.py:65-73``, ``transforms/albu.py:9-26``), the 20 BGR frames
  stacked into ``[1, 3, 20, 224, 224]`` (``S3D-test.py:94-96``): one
  ``fac_clip_stage_u8`` launch for every box of every clip
  (``stage_clips``, fac_fake_amd/csrc/clip.hip), uint8 straight into the
  layout ``S3D._pack`` reads.  The output size of each box comes from the host
  in float64, as ``isotropically_resize_image`` computes it (``box_table``).

``create_base_transform`` also holds ``ImageCompression`` and ``GaussNoise``:
those are the harness's robustness degradations of its test images (random
JPEG quality and noise), not staging, and are left out.  Parity with cv2's
own resize is unpinned (clip.hip's header).

``predict_clip_video`` / ``predict_clip_video_detect`` go from frames (and
boxes, or the BlazeFace detector's) to the harness's video score.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .video import _work_device, detect_faces

CLIP = 224
CLIP_FRAMES = 20             # 200 // 10 (S3D-test.py:185-187)
SCHEDULE_FIRST, SCHEDULE_STEP = 200, 10


def square_boxes(boxes, H: int, W: int) -> np.ndarray:
    """extract_crops.py:52-69 on int boxes [n, 5] = (frame, left, top, right,
    bottom) of H x W frames: the short side grows by ``int((long - short) / 2)``
    at both ends, the start is clamped at 0 and the end by the frame, as the
    numpy slice ``frame[max(ymin - p_h, 0):ymax + p_h, max(xmin - p_w, 0):xmax
    + p_w]`` does.  (A box that ends left of or above the frame becomes empty;
    numpy would count a negative end from the far edge.)  Returns int32 [n, 5]."""
    b = np.asarray(boxes, dtype=np.int64).reshape(-1, 5)
    w, h = b[:, 3] - b[:, 1], b[:, 4] - b[:, 2]
    p_w = np.where(h > w, (h - w) // 2, 0)
    p_h = np.where(h < w, (w - h) // 2, 0)
    out = np.empty_like(b)
    out[:, 0] = b[:, 0]
    out[:, 1] = np.maximum(b[:, 1] - p_w, 0)
    out[:, 2] = np.maximum(b[:, 2] - p_h, 0)
    out[:, 3] = np.clip(b[:, 3] + p_w, 0, W)
    out[:, 4] = np.clip(b[:, 4] + p_h, 0, H)
    return out.astype(np.int32)


def clip_schedule(face_frames, first: int = SCHEDULE_FIRST, step: int = SCHEDULE_STEP):
    """The frames of the harness's snippet (S3D-test.py:183-189): of the
    ordered indices of the frames that have a face 0, every ``step``-th of the
    first ``first``; ``None`` when there are fewer than ``first`` (the harness
    skips such a video)."""
    ff = np.asarray(face_frames, dtype=np.int64).reshape(-1)
    if len(ff) < first:
        return None
    return ff[:first:step]


def box_table(boxes, H: int, W: int) -> np.ndarray:
    """Rows of ``fac_clip_stage_u8``: boxes [n, 5] -> int32 [n, 7] = (frame,
    left, top, right, bottom, ow, oh) with ow x oh the size
    ``isotropically_resize_image(crop, 224)`` resizes the clipped box to
    (albu.py:10-25, float64): w x h when max(w, h) == 224; else w > h gives
    (224, int(h * (224 / w))), otherwise (int(w * (224 / h)), 224).  An empty
    box has ow = oh = 0."""
    b = np.asarray(boxes, dtype=np.int64).reshape(-1, 5)
    w = np.minimum(b[:, 3], W) - np.maximum(b[:, 1], 0)
    h = np.minimum(b[:, 4], H) - np.maximum(b[:, 2], 0)
    live = (w > 0) & (h > 0)
    wf, hf = np.where(live, w, 1).astype(np.float64), np.where(live, h, 1).astype(np.float64)
    wide = w > h
    scale = float(CLIP) / np.where(wide, wf, hf)
    ow = np.where(wide, CLIP, (wf * scale).astype(np.int64))       # int(): truncation
    oh = np.where(wide, (hf * scale).astype(np.int64), CLIP)
    same = np.maximum(w, h) == CLIP
    ow, oh = np.where(same, w, ow), np.where(same, h, oh)
    t = np.empty((len(b), 7), np.int32)
    t[:, :5] = b
    t[:, 5] = np.where(live, ow, 0)
    t[:, 6] = np.where(live, oh, 0)
    return t


def stage_clips(frames: torch.Tensor, boxes, T: int = CLIP_FRAMES, out: torch.Tensor | None = None) -> torch.Tensor:
    """uint8 BGR frames [F, H, W, 3] (device) + boxes [n, 5] (frame, left,
    top, right, bottom), n a multiple of T -> uint8 BGR clips
    [n / T, 3, T, 224, 224] (device): box i is frame i % T of clip i // T, each
    resized as IsotropicResize does and zero-padded to 224 x 224.  Written into
    ``out`` when given (a contiguous [n / T, 3, T, 224, 224] uint8 tensor on the
    frames' device, e.g. a slice of a batch that several videos fill)."""
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda or frames.dtype != torch.uint8 \
            or frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError("frames must be a uint8 [F, H, W, 3] device tensor")
    b = np.asarray(boxes)
    if b.size and (b.ndim != 2 or b.shape[1] != 5):
        raise ValueError(f"boxes must be [n, 5] (frame, left, top, right, bottom), got {b.shape}")
    b = b.reshape(-1, 5)
    n = len(b)
    if int(T) != T or T <= 0 or n % T:
        raise ValueError(f"{n} boxes do not fill clips of T = {T} frames")
    shape = (n // T, 3, T, CLIP, CLIP)
    if out is None:
        clips = torch.empty(shape, dtype=torch.uint8, device=frames.device)
    else:
        if (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != shape
                or not out.is_contiguous() or out.device != frames.device):
            raise ValueError(f"out must be a contiguous uint8 {list(shape)} tensor on {frames.device}")
        clips = out
    if n:
        if frames.shape[0] * frames.shape[1] * frames.shape[2] < 2:
            raise ValueError(f"frames {tuple(frames.shape)} hold under two pixels")
        frames = frames.contiguous()
        F, H, W, _ = frames.shape
        table = torch.from_numpy(box_table(b, H, W)).to(frames.device)
        _lib.check(_lib.load().fac_clip_stage_u8(frames.data_ptr(), F, H, W, table.data_ptr(), n, int(T),
                                                 clips.data_ptr(),
                                                 torch.cuda.current_stream(frames.device).cuda_stream),
                   None, "fac_clip_stage_u8")
    return clips


def first_faces(boxes) -> np.ndarray:
    """Face 0 of every frame that has a face: the first row of each frame in
    list order, frames ascending (S3D-test.py:166-177 sorts the crop files by
    frame and keeps the ``_0`` ones).  int32 [m, 5]."""
    b = np.asarray(boxes, dtype=np.int32).reshape(-1, 5)
    _, idx = np.unique(b[:, 0], return_index=True)
    return b[idx]


def predict_clip_video(model, frames, boxes, return_probs: bool = False, *, first: int = SCHEDULE_FIRST,
                       step: int = SCHEDULE_STEP):
    """The harness's score of one video (S3D-test.py:165-191,260-286) for a
    ``fac_fake_amd`` S3D, CA_S3D_v3 or msca_S3D ``model`` (either SRM setting).

    ``frames``: the decoded video, uint8 BGR [F, H, W, 3], a device tensor or a
    host array / CPU tensor (only the snippet's frames are then uploaded);
    ``boxes``: [n, 5] (frame, left, top, right, bottom), face boxes in frame
    pixels, a frame's face 0 first.  Face 0 of each frame -> ``clip_schedule``
    -> ``square_boxes`` -> ``stage_clips`` -> the model; the score is
    ``s3d.video_predictions``' rule for one snippet: element [0] of the
    sigmoid of the model's output row.  Returns ``None`` for a video the
    harness skips (fewer than ``first`` frames with a face); with
    ``return_probs`` also the model's [1, num_class] probabilities."""
    faces = first_faces(boxes)
    ids = clip_schedule(faces[:, 0], first, step)
    if ids is None:
        return (None, None) if return_probs else None
    sel = faces[np.searchsorted(faces[:, 0], ids)]
    H, W = int(frames.shape[1]), int(frames.shape[2])
    sel = square_boxes(sel, H, W)
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda):
        host = frames.numpy() if isinstance(frames, torch.Tensor) else np.asarray(frames)
        inside = (sel[:, 0] >= 0) & (sel[:, 0] < len(host))
        fr = np.ascontiguousarray(host[np.where(inside, sel[:, 0], 0)])
        frames = torch.from_numpy(fr).to(_work_device(frames))
        sel[:, 0] = np.where(inside, np.arange(len(sel)), -1)
    clip = stage_clips(frames, sel, T=len(sel))
    with torch.no_grad():
        _, probs = model(clip, return_probs=True)
    score = float(probs.double().cpu()[0][0])
    return (score, probs) if return_probs else score


def predict_clip_video_detect(model, detector, frames, chunk: int = 64, return_probs: bool = False, *,
                              first: int = SCHEDULE_FIRST, step: int = SCHEDULE_STEP):
    """``predict_clip_video`` on the boxes ``video.detect_faces`` finds: frames
    -> score with no box list from outside.  The video is searched ``chunk``
    frames at a time and the search stops once ``first`` frames with a face
    are found (the snippet reads nothing beyond them) or the video ends."""
    if chunk <= 0:
        raise ValueError("chunk must be positive")
    F = int(frames.shape[0])
    found, rows = 0, []
    for f0 in range(0, F, chunk):
        part = frames[f0:f0 + chunk]
        if not (isinstance(part, torch.Tensor) and part.is_cuda):
            part = torch.as_tensor(np.ascontiguousarray(np.asarray(part))).to(_work_device(frames))
        b = detect_faces(detector, part)
        b[:, 0] += f0
        rows.append(b)
        found += len(np.unique(b[:, 0]))
        if found >= first:
            break
    boxes = np.concatenate(rows) if rows else np.zeros((0, 5), np.int32)
    return predict_clip_video(model, frames, boxes, return_probs, first=first, step=step)


__all__ = ["CLIP", "CLIP_FRAMES", "box_table", "clip_schedule", "first_faces", "predict_clip_video",
           "predict_clip_video_detect", "square_boxes", "stage_clips"]
