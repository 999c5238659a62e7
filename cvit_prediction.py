"""Video-level entry point: the drop-in for ``CViT-main/cvit_prediction.py``.

The reference script scores every ``.mp4`` of a folder (``predict_on_video``,
cvit_prediction.py:73-83, from ``__main__`` :300-343): per video ``predict``
(:153-242) reads frames with cv2, finds faces with face_recognition, crops /
resizes them (``face_face_rec`` :106-121), runs the CViT on the crops in
chunks of 32 and reduces the per-crop sigmoids to one score
(``pre_process_prediction`` :266-281); the scores go to a ``filename,label``
CSV (:341-343, "label" is the score) and, with a metadata file, an accuracy
(:346-371).

Video decoding (cv2) and the CPU face detectors (dlib HOG / MTCNN) are
outside this path (only the crop/resize is in scope),
so a "video file" here is the decoded video plus its face locations: an
``.npz`` holding

* ``frames``: uint8 [F, H, W, 3], BGR as ``cv2.VideoCapture.read`` returns;
* ``face_locations``: int32 [n, 5] = (frame, top, right, bottom, left), what
  ``face_recognition.face_locations(frame)`` returns per frame, or ``boxes``:
  int32 [n, 5] = (frame, left, top, right, bottom).

With ``--detect`` (``load_detector()``) a file without either list is scored
through the GPU BlazeFace detector (fac_fake_amd/blazeface.py), the
reference's third detector.

From there everything runs on the GPU (fac_fake_amd/video.py): the frame
schedule of :165-198, crop + INTER_AREA + channel swap (``fac_crop_resize_u8``),
the CViT forward with the chunk slots of :224-238, and the score.  The names,
arguments and return values of the reference's functions are kept.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from fac_fake_amd.prediction import (label, non_empty, pre_process_prediction, pred_sig,  # noqa: E402,F401
                                     pred_tensor)
from fac_fake_amd.video import (MAX_CROPS_REFERENCE, crop_faces, predict_video, predict_video_detect,  # noqa: E402
                                score_selected, select_reference)

mean = [0.485, 0.456, 0.406]    # cvit_prediction.py:41 (fused into conv1 here)
std = [0.229, 0.224, 0.225]     # cvit_prediction.py:42
sample = "."                    # folder of videos (cvit_prediction.py:50)
save_csv_path = "./wprediction/cvit.csv"   # :54
model = None                    # set by load_model() (the reference builds it at import, :62-70)
detector = None                 # set by load_detector(): scores videos that carry no face boxes
device = "cuda" if torch.cuda.is_available() else "cpu"


MODEL_NAMES = ("cvit", "cvit_GGCA_ADD_DEConv_RepBn8", "cvit_DEConv", "cvit_GGCA_ADD", "cvit_GGCA_ADD_DEConv",
               "cvit_GGCA_ADD_RepBn", "cvit_GGCA_ADD_DEConv_RepBn", "cvit_GGCA_ADD_DEConv_RepBn3",
               "cvit_GGCA_ADD_DEConv_RepBn4", "cvit_GGCA_ADD_DEConv_RepBn5")   # the reference's model/<name>.py


def model_class(name: str | None = None):
    """The drop-in ``CViT`` class of ``model/<name>.py``; None is the base ``cvit``."""
    if name in (None, "cvit"):
        from fac_fake_amd.cvit import CViT
        return CViT
    # weights.CVIT_FAMILY's names; cvit_GGCA_ADD_DConv and the model/other/ ones
    # are not --model choices: see INTEGRATION.md
    from fac_fake_amd.variants import variant_class
    return variant_class(name)


def _synthetic_state_dict(name: str | None):
    from fac_fake_amd import weights as W
    if name in (None, "cvit"):
        return W.make_state_dict(0)
    return W.make_family_state_dict(name, 0)


def load_model(weights: str | None = None, dtype: str = "fp16", dev: str | None = None, name: str | None = None):
    """``CViT(224, 7, 2, 512, 1024, 6, 8, 2048)`` + ``load_state_dict`` + ``eval``
    (cvit_prediction.py:62-70).  ``weights``: a state_dict checkpoint as
    ``cvit_train.py:210`` saves it (loaded with ``weights_only=True``), or
    None for the deterministic synthetic weights (the reference ships no
    trained checkpoint).  ``name``: which ``model/<name>.py`` class the
    checkpoint belongs to (the reference edits its `from cvit import CViT` line, :23);
    None is the base ``cvit``."""
    global model
    m = model_class(name)(image_size=224, patch_size=7, num_classes=2, channels=512, dim=1024, depth=6, heads=8,
                          mlp_dim=2048, dtype=dtype)
    if weights:
        sd = torch.load(weights, map_location="cpu", weights_only=True)
    else:
        sd = {k: torch.from_numpy(np.asarray(v)) for k, v in _synthetic_state_dict(name).items()}
    m.load_state_dict(sd)
    m.to(dev or device)
    m.eval()
    model = m
    return m


DETECTOR_WEIGHTS = Path(__file__).resolve().parent / "tests" / "golden" / "blazeface_weights.npz"


def load_detector(weights: str | None = None, anchors: str | None = None, dev: str | None = None):
    """``BlazeFace()`` + ``load_weights`` + ``load_anchors`` as the reference's
    ``FaceExtractor`` users set it up.  ``weights``: ``blazeface.pth``,
    ``anchors``: ``anchors.npy``; None for either takes the reference's trained
    weights / anchors shipped as tests/golden/blazeface_weights.npz."""
    global detector
    from fac_fake_amd.blazeface import BlazeFace
    d = BlazeFace().to(dev or device)
    d.load_weights(weights or DETECTOR_WEIGHTS)
    d.load_anchors(anchors or DETECTOR_WEIGHTS)      # the shipped anchors are the reference's anchors.npy
    detector = d
    return d


def read_video(filename: str):
    """The decoded video container: (frames uint8 [F,H,W,3] BGR, boxes int32
    [n,5] as (frame, left, top, right, bottom)); boxes is None for a file with
    neither ``boxes`` nor ``face_locations`` when a detector is loaded."""
    with np.load(filename, allow_pickle=False) as z:
        frames = z["frames"]
        if "boxes" in z:
            boxes = z["boxes"].astype(np.int32).reshape(-1, 5)
        elif "face_locations" not in z and detector is not None:
            boxes = None
        else:
            fl = z["face_locations"].astype(np.int32).reshape(-1, 5)    # frame, top, right, bottom, left
            boxes = np.stack([fl[:, 0], fl[:, 4], fl[:, 1], fl[:, 2], fl[:, 3]], 1).astype(np.int32)
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[3] != 3:
        raise ValueError(f"{filename}: frames must be uint8 [F,H,W,3], got {frames.dtype} {frames.shape}")
    return frames, boxes


def face_face_rec(frame, face_locations):
    """Crops of one frame (cvit_prediction.py:106-121): the first 5 face
    locations (top, right, bottom, left), ``frame[top:bottom, left:right]``
    -> INTER_AREA 224x224 -> channel swap, as uint8 [n,224,224,3] (on the
    GPU), or ``([], 0)`` when there is no face."""
    locs = list(face_locations)[:5]
    if not locs:
        return [], 0
    fr = torch.as_tensor(np.ascontiguousarray(frame)).to(device).unsqueeze(0)
    boxes = np.array([[0, l, t, r, b] for (t, r, b, l) in locs], np.int32)
    return crop_faces(fr, boxes), len(locs)


def predict(filename, mtcnn=None, mode: str = "reference"):
    """Score of one video, a float (< 0.5 REAL, >= 0.5 FAKE), as
    cvit_prediction.py:153-242 returns it; 0.5 when no face is found.
    ``mtcnn`` is accepted for signature compatibility and unused, as in the
    reference's live path (:180-187 is commented out)."""
    if model is None:
        raise RuntimeError("call load_model() first (the reference builds its model at import)")
    frames, boxes = read_video(filename)
    if boxes is None:
        return predict_video_detect(model, detector, frames, mode=mode)
    # host frames: predict_video uploads only the frames its crops come from
    return predict_video(model, frames, boxes, mode=mode)


def predict_on_video(dfdc_filenames, num_workers, batch: int = 256):
    """Scores of the videos ``sample/<filename>`` in order (:73-83).

    The reference maps ``predict`` over a ``ThreadPoolExecutor(num_workers)``
    (one worker, :303), i.e. one <= 29-crop forward per video.  Here the
    ``num_workers`` threads only read the files and keep each video's crop
    selection and the frames it needs (``select_reference``); the GPU work
    stays on the calling thread, which scores the crops of consecutive videos
    together in forwards of up to ``batch`` crops (``score_selected``: each
    video keeps its own slots 0..n-1, one segmented score launch per group).
    Every score is bit-identical to ``predict`` on that video alone."""
    if model is None:
        raise RuntimeError("call load_model() first (the reference builds its model at import)")

    def load(i):
        frames, boxes = read_video(os.path.join(sample, dfdc_filenames[i]))
        if boxes is None:   # no boxes in the file: found by the detector, on the calling thread
            return frames, None
        return select_reference(frames, boxes)

    # read-ahead is bounded: at most num_workers + 1 loaded videos wait for
    # the GPU (each holds its selected host frames, ~190 MB at 1080p; the
    # reference's threads only ever hold float scores)
    from collections import deque
    workers = max(1, int(num_workers))
    n = len(dfdc_filenames)

    def items(ex):
        pending, nxt = deque(), 0
        while nxt < n or pending:
            while nxt < n and len(pending) < workers + 1:
                pending.append(ex.submit(load, nxt))
                nxt += 1
            yield pending.popleft().result()

    predictions, group, ncrops = [], [], 0
    with ThreadPoolExecutor(max_workers=workers) as ex:
        for item in items(ex):
            if item[1] is None:
                item = select_reference(item[0], _detect_reference(item[0]))
            if group and ncrops + len(item[1]) > batch:
                predictions += score_selected(model, group, batch)
                group, ncrops = [], 0
            group.append(item)
            ncrops += len(item[1])
        if group:
            predictions += score_selected(model, group, batch)
    return predictions


def _detect_reference(frames) -> np.ndarray:
    """The detector's boxes on the frames the reference schedule reads."""
    from fac_fake_amd.video import detect_faces, frame_indices
    ids = sorted(set(frame_indices(int(frames.shape[0]))))
    if not ids:
        return np.zeros((0, 5), np.int32)
    sub = torch.as_tensor(np.ascontiguousarray(np.asarray(frames)[ids])).to(device)
    boxes = detect_faces(detector, sub)
    boxes[:, 0] = np.asarray(ids, np.int32)[boxes[:, 0]]
    return boxes


def real_or_fake(filenames, predictions):
    """Per-video labels, REAL if the score < 0.5 else FAKE (:289-296)."""
    return [label(float(p)) for p in predictions]


def write_predictions(filenames, predictions, path=None):
    """``pd.DataFrame({"filename": ..., "label": ...}).to_csv(path, index=False)``
    (:341-343): a header line, then ``filename,score`` rows, floats in
    Python's shortest round-trip form as pandas writes them."""
    path = Path(path or save_csv_path)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(["filename", "label"])
        for fn, p in zip(filenames, predictions):
            w.writerow([fn, repr(float(p))])
    return path


def prediction_accuracy(csv_path, metadata) -> float:
    """:346-371: a score < 0.5 counts as 1, else 0, compared with
    ``metadata[filename]``; returns the fraction correct."""
    data = json.loads(Path(metadata).read_text()) if isinstance(metadata, (str, Path)) else metadata
    rows = list(csv.DictReader(open(csv_path)))
    score = 0
    for r in rows:
        pred = 1 if float(r["label"]) < 0.5 else 0
        if pred == data[r["filename"]]:
            score += 1
    return score / len(rows) if rows else 0.0


def main(argv=None):
    global sample, save_csv_path
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sample", default=sample, help="folder of decoded videos (.npz)")
    ap.add_argument("--csv", default=save_csv_path)
    ap.add_argument("--weights", default=None, help="CViT state_dict checkpoint (default: synthetic weights)")
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--model", default="cvit", choices=MODEL_NAMES,
                    help="the reference's model/<name>.py class the weights belong to (default: the base cvit)")
    ap.add_argument("--metadata", default=None, help="json {filename: 0/1} for the accuracy")
    ap.add_argument("--num-workers", type=int, default=1)
    ap.add_argument("--detect", action="store_true",
                    help="find the faces of videos that carry no boxes with the GPU BlazeFace detector")
    ap.add_argument("--detector-weights", default=None, help="blazeface.pth (default: the shipped trained weights)")
    ap.add_argument("--detector-anchors", default=None, help="anchors.npy (with --detector-weights)")
    args = ap.parse_args(argv)
    sample, save_csv_path = args.sample, args.csv
    load_model(args.weights, args.dtype, name=args.model)
    if args.detect:
        load_detector(args.detector_weights, args.detector_anchors)
    filenames = sorted(x for x in os.listdir(sample) if x.endswith(".npz"))
    predictions = predict_on_video(filenames, num_workers=args.num_workers)
    print(predictions)
    for fn, lb in zip(filenames, real_or_fake(filenames, predictions)):
        print("Filname:", fn, lb)
    write_predictions(filenames, predictions, save_csv_path)
    if args.metadata:
        print(f"prediction Acc:  {prediction_accuracy(save_csv_path, args.metadata) * 100}%")
    return predictions


__all__ = ["MAX_CROPS_REFERENCE", "MODEL_NAMES", "face_face_rec", "load_detector", "load_model", "model_class", "non_empty", "pre_process_prediction", "pred_sig",
           "pred_tensor", "predict", "predict_on_video", "prediction_accuracy", "read_video", "real_or_fake",
           "write_predictions"]

if __name__ == "__main__":
    main()
