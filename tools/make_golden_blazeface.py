"""Generate the BlazeFace fixtures under tests/golden/ from the REFERENCE's own code.

Runs only in the build container (it reads /root/reference, which does not
exist on the GPU box).  ``CViT-main/helpers/blazeface.py`` is imported as is;
``helpers_face_extract_1.py`` imports cv2, which is not in the image, so its
source is parsed, the ``import cv2`` statement dropped, and the rest executed
with a stand-in ``cv2`` whose ``resize(.., INTER_AREA)`` is the exact-integer
area average of ``fac_fake_amd.blazeface.area_resize_np`` (parity of the
tiles with cv2's own INTER_AREA is unpinned, as it is for the crops).
Everything else - the tiling, the network in fp32 and in an fp64 copy,
``predict_on_batch``, ``_resize_detections``, ``_untile_detections``, ``nms``,
``_add_margin_to_detections`` - is the reference's code on PyTorch CPU.

Writes (data only):

  blazeface_weights.npz  the 74 tensors of blazeface.pth + ``anchors``, fp32
  blazeface_golden.npz   per input (video 2x360x640, portrait 640x360, square
                         128x128 with a 64 px face): the paste positions the inputs are rebuilt
                         from, a checksum of the frames and tiles, the fp32
                         reference's tile detections, per-frame NMS output,
                         margin boxes and int boxes, and the decision margins;
                         for the first 5 video tiles the fp64 copy's
                         backbone1 / backbone2 (sampled pixels) and raw r / c
                         (sampled anchors for r), and E_b1, E_b2, E_r, E_c =
                         max|ref_fp32 - ref_fp64| over those tiles.

The paste position of each input is shifted until every decision margin holds
(asserted): score to threshold >= 1e-3, IoU to 0.3 >= 1e-2, gap between
candidate scores >= 1e-4, margin round() argument >= 1e-2 from .5, margin
box coordinates >= 1e-2 from an integer.
"""
from __future__ import annotations

import ast
import copy
import importlib.util
import sys
import types
import zlib
from pathlib import Path

sys.dont_write_bytecode = True
REPO = Path(__file__).resolve().parents[1]
REF = Path("/root/reference/CViT-main/helpers")
OUT = REPO / "tests" / "golden"
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fac_fake_amd import blazeface as bz  # noqa: E402

N_ACT_TILES = 5
B1_PIX = np.arange(0, 256, 4)          # sampled pixels of the 16x16 backbone1 output
B2_PIX = np.arange(0, 64, 2)           # sampled pixels of the 8x8 backbone2 output
R_ROWS = np.concatenate([np.arange(0, 512, 4), np.arange(512, 896, 3)])   # sampled anchors of r


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_blazeface", REF / "blazeface.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    src = REF / "helpers_face_extract_1.py"
    tree = ast.parse(src.read_text(), filename=str(src))
    body = [n for n in tree.body
            if not (isinstance(n, ast.Import) and any(a.name == "cv2" for a in n.names))]

    def resize(img, size, interpolation=None):
        assert size[0] == size[1] and interpolation == 3
        return bz.area_resize_np(np.asarray(img), size[0])

    ns = {"__name__": "ref_face_extract", "cv2": types.SimpleNamespace(resize=resize, INTER_AREA=3)}
    exec(compile(ast.Module(body=body, type_ignores=[]), str(src), "exec"), ns)
    return mod.BlazeFace, ns["FaceExtractor"]


def run_net(net, tiles, dtype):
    """(backbone1, backbone2, r, c) of uint8 tiles [T,128,128,3], activations NHWC."""
    got = {}
    h1 = net.backbone1.register_forward_hook(lambda m, i, o: got.__setitem__("b1", o.detach().clone()))
    h2 = net.backbone2.register_forward_hook(lambda m, i, o: got.__setitem__("b2", o.detach().clone()))
    x = torch.from_numpy(tiles).permute(0, 3, 1, 2).to(dtype) / 127.5 - 1.0
    with torch.no_grad():
        r, c = net(x)
    h1.remove()
    h2.remove()
    return (got["b1"].permute(0, 2, 3, 1).contiguous().numpy(), got["b2"].permute(0, 2, 3, 1).contiguous().numpy(),
            r.numpy(), c.numpy())


def dist_to_half(v):
    return np.abs(np.abs(v - np.floor(v)) - 0.5)


def dist_to_int(v):
    return np.abs(v - np.rint(v))


def reference_flow(net, fx, frames):
    """The FaceExtractor flow (helpers_face_extract_1.py:76-131) on one video."""
    F, H, W, _ = frames.shape
    tiles, info = fx._tile_frames(frames, net.input_size)
    tile_dets = net.predict_on_batch(tiles, apply_nms=False)
    proj = fx._resize_detections(tile_dets, net.input_size, info)
    per_frame = fx._untile_detections(F, (W, H), proj)
    nms = net.nms(per_frame)
    margin = [fx._add_margin_to_detections(d, (W, H), 0.2) for d in nms]
    boxes = []
    for f, m in enumerate(margin):
        for i in range(len(m)):
            ymin, xmin, ymax, xmax = m[i, :4].cpu().numpy().astype(int)   # _crop_faces :314
            boxes.append((f, xmin, ymin, xmax, ymax))
    return dict(tiles=tiles, tile_dets=[d.numpy() for d in tile_dets], per_frame=[d.numpy() for d in per_frame],
                nms=[d.numpy() for d in nms], margin=[d.numpy() for d in margin],
                boxes=np.asarray(boxes, np.int32).reshape(-1, 5))


def margins(net, flow, frames):
    """The decision margins of one input: (score-to-threshold, IoU-to-threshold,
    score gap, round-argument-to-.5, margin-coordinate-to-integer)."""
    H, W = frames.shape[1:3]
    x = torch.from_numpy(flow["tiles"]).permute(0, 3, 1, 2).float() / 127.5 - 1.0
    with torch.no_grad():
        _, c = net(x)
    score = torch.sigmoid(c.clamp(-100, 100)).numpy()
    m_score = float(np.abs(score - net.min_score_thresh).min())
    m_iou = m_gap = m_round = m_int = np.inf
    for d, n in zip(flow["per_frame"], flow["nms"]):
        seen = []
        got, _ = bz.weighted_nms_np(d, net.min_suppression_threshold, ious_seen=seen)
        assert got.shape == n.shape and np.allclose(got, n, rtol=1e-5, atol=1e-3)   # the restatement follows it
        if seen:
            m_iou = min(m_iou, float(np.abs(np.asarray(seen) - net.min_suppression_threshold).min()))
        s = np.sort(d[:, 16].astype(np.float64))
        if len(s) > 1:
            m_gap = min(m_gap, float(np.diff(s).min()))
        if len(n):
            m_round = min(m_round, float(dist_to_half(0.2 * (n[:, 2] - n[:, 0]).astype(np.float64)).min()))
            mg = bz.add_margin_np(n, H, W)[:, :4].astype(np.float64)
            inner = mg[(mg > 0) & (mg != H) & (mg != W)]       # a clamped coordinate is an exact integer by design
            if inner.size:
                m_int = min(m_int, float(dist_to_int(inner).min()))
    return np.asarray([m_score, m_iou, m_gap, m_round, m_int], np.float64)


def margins_ok(m):
    return m[0] >= 1e-3 and m[1] >= 1e-2 and m[2] >= 1e-4 and m[3] >= 1e-2 and m[4] >= 1e-2


PASTE = {"video": [[30, 40], [30, 330]], "portrait": [[60, 120]], "square": [[30, 30]]}


def build_input(name, crops, dy=0, dx=0):
    """A fixture input with its pastes shifted by (dy, dx)."""
    pos = np.asarray(PASTE[name], np.int32) + np.asarray([dy, dx], np.int32)
    return bz.fixture_input(name, crops, pos), pos


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    BlazeFace, FaceExtractor = load_reference()
    net = BlazeFace()
    net.load_weights(str(REF / "blazeface.pth"))
    net.load_anchors(str(REF / "anchors.npy"))
    net64 = copy.deepcopy(net).double()
    fx = FaceExtractor(None, net)

    sd = {k: v.numpy().astype(np.float32) for k, v in net.state_dict().items()}
    assert len(sd) == 74
    np.savez_compressed(OUT / "blazeface_weights.npz", anchors=net.anchors.numpy().astype(np.float32), **sd)

    with np.load(OUT / "golden_real.npz", allow_pickle=False) as z:
        faces = z["crops"]

    out = {}
    shifts = [(0, 0)] + [(dy, dx) for dy in range(0, 8) for dx in range(0, 8) if (dy, dx) != (0, 0)]
    for name in ("video", "portrait", "square"):
        for dy, dx in shifts:
            frames, pos = build_input(name, faces, dy, dx)
            flow = reference_flow(net, fx, frames)
            m = margins(net, flow, frames)
            print(name, (dy, dx), "dets/tile", [len(d) for d in flow["tile_dets"]], "faces/frame",
                  [len(d) for d in flow["nms"]], "margins", m)
            if margins_ok(m):
                break
        else:
            raise AssertionError(f"{name}: no paste position satisfies the margins")
        assert margins_ok(m)
        out[f"{name}_paste"] = pos
        out[f"{name}_frames_crc"] = np.int64(zlib.crc32(frames.tobytes()))
        out[f"{name}_tiles_crc"] = np.int64(zlib.crc32(flow["tiles"].tobytes()))
        out[f"{name}_margins"] = m
        out[f"{name}_tile_counts"] = np.asarray([len(d) for d in flow["tile_dets"]], np.int32)
        out[f"{name}_tile_dets"] = np.concatenate(flow["tile_dets"]).astype(np.float32).reshape(-1, 17)
        out[f"{name}_nms_counts"] = np.asarray([len(d) for d in flow["nms"]], np.int32)
        out[f"{name}_nms"] = np.concatenate(flow["nms"]).astype(np.float32).reshape(-1, 17)
        out[f"{name}_margin"] = np.concatenate(flow["margin"]).astype(np.float32).reshape(-1, 17)
        out[f"{name}_boxes"] = flow["boxes"]
        if name == "video":
            tiles = flow["tiles"][:N_ACT_TILES]
            a32 = run_net(net, tiles, torch.float32)
            a64 = run_net(net64, tiles, torch.float64)
            for key, x32, x64 in zip(("b1", "b2", "r", "c"), a32, a64):
                out[f"E_{key}"] = np.float64(np.abs(x32.astype(np.float64) - x64).max())
                print(f"E_{key}", out[f"E_{key}"], "max|x|", np.abs(x64).max())
            out["b1_pix"], out["b2_pix"], out["r_rows"] = B1_PIX, B2_PIX, R_ROWS
            out["b1_64"] = a64[0].reshape(N_ACT_TILES, 256, 88)[:, B1_PIX]
            out["b2_64"] = a64[1].reshape(N_ACT_TILES, 64, 96)[:, B2_PIX]
            out["r_64"] = a64[2][:, R_ROWS]
            out["c_64"] = a64[3]
            # fp32 raw tensors of all 6 video tiles: the input of the host post-processing test
            r32, c32 = run_net(net, flow["tiles"], torch.float32)[2:]
            keep = np.unique(np.nonzero(c32[..., 0] > 0.0)[1])      # every anchor that can pass a threshold >= 0.5
            out["video_raw_rows"] = keep.astype(np.int32)
            out["video_raw_r"] = r32[:, keep]
            out["video_raw_c"] = c32
    np.savez_compressed(OUT / "blazeface_golden.npz", **out)
    for f in ("blazeface_weights.npz", "blazeface_golden.npz"):
        print(f, (OUT / f).stat().st_size, "bytes")
        assert (OUT / f).stat().st_size < (1 << 20)


if __name__ == "__main__":
    main()
