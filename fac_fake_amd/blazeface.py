"""BlazeFace face detector on the GPU: the drop-in for ``CViT-main/helpers/blazeface.py``
and the tile / untile / NMS / margin flow of ``helpers_face_extract_1.py:76-131,139-299``.

The network (5x5 stem, 16 BlazeBlocks, two classifier / regressor heads, 896
anchors) and everything around it run in fp32 HIP kernels
(fac_fake_amd/csrc/blazeface.hip): window cut + area resize to 128x128, the
net, decode + threshold + order-preserving compaction, and one workgroup per
frame for untile -> sort -> weighted NMS -> margin -> int boxes.  There is no
CPU fallback: a call without a GPU raises.

The ``*_np`` functions are float32 / exact-integer numpy restatements of the
same arithmetic (tests and tools/make_golden_blazeface.py compare against
them); they are not used by the GPU path.
"""
from __future__ import annotations

import ctypes
import threading

import numpy as np
import torch
from torch import nn

from . import _lib
from .cvit import weight_versions

TILE = 128                 # BlazeFace.input_size
NUM_ANCHORS = 896
MARGIN = 0.2               # helpers_face_extract_1.py:114
CAPACITY = 1024            # NMS candidates kept per frame (fac_bf_capacity())

# (cin, cout, stride) of backbone1.2 .. backbone1.12 and backbone2.0 .. backbone2.4
BLOCKS1 = [(24, 24, 1), (24, 28, 1), (28, 32, 2), (32, 36, 1), (36, 42, 1), (42, 48, 2), (48, 56, 1), (56, 64, 1),
           (64, 72, 1), (72, 80, 1), (80, 88, 1)]
BLOCKS2 = [(88, 96, 2), (96, 96, 1), (96, 96, 1), (96, 96, 1), (96, 96, 1)]


# ----------------------------------------------------------------- windows
def tile_windows(H: int, W: int):
    """The reference's windows of an H x W frame (``_tile_frames``): side
    ``split = min(H, W)``, 3 windows ``x_step = (W - split) // 2`` apart if the
    frame is landscape, else 1, all at y = 0.  Returns (split, x_step, n)."""
    split = min(H, W)
    return split, (W - split) // 2, (3 if W > H else 1)


def _overlap(n: int, out: int) -> np.ndarray:
    """R[o, s]: overlap, in 1/out pixel, of output pixel o's interval with source pixel s."""
    o = np.arange(out, dtype=np.int64)[:, None]
    s = np.arange(n, dtype=np.int64)[None, :]
    return np.maximum(np.minimum((o + 1) * n, (s + 1) * out) - np.maximum(o * n, s * out), 0)


def area_resize_np(src: np.ndarray, out: int = TILE) -> np.ndarray:
    """uint8 [n, n, 3] -> uint8 [out, out, 3]: area average in exact integers,
    round half up (the arithmetic of crop.hip's area branch, no channel swap)."""
    ny, nx = src.shape[:2]
    if ny < out or nx < out:
        raise ValueError("area_resize_np only shrinks")
    ry, rx = _overlap(ny, out), _overlap(nx, out)
    den = nx * ny
    s = src.astype(np.int64)
    res = np.empty((out, out, 3), np.uint8)
    for c in range(3):
        num = ry @ s[:, :, c] @ rx.T
        res[:, :, c] = ((2 * num + den) // (2 * den)).astype(np.uint8)
    return res


def tile_frames_np(frames: np.ndarray) -> np.ndarray:
    """uint8 [F, H, W, 3] -> uint8 [F * n, 128, 128, 3], frame-major, windows left to right."""
    F, H, W, _ = frames.shape
    split, x_step, n = tile_windows(H, W)
    out = np.empty((F * n, TILE, TILE, 3), np.uint8)
    for f in range(F):
        for h in range(n):
            out[f * n + h] = area_resize_np(frames[f, :split, h * x_step:h * x_step + split])
    return out


# ------------------------------------------------------ float32 post-processing
_f32 = np.float32


def decode_np(raw_r: np.ndarray, raw_c: np.ndarray, anchors: np.ndarray, min_score: float = 0.75):
    """``_tensors_to_detections`` in float32: raw [T, 896, 16], [T, 896, 1] ->
    (list of [n, 17] arrays in anchor order, scores [T, 896])."""
    r = np.asarray(raw_r, _f32)
    a = np.asarray(anchors, _f32)
    d = np.empty(r.shape[:2] + (17,), _f32)
    xc = r[..., 0] / _f32(128) * a[:, 2] + a[:, 0]
    yc = r[..., 1] / _f32(128) * a[:, 3] + a[:, 1]
    w = r[..., 2] / _f32(128) * a[:, 2]
    h = r[..., 3] / _f32(128) * a[:, 3]
    d[..., 0] = yc - h / _f32(2)
    d[..., 1] = xc - w / _f32(2)
    d[..., 2] = yc + h / _f32(2)
    d[..., 3] = xc + w / _f32(2)
    for k in range(6):
        o = 4 + 2 * k
        d[..., o] = r[..., o] / _f32(128) * a[:, 2] + a[:, 0]
        d[..., o + 1] = r[..., o + 1] / _f32(128) * a[:, 3] + a[:, 1]
    s = np.clip(np.asarray(raw_c, _f32)[..., 0], _f32(-100), _f32(100))
    score = (_f32(1) / (_f32(1) + np.exp(-s, dtype=_f32))).astype(_f32)
    d[..., 16] = score
    return [d[t][score[t] >= _f32(min_score)] for t in range(r.shape[0])], score


def untile_np(tile_dets, H: int, W: int):
    """``_resize_detections`` + ``_untile_detections`` in float32: per-tile
    [n, 17] lists (normalised) -> per-frame [n, 17] in frame pixels."""
    split, x_step, n = tile_windows(H, W)
    scale = _f32(split / TILE)
    frames = []
    for f in range(len(tile_dets) // n):
        parts = []
        for h in range(n):
            d = np.array(tile_dets[f * n + h], _f32).reshape(-1, 17)
            d[:, :16] = d[:, :16] * _f32(TILE) * scale
            xoff = _f32(h * x_step)
            d[:, 1:4:2] += xoff          # boxes are (y, x, y, x)
            d[:, 4:16:2] += xoff         # keypoints are (x, y)
            parts.append(d)
        frames.append(np.concatenate(parts) if parts else np.zeros((0, 17), _f32))
    return frames


def _iou_np(box, others):
    iy = np.maximum(np.minimum(box[2], others[:, 2]) - np.maximum(box[0], others[:, 0]), _f32(0))
    ix = np.maximum(np.minimum(box[3], others[:, 3]) - np.maximum(box[1], others[:, 1]), _f32(0))
    inter = (iy * ix).astype(_f32)
    area_a = _f32((box[2] - box[0]) * (box[3] - box[1]))
    area_b = ((others[:, 2] - others[:, 0]) * (others[:, 3] - others[:, 1])).astype(_f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (inter / (area_a + area_b - inter)).astype(_f32)


def weighted_nms_np(dets: np.ndarray, min_iou: float = 0.3, capacity: int = CAPACITY, ious_seen: list | None = None):
    """``_weighted_non_max_suppression`` in float32 on one frame's [n, 17]:
    candidates sorted by score descending (ties: first in the list first), the
    best ``capacity`` kept, then the blending loop with every sum taken in
    sorted order.  Returns ([m, 17], overflow count).  ``ious_seen`` collects
    every IoU that was compared with the threshold."""
    d = np.asarray(dets, _f32).reshape(-1, 17)
    order = np.argsort(-d[:, 16], kind="stable")
    overflow = max(len(order) - capacity, 0)
    d = d[order[:capacity]]
    alive = np.ones(len(d), bool)
    out = []
    while alive.any():
        first = int(np.argmax(alive))
        idx = np.nonzero(alive)[0]
        iou = _iou_np(d[first, :4], d[idx, :4])
        if ious_seen is not None:
            ious_seen.extend(float(v) for i, v in zip(idx, iou) if i != first)
        members = idx[iou > _f32(min_iou)]
        alive[members] = False
        alive[first] = False
        w = d[first].copy()
        if len(members) > 1:
            acc, tot = np.zeros(16, _f32), _f32(0)
            for i in members:
                acc = (acc + d[i, :16] * d[i, 16]).astype(_f32)
                tot = _f32(tot + d[i, 16])
            w[:16] = acc / tot
            w[16] = tot / _f32(len(members))
        out.append(w)
    return (np.stack(out) if out else np.zeros((0, 17), _f32)), overflow


def add_margin_np(dets: np.ndarray, H: int, W: int, margin: float = MARGIN) -> np.ndarray:
    """``_add_margin_to_detections`` in float32 (round half to even)."""
    d = np.array(dets, _f32).reshape(-1, 17)
    off = np.rint(_f32(margin) * (d[:, 2] - d[:, 0])).astype(_f32)
    d[:, 0] = np.maximum(d[:, 0] - off * _f32(2), _f32(0))
    d[:, 1] = np.maximum(d[:, 1] - off, _f32(0))
    d[:, 2] = np.minimum(d[:, 2] + off, _f32(H))
    d[:, 3] = np.minimum(d[:, 3] + off, _f32(W))
    return d


def int_boxes_np(frame_dets, H: int, W: int) -> np.ndarray:
    """Per-frame NMS output -> int32 [n, 5] (frame, left, top, right, bottom),
    the margin boxes truncated toward zero: what ``crop_faces`` takes."""
    rows = []
    for f, d in enumerate(frame_dets):
        m = add_margin_np(d, H, W)
        for ymin, xmin, ymax, xmax in m[:, :4]:
            rows.append((f, int(xmin), int(ymin), int(xmax), int(ymax)))
    return np.asarray(rows, np.int32).reshape(-1, 5)


def postprocess_np(raw_r, raw_c, anchors, H: int, W: int, min_score: float = 0.75, min_iou: float = 0.3,
                   capacity: int = CAPACITY):
    """Raw tensors of F * n tiles -> (tile dets, per-frame NMS dets, int boxes, overflow per frame)."""
    tile_dets, _ = decode_np(raw_r, raw_c, anchors, min_score)
    frames = untile_np(tile_dets, H, W)
    res = [weighted_nms_np(d, min_iou, capacity) for d in frames]
    nms = [r[0] for r in res]
    return tile_dets, nms, int_boxes_np(nms, H, W), np.asarray([r[1] for r in res], np.int32)


# ------------------------------------------------------------- fixture inputs
def fixture_frame(H: int, W: int, seed: int, faces=()) -> np.ndarray:
    """uint8 [H, W, 3] of uniform noise (``default_rng(seed)``) with each
    (image [h, w, 3], y, x) of ``faces`` pasted in."""
    fr = np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    for img, y, x in faces:
        fr[y:y + img.shape[0], x:x + img.shape[1]] = img
    return fr


def fixture_input(name: str, crops: np.ndarray, paste) -> np.ndarray:
    """The inputs of tests/golden/blazeface_golden.npz, rebuilt from its paste
    positions (tools/make_golden_blazeface.py) and the two face crops of
    golden_real.npz: "video" 2 x 360 x 640 (two 112 px faces in frame 0, frame
    1 noise only), "portrait" 1 x 640 x 360 (one 112 px face), "square"
    1 x 128 x 128 (one 64 px face)."""
    paste = np.asarray(paste).reshape(-1, 2)
    faces = [area_resize_np(c, 112) for c in crops]
    if name == "video":
        return np.stack([fixture_frame(360, 640, 0, [(faces[0], *paste[0]), (faces[1], *paste[1])]),
                         fixture_frame(360, 640, 1)])
    if name == "portrait":
        return fixture_frame(640, 360, 2, [(faces[0], *paste[0])])[None]
    if name == "square":
        return fixture_frame(128, 128, 3, [(area_resize_np(faces[1], 64), *paste[0])])[None]
    raise ValueError(name)


# ------------------------------------------------------------------- the model
class _Block(nn.Module):
    """Parameter container of one BlazeBlock: convs.0 depthwise 3x3, convs.1 pointwise 1x1."""

    def __init__(self, cin: int, cout: int, stride: int = 1):
        super().__init__()
        self.stride = stride
        self.channel_pad = cout - cin
        self.convs = nn.Sequential(nn.Conv2d(cin, cin, 3, stride, 0 if stride == 2 else 1, groups=cin, bias=True),
                                   nn.Conv2d(cin, cout, 1, bias=True))

    def forward(self, *a, **k):  # pragma: no cover - the HIP path never calls it
        raise RuntimeError("parameter container")


class BlazeFace(nn.Module):
    """MediaPipe BlazeFace (front camera, 128x128, 896 anchors) with the
    reference class's attributes, state_dict and prediction methods; the
    arithmetic is the fp32 HIP path."""
    input_size = (TILE, TILE)

    def __init__(self):
        super().__init__()
        self.num_classes = 1
        self.num_anchors = NUM_ANCHORS
        self.num_coords = 16
        self.score_clipping_thresh = 100.0
        self.x_scale = self.y_scale = self.h_scale = self.w_scale = 128.0
        self.min_score_thresh = 0.75
        self.min_suppression_threshold = 0.3
        self.backbone1 = nn.Sequential(nn.Conv2d(3, 24, 5, 2, 0, bias=True), nn.ReLU(inplace=True),
                                       *[_Block(*b) for b in BLOCKS1])
        self.backbone2 = nn.Sequential(*[_Block(*b) for b in BLOCKS2])
        self.classifier_8 = nn.Conv2d(88, 2, 1, bias=True)
        self.classifier_16 = nn.Conv2d(96, 6, 1, bias=True)
        self.regressor_8 = nn.Conv2d(88, 32, 1, bias=True)
        self.regressor_16 = nn.Conv2d(96, 96, 1, bias=True)
        self.anchors = None
        self._h = None
        self._h_device = None
        self._loaded = None
        self._lock = threading.RLock()
        self.eval()
        for p in self.parameters():
            p.requires_grad_(False)

    # ------------------------------------------------------------- weights
    def _device(self):
        return self.classifier_8.weight.device

    def load_weights(self, path):
        """A torch checkpoint of the 74-key state_dict, or an ``.npz`` of the
        same keys (an ``anchors`` array in it is loaded as the anchors)."""
        if str(path).endswith(".npz"):
            with np.load(path, allow_pickle=False) as z:
                sd = {k: torch.from_numpy(np.asarray(z[k], np.float32)) for k in z.files if k != "anchors"}
                if "anchors" in z.files:
                    self._set_anchors(z["anchors"])
        else:
            sd = torch.load(path, map_location="cpu", weights_only=True)
        self.load_state_dict(sd)
        self.eval()

    def load_anchors(self, path):
        if str(path).endswith(".npz"):
            with np.load(path, allow_pickle=False) as z:
                self._set_anchors(z["anchors"])
        else:
            self._set_anchors(np.load(path, allow_pickle=False))

    def _set_anchors(self, a):
        a = torch.tensor(np.asarray(a), dtype=torch.float32, device=self._device())
        assert a.ndimension() == 2 and a.shape[0] == self.num_anchors and a.shape[1] == 4
        self.anchors = a
        self._loaded = None

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        out = super().load_state_dict(state_dict, strict=strict, assign=assign)
        self._loaded = None
        return out

    def _release(self):
        if self._h is not None:
            _lib.load().fac_bf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _ensure(self, device: torch.device):
        if device.type != "cuda":
            raise RuntimeError("BlazeFace runs on the GPU only (no CPU fallback): move the model and inputs to cuda")
        if self.anchors is None:
            raise RuntimeError("load_anchors() first")
        lib = _lib.load()
        idx = device.index if device.index is not None else torch.cuda.current_device()
        if self._h is None or self._h_device != idx:
            self._release()
            h = ctypes.c_void_p()
            _lib.check(lib.fac_bf_create(idx, ctypes.byref(h)), None, "fac_bf_create")
            self._h, self._h_device, self._loaded = h, idx, None
        v = weight_versions(self) + (self.anchors._version, self.anchors.data_ptr())
        if self._loaded != v:
            keep, descs = [], []
            items = list(self.state_dict().items()) + [("anchors", self.anchors)]
            for k, t in items:
                h = t.detach().to("cpu", torch.float32).contiguous()
                keep.append(h)
                d = _lib.TensorDesc()
                d.name = k.encode()
                d.data = h.data_ptr()
                d.ndim = h.dim()
                for i, s in enumerate(h.shape):
                    d.shape[i] = s
                descs.append(d)
            arr = (_lib.TensorDesc * len(descs))(*descs)
            _lib.check(lib.fac_bf_load(self._h, ctypes.cast(arr, ctypes.c_void_p), len(descs)), None, "fac_bf_load")
            self._loaded = v
        return lib

    @staticmethod
    def _stream(dev):
        return torch.cuda.current_stream(dev).cuda_stream

    def _work_device(self, t=None) -> torch.device:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
        return self._device()

    # ------------------------------------------------------------- inputs
    def _tiles_u8(self, x) -> torch.Tensor:
        """A batch as the reference takes it (numpy [b, 128, 128, 3] or tensor
        [b, 3, 128, 128]) -> contiguous uint8 [b, 128, 128, 3] on the device."""
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x))
        elif not (x.dtype == torch.uint8 and tuple(x.shape[1:]) == (TILE, TILE, 3)):   # NHWC uint8 tiles pass as is
            assert x.shape[1] == 3
            x = x.permute(0, 2, 3, 1)
        assert x.shape[1] == TILE and x.shape[2] == TILE and x.shape[3] == 3
        if x.dtype != torch.uint8:
            if x.dtype.is_floating_point and not bool((x == x.round()).all()):
                raise ValueError("BlazeFace takes integer pixel values 0..255")
            x = x.to(torch.uint8)
        dev = self._work_device(x)
        if dev.type != "cuda":
            raise RuntimeError("BlazeFace runs on the GPU only (no CPU fallback): move the model to cuda")
        return x.to(dev).contiguous()

    @staticmethod
    def _split(dets: torch.Tensor, counts: torch.Tensor):
        return [dets[i, :n] for i, n in enumerate(counts.cpu().tolist())]

    # -------------------------------------------------------- predictions
    def forward(self, x):
        """uint8 tiles -> [r [b, 896, 16], c [b, 896, 1]] (fp32)."""
        return list(self.debug_net(x)[2:])

    def debug_net(self, x):
        """(backbone1 [b,16,16,88], backbone2 [b,8,8,96], r, c) of uint8 tiles, NHWC fp32."""
        t = self._tiles_u8(x)
        b, dev = int(t.shape[0]), t.device
        b1 = torch.empty(b, 16, 16, 88, dtype=torch.float32, device=dev)
        b2 = torch.empty(b, 8, 8, 96, dtype=torch.float32, device=dev)
        r = torch.empty(b, NUM_ANCHORS, 16, dtype=torch.float32, device=dev)
        c = torch.empty(b, NUM_ANCHORS, 1, dtype=torch.float32, device=dev)
        if b:
            with self._lock:
                lib = self._ensure(dev)
                _lib.check(lib.fac_bf_debug_net(self._h, t.data_ptr(), b, b1.data_ptr(), b2.data_ptr(), r.data_ptr(),
                                                c.data_ptr(), self._stream(dev)), None, "fac_bf_debug_net")
        return b1, b2, r, c

    # ------------------------------------------- one layer kernel at a time
    @staticmethod
    def block_shapes(index: int):
        """((hin, hin, cin), (hout, hout, cout)) of BlazeBlock ``index`` 0..15."""
        if not 0 <= index < 16:
            raise ValueError("BlazeBlock index must be 0..15")
        h = 64
        for i, (cin, cout, stride) in enumerate(BLOCKS1 + BLOCKS2):
            if i == index:
                return (h, h, cin), (h // stride, h // stride, cout)
            h //= stride

    @staticmethod
    def _f32_in(x, dev, shape) -> torch.Tensor:
        x = torch.as_tensor(x)
        if x.dtype != torch.float32 or tuple(x.shape[1:]) != tuple(shape):
            raise ValueError(f"expected float32 [T, {', '.join(map(str, shape))}]")
        return x.to(dev).contiguous()

    @staticmethod
    def _f32_out(out, dev, shape) -> torch.Tensor:
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=dev)
        if (out.dtype != torch.float32 or out.device != dev or not out.is_contiguous()
                or tuple(out.shape) != tuple(shape)):
            raise ValueError(f"out must be a contiguous float32 {tuple(shape)} tensor on {dev}")
        return out

    def debug_stem(self, x, out=None):
        """Debug: the stem kernel alone, uint8 tiles -> [b, 64, 64, 24] (NHWC fp32)."""
        t = self._tiles_u8(x)
        b, dev = int(t.shape[0]), t.device
        out = self._f32_out(out, dev, (b, 64, 64, 24))
        if b:
            with self._lock:
                lib = self._ensure(dev)
                _lib.check(lib.fac_bf_debug_stem(self._h, t.data_ptr(), b, out.data_ptr(), self._stream(dev)),
                           None, "fac_bf_debug_stem")
        return out

    def debug_block(self, index: int, x, out=None):
        """Debug: BlazeBlock ``index`` alone, [b, hin, hin, cin] -> [b, hout, hout, cout] (NHWC fp32)."""
        sin, sout = self.block_shapes(index)
        dev = self._work_device(x)
        if dev.type != "cuda":
            raise RuntimeError("BlazeFace runs on the GPU only (no CPU fallback): move the model to cuda")
        x = self._f32_in(x, dev, sin)
        b = int(x.shape[0])
        out = self._f32_out(out, dev, (b,) + sout)
        if b:
            with self._lock:
                lib = self._ensure(dev)
                _lib.check(lib.fac_bf_debug_block(self._h, index, x.data_ptr(), b, out.data_ptr(),
                                                  self._stream(dev)), None, "fac_bf_debug_block")
        return out

    def debug_heads(self, b1, b2, out_r=None, out_c=None):
        """Debug: the heads kernel alone, backbone1 [b, 16, 16, 88] and backbone2
        [b, 8, 8, 96] -> (r [b, 896, 16], c [b, 896]) in anchor order."""
        dev = self._work_device(b1)
        if dev.type != "cuda":
            raise RuntimeError("BlazeFace runs on the GPU only (no CPU fallback): move the model to cuda")
        b1 = self._f32_in(b1, dev, (16, 16, 88))
        b2 = self._f32_in(b2, dev, (8, 8, 96))
        b = int(b1.shape[0])
        if int(b2.shape[0]) != b:
            raise ValueError("b1 and b2 must hold the same tiles")
        r = self._f32_out(out_r, dev, (b, NUM_ANCHORS, 16))
        c = self._f32_out(out_c, dev, (b, NUM_ANCHORS))
        if b:
            with self._lock:
                lib = self._ensure(dev)
                _lib.check(lib.fac_bf_debug_heads(self._h, b1.data_ptr(), b2.data_ptr(), b, r.data_ptr(),
                                                  c.data_ptr(), self._stream(dev)), None, "fac_bf_debug_heads")
        return r, c

    def predict_on_image(self, img):
        if isinstance(img, np.ndarray):
            img = torch.from_numpy(img).permute((2, 0, 1))
        return self.predict_on_batch(img.unsqueeze(0))[0]

    def predict_on_batch(self, x, apply_nms: bool = True):
        """Detections of a batch of 128x128 images: a list of [n, 17] tensors
        (ymin, xmin, ymax, xmax, 6 keypoints (x, y), score; normalised), [0, 17]
        where nothing is found."""
        t = self._tiles_u8(x)
        b, dev = int(t.shape[0]), t.device
        dets = torch.empty(b, NUM_ANCHORS, 17, dtype=torch.float32, device=dev)
        counts = torch.zeros(b, dtype=torch.int32, device=dev)
        if b:
            with self._lock:
                lib = self._ensure(dev)
                _lib.check(lib.fac_bf_tile_detections(self._h, t.data_ptr(), b, float(self.min_score_thresh),
                                                      dets.data_ptr(), counts.data_ptr(), self._stream(dev)),
                           None, "fac_bf_tile_detections")
        if apply_nms:
            return self._nms_packed(dets, counts)
        return self._split(dets, counts)

    def nms(self, detections):
        """Weighted NMS of each [n, 17] tensor of the list."""
        detections = list(detections)
        if not detections:
            return []
        dev = self._work_device(detections[0])
        if dev.type != "cuda":
            raise RuntimeError("BlazeFace runs on the GPU only (no CPU fallback): move the model to cuda")
        n = max(max(int(d.shape[0]) for d in detections), 1)
        if n > 3 * NUM_ANCHORS:
            raise ValueError(f"nms takes at most {3 * NUM_ANCHORS} detections per image")
        packed = torch.zeros(len(detections), n, 17, dtype=torch.float32, device=dev)
        for i, d in enumerate(detections):
            if d.shape[0]:
                packed[i, :d.shape[0]] = d.to(dev, torch.float32)
        counts = torch.tensor([int(d.shape[0]) for d in detections], dtype=torch.int32, device=dev)
        return self._nms_packed(packed, counts)

    def _nms_packed(self, dets: torch.Tensor, counts: torch.Tensor):
        g, stride, dev = int(dets.shape[0]), int(dets.shape[1]), dets.device
        out = torch.empty(g, CAPACITY, 17, dtype=torch.float32, device=dev)
        oc = torch.zeros(g, dtype=torch.int32, device=dev)
        ov = torch.zeros(g, dtype=torch.int32, device=dev)
        if g:
            with self._lock:
                lib = self._ensure(dev)
                _lib.check(lib.fac_bf_nms(self._h, dets.data_ptr(), counts.data_ptr(), g, stride,
                                          float(self.min_suppression_threshold), out.data_ptr(), oc.data_ptr(),
                                          ov.data_ptr(), self._stream(dev)), None, "fac_bf_nms")
        return self._split(out, oc)

    # -------------------------------------------------------- whole frames
    def tiles(self, frames: torch.Tensor) -> torch.Tensor:
        """uint8 frames [F, H, W, 3] (device) -> uint8 tiles [F * n, 128, 128, 3]."""
        frames = _check_frames(frames)
        F, H, W, _ = frames.shape
        n = tile_windows(H, W)[2]
        out = torch.empty(F * n, TILE, TILE, 3, dtype=torch.uint8, device=frames.device)
        if F:
            with self._lock:
                lib = self._ensure(frames.device)
                _lib.check(lib.fac_bf_debug_tiles(self._h, frames.data_ptr(), F, H, W, out.data_ptr(),
                                                  self._stream(frames.device)), None, "fac_bf_debug_tiles")
        return out

    def detect(self, frames: torch.Tensor):
        """The whole FaceExtractor flow on uint8 frames [F, H, W, 3] (device):
        (dets [F, CAPACITY, 17] in frame pixels before the margin, boxes
        [F, CAPACITY, 5] int32, counts [F], overflow [F]), all on the device."""
        frames = _check_frames(frames)
        F, H, W, _ = frames.shape
        dev = frames.device
        dets = torch.empty(F, CAPACITY, 17, dtype=torch.float32, device=dev)
        boxes = torch.empty(F, CAPACITY, 5, dtype=torch.int32, device=dev)
        counts = torch.zeros(F, dtype=torch.int32, device=dev)
        over = torch.zeros(F, dtype=torch.int32, device=dev)
        if F:
            with self._lock:
                lib = self._ensure(dev)
                _lib.check(lib.fac_bf_detect(self._h, frames.data_ptr(), F, H, W, float(self.min_score_thresh),
                                             float(self.min_suppression_threshold), dets.data_ptr(), boxes.data_ptr(),
                                             counts.data_ptr(), over.data_ptr(), self._stream(dev)),
                           None, "fac_bf_detect")
        return dets, boxes, counts, over

    def postprocess(self, raw_r: torch.Tensor, raw_c: torch.Tensor, H: int, W: int):
        """Debug: the post-processing of ``detect`` from caller-supplied raw
        tensors of F * n tiles of H x W frames.  Returns (tile dets
        [T, 896, 17], tile counts [T], dets, boxes, counts, overflow)."""
        n = tile_windows(H, W)[2]
        T = int(raw_r.shape[0])
        if T % n or tuple(raw_r.shape[1:]) != (NUM_ANCHORS, 16) or raw_c.numel() != T * NUM_ANCHORS:
            raise ValueError("raw tensors must be [F*n, 896, 16] and [F*n, 896, 1]")
        F = T // n
        dev = raw_r.device
        r = raw_r.to(torch.float32).contiguous()
        c = raw_c.to(dev, torch.float32).contiguous()
        td = torch.empty(T, NUM_ANCHORS, 17, dtype=torch.float32, device=dev)
        tc = torch.zeros(T, dtype=torch.int32, device=dev)
        dets = torch.empty(F, CAPACITY, 17, dtype=torch.float32, device=dev)
        boxes = torch.empty(F, CAPACITY, 5, dtype=torch.int32, device=dev)
        counts = torch.zeros(F, dtype=torch.int32, device=dev)
        over = torch.zeros(F, dtype=torch.int32, device=dev)
        if F:
            with self._lock:
                lib = self._ensure(dev)
                _lib.check(lib.fac_bf_debug_postprocess(self._h, r.data_ptr(), c.data_ptr(), F, H, W,
                                                        float(self.min_score_thresh),
                                                        float(self.min_suppression_threshold), td.data_ptr(),
                                                        tc.data_ptr(), dets.data_ptr(), boxes.data_ptr(),
                                                        counts.data_ptr(), over.data_ptr(), self._stream(dev)),
                           None, "fac_bf_debug_postprocess")
        return td, tc, dets, boxes, counts, over


def _check_frames(frames) -> torch.Tensor:
    if (not isinstance(frames, torch.Tensor) or not frames.is_cuda or frames.dtype != torch.uint8
            or frames.dim() != 4 or frames.shape[3] != 3):
        raise ValueError("frames must be a uint8 [F, H, W, 3] device tensor")
    if min(int(frames.shape[1]), int(frames.shape[2])) < TILE:
        raise ValueError(f"frames must be at least {TILE} px on both axes (the detector's tiles only shrink)")
    return frames.contiguous()


__all__ = ["BlazeFace", "CAPACITY", "tile_windows", "tile_frames_np", "area_resize_np", "decode_np", "untile_np",
           "weighted_nms_np", "add_margin_np", "int_boxes_np", "postprocess_np", "fixture_frame", "fixture_input"]
