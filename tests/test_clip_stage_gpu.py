"""S3D clip staging on the GPU: fac_clip_stage_u8 (fac_fake_amd/csrc/clip.hip)
bit for bit against the numpy restatement (tests/clip_stage_ref.py), and the
video-level entry points of fac_fake_amd/clip.py."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import clip_stage_ref as R  # noqa: E402
from fac_fake_amd import clip, video  # noqa: E402
from fac_fake_amd.weights import make_ca_s3d_state_dict, make_msca_s3d_state_dict, make_s3d_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = Path(__file__).resolve().parent / "golden"


def _box(f, l, t, w, h):
    return [f, l, t, l + w, t + h]


# frames [3, 340, 460, 3]; (frame, left, top, right, bottom), w x h in the comments
KERNEL_BOXES = [
    _box(0, 7, 5, 224, 224),        # copy
    _box(1, 100, 30, 224, 100),     # copy, padded top / bottom
    _box(2, 11, 3, 100, 224),       # copy, padded left / right
    _box(0, 20, 10, 300, 300),      # area, square
    _box(1, 5, 2, 448, 336),        # area, ratio 2: 224 x 168
    [2, 1, 1, 500, 400],            # area, clipped by the frame to 459 x 339
    _box(0, 30, 200, 400, 2),       # area, 2 px high: 224 x 1
    _box(1, 3, 9, 17, 23),          # cubic
    _box(2, 459, 339, 1, 1),        # cubic, one pixel (the frame's last)
    _box(0, 200, 100, 2, 5),
    _box(1, 0, 0, 223, 223),
    _box(2, 300, 17, 100, 37),
    _box(0, 453, 100, 7, 222),
    [1, -4, -6, 49, 196],           # cubic, clipped to 49 x 196 at the near edges
    _box(2, 50, 50, 0, 40),         # empty
    _box(0, 50, 50, 40, -3),        # negative height
    _box(1, 600, 400, 100, 100),    # outside
    [2, -90, -80, -10, -5],         # outside, before the frame
    _box(-1, 0, 0, 224, 224),       # bad frame indices
    _box(3, 0, 0, 224, 224),
    _box(0, 10, 10, 300, 1),        # oh = int(1 * 224 / 300) = 0
    _box(1, 10, 10, 1, 300),        # ow = 0
    _box(2, 2, 0, 151, 224),        # copy with an odd margin: left 36, right 37
    _box(0, 0, 100, 460, 120),      # area, the full frame width
    _box(1, 50, 10, 120, 330),      # area, tall: 81 x 224
    _box(2, 0, 0, 460, 340),        # area, the whole last frame
]


@pytest.fixture(scope="module")
def kernel_case():
    frames = np.random.default_rng(5).integers(0, 256, (3, 340, 460, 3), dtype=np.uint8)
    boxes = np.asarray(KERNEL_BOXES, np.int32)
    assert len(boxes) % 2 == 0
    return frames, boxes, R.stage_clips_ref(frames, boxes, 2)


def test_kernel_equals_the_restatement_bit_for_bit(kernel_case):
    frames, boxes, want = kernel_case
    out = torch.full((len(boxes) // 2, 3, 2, 224, 224), 0xAA, dtype=torch.uint8, device=DEV)
    got = clip.stage_clips(torch.from_numpy(frames).to(DEV), boxes, T=2, out=out)
    assert got is out
    got = got.cpu().numpy()
    for i in range(len(boxes)):
        g, w = got[i // 2, :, i % 2], want[i // 2, :, i % 2]
        assert np.array_equal(g, w), (i, boxes[i].tolist(), int(np.count_nonzero(g != w)),
                                      int(np.abs(g.astype(int) - w).max()))
    # the cases the list is meant to hold: every branch and non-trivial content
    tab = clip.box_table(boxes, 340, 460)
    assert tuple(tab[5, 5:]) == (224, 165) and tuple(tab[6, 5:]) == (224, 1) and tuple(tab[20, 5:]) == (224, 0)
    assert want[0, :, 0].any() and want[1, :, 1].any() and want[3, :, 0].any() and not want[7:11].any()


def test_smallest_frames():
    """Two pixels in all (the kernel loads a pixel as a dword; the last pixel's starts a byte early)."""
    frames = np.asarray([[[[10, 200, 30], [250, 5, 128]]]], np.uint8)
    boxes = np.asarray([[0, 0, 0, 2, 1], [0, 1, 0, 2, 1], [0, 0, 0, 1, 1], [0, -3, -3, 9, 9]], np.int32)
    for fr in (frames, frames.transpose(0, 2, 1, 3).copy()):                # 1 x 2 and 2 x 1
        b = boxes if fr is frames else boxes[:, [0, 2, 1, 4, 3]]
        got = clip.stage_clips(torch.from_numpy(fr).to(DEV), b, T=4)
        assert np.array_equal(got.cpu().numpy(), R.stage_clips_ref(fr, b, 4))


def test_area_sums_at_the_32_bit_limit():
    """The kernel divides in 32 bits while 511 * cw * ch < 2^32 (boxes of up to
    8 404 991 px) and in 64 bits beyond: the largest square below (2899^2) and
    the first above (2900^2), on bright pixels (sums near 255 * cw * ch).  The
    reference is the restatement's overlap matrices in float64 matrix products,
    exact here (every partial sum is an integer of at most 255 * 2900^2 < 2^53)."""
    g = torch.Generator(device=DEV).manual_seed(2)
    fr = torch.randint(236, 256, (1, 2900, 2900, 3), dtype=torch.uint8, device=DEV, generator=g)
    boxes = np.asarray([[0, 0, 0, 2900, 2900], [0, 1, 0, 2900, 2899]], np.int32)
    sizes = [tuple(r) for r in clip.box_table(boxes, 2900, 2900)[:, 5:]]
    assert sizes == [(224, 224), (223, 224)] == [R.iso_size(2900, 2900), R.iso_size(2899, 2899)]
    got = clip.stage_clips(fr, boxes, T=2).cpu().numpy()
    host = fr[0].cpu().numpy().astype(np.float64)
    for i, side in enumerate((2900, 2899)):
        ow, oh = sizes[i]
        src = host[:side, 2900 - side:]
        ry, rx = R.overlap_matrix(side, oh).astype(np.float64), R.overlap_matrix(side, ow).astype(np.float64)
        den = side * side
        left = R.pad_offsets(ow, oh)[0]
        for c in range(3):
            num = (ry @ np.ascontiguousarray(src[:, :, c]) @ rx.T).astype(np.int64)   # (contiguous: BLAS)
            want = np.zeros((224, 224), np.int64)
            want[:, left:left + ow] = (2 * num + den) // (2 * den)
            assert num.min() >= 236 * den and np.array_equal(got[0, c, i], want), (side, c)


def test_square_boxes_equal_the_crop_kernel(kernel_case):
    """>= 224 px squares resize to 224 x 224 by the same area sums as
    fac_crop_resize_u8, which swaps the channels and stores them interleaved."""
    frames = torch.from_numpy(kernel_case[0]).to(DEV)
    boxes = np.asarray([_box(0, 3, 4, 224, 224), _box(1, 0, 0, 225, 225), _box(2, 40, 20, 300, 300),
                        _box(0, 100, 1, 339, 339)], np.int32)
    assert [tuple(r) for r in clip.box_table(boxes, 340, 460)[:, 5:]] == [(224, 224)] * 4
    got = clip.stage_clips(frames, boxes, T=4)
    crops = video.crop_faces(frames, boxes)                            # [4, 224, 224, 3] RGB
    assert tuple(got.shape) == (1, 3, 4, 224, 224)
    assert torch.equal(got[0], crops.flip(3).permute(3, 0, 1, 2))


def test_out_slices_fill_one_batch():
    g = torch.Generator(device=DEV).manual_seed(9)
    fa = torch.randint(0, 256, (20, 300, 280, 3), dtype=torch.uint8, device=DEV, generator=g)
    fb = torch.randint(0, 256, (25, 200, 420, 3), dtype=torch.uint8, device=DEV, generator=g)
    ba = np.asarray([_box(i, i, 2 * i, 150 + 7 * i, 130 + 8 * i) for i in range(20)], np.int32)
    bb = np.asarray([_box(24 - i, 3 * i, i, 100 + 15 * i, 190 - 6 * i) for i in range(20)], np.int32)
    batch = torch.full((2, 3, 20, 224, 224), 0xAA, dtype=torch.uint8, device=DEV)
    assert clip.stage_clips(fa, ba, out=batch[0:1]).data_ptr() == batch.data_ptr()
    clip.stage_clips(fb, bb, out=batch[1:2])
    a, b = clip.stage_clips(fa, ba), clip.stage_clips(fb, bb)
    assert tuple(a.shape) == (1, 3, 20, 224, 224) and a.dtype == torch.uint8
    assert torch.equal(batch[0:1], a) and torch.equal(batch[1:2], b)
    assert np.array_equal(b.cpu().numpy(), R.stage_clips_ref(fb.cpu().numpy(), bb, 20))
    assert tuple(clip.stage_clips(fa, np.zeros((0, 5), np.int32)).shape) == (0, 3, 20, 224, 224)


def test_wrong_inputs_raise():
    fr = torch.zeros(2, 240, 250, 3, dtype=torch.uint8, device=DEV)
    boxes = np.asarray([_box(0, 0, 0, 100, 100), _box(1, 0, 0, 100, 100)], np.int32)
    ok = clip.stage_clips(fr, boxes, T=2)
    assert tuple(ok.shape) == (1, 3, 2, 224, 224)
    bad = [
        lambda: clip.stage_clips(fr.cpu(), boxes, T=2),                            # device
        lambda: clip.stage_clips(fr.float(), boxes, T=2),                          # dtype
        lambda: clip.stage_clips(fr[..., :2], boxes, T=2),                         # shape
        lambda: clip.stage_clips(fr[0], boxes, T=2),
        lambda: clip.stage_clips(fr.cpu().numpy(), boxes, T=2),
        lambda: clip.stage_clips(fr, boxes[:, :4], T=2),                           # boxes [n, 4]
        lambda: clip.stage_clips(fr, boxes, T=20),                                 # n % T
        lambda: clip.stage_clips(fr, boxes[:1], T=2),
        lambda: clip.stage_clips(fr, boxes, T=0),
        lambda: clip.stage_clips(fr[:1, :1, :1], boxes, T=2),                      # one pixel
        lambda: clip.stage_clips(fr[:0], boxes, T=2),
        lambda: clip.stage_clips(fr, boxes, T=2, out=torch.empty(1, 3, 2, 224, 224, device=DEV)),             # out dtype
        lambda: clip.stage_clips(fr, boxes, T=2, out=torch.empty(2, 3, 1, 224, 224, dtype=torch.uint8, device=DEV)),
        lambda: clip.stage_clips(fr, boxes, T=2, out=torch.empty(1, 3, 2, 224, 224, dtype=torch.uint8)),      # out device
        lambda: clip.stage_clips(fr, boxes, T=2,
                                 out=torch.empty(1, 3, 2, 224, 448, dtype=torch.uint8, device=DEV)[..., ::2]),
    ]
    for i, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail(f"case {i} did not raise")


# ------------------------------------------------------------- end to end
def _load(cls, make, srm, dt="fp16"):
    m = cls(1, srm, dtype=dt)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in make(0, 1, srm == "yes").items()})
    return m


@pytest.fixture(scope="module")
def e2e():
    """230 frames of 256 x 320 with a face box on every frame but a few, boxes
    of every shape (tall, wide, over the frame edge, above and below 224 px),
    a second face on some frames; and the harness's clip by the restatement:
    face 0 per frame, every 10th of the first 200, squared box by box."""
    rng = np.random.default_rng(21)
    frames = rng.integers(0, 256, (230, 256, 320, 3), dtype=np.uint8)
    rows = []
    for f in range(230):
        if f in (0, 7, 50, 51, 52, 120, 199):
            continue
        w, h = int(rng.integers(30, 300)), int(rng.integers(30, 250))
        l, t = int(rng.integers(-20, 300)), int(rng.integers(-20, 230))
        rows.append([f, l, t, l + w, t + h])
        if f % 9 == 0:
            rows.append([f, 5, 5, 60, 60])            # face 1: never read
    boxes = np.asarray(rows, np.int32)
    face0 = {}
    for r in rows:
        face0.setdefault(r[0], r)
    ids = sorted(face0)[:200][::10]
    sq = []
    for f in ids:
        _, x0, y0, x1, y1 = face0[f]
        w, h = x1 - x0, y1 - y0
        p_w = int((h - w) / 2) if h > w else 0
        p_h = int((w - h) / 2) if h < w else 0
        sq.append([f, max(x0 - p_w, 0), max(y0 - p_h, 0), max(x1 + p_w, 0), max(y1 + p_h, 0)])
    want = R.stage_clips_ref(frames, np.asarray(sq), 20)
    assert len(ids) == 20 and ids[0] == 1 and want.shape == (1, 3, 20, 224, 224)
    return frames, boxes, want, np.asarray(sq, np.int32)


@pytest.fixture(scope="module")
def s3d_model():
    from fac_fake_amd.s3d import S3D
    return _load(S3D, make_s3d_state_dict, "no")


def test_predict_clip_video_end_to_end(e2e, s3d_model):
    from fac_fake_amd.s3d import video_predictions
    frames, boxes, want, sq = e2e
    fr = torch.from_numpy(frames).to(DEV)
    H, W = frames.shape[1:3]
    # the clip, bit for bit
    sel = clip.square_boxes(clip.first_faces(boxes)[:200:10], H, W)
    assert np.array_equal(clip.box_table(sel, H, W)[:, 5:], clip.box_table(sq, H, W)[:, 5:])
    got = clip.stage_clips(fr, sel)
    assert np.array_equal(got.cpu().numpy(), want)
    # the score
    with torch.no_grad():
        _, p_ref = s3d_model(torch.from_numpy(want).to(DEV), return_probs=True)
    score, probs = clip.predict_clip_video(s3d_model, fr, boxes, return_probs=True)
    assert tuple(probs.shape) == (1, 1) and torch.equal(probs, p_ref)
    assert score == float(p_ref.double().cpu()[0][0]) == video_predictions(s3d_model, got)[0]
    assert 0.0 < score < 1.0
    assert clip.predict_clip_video(s3d_model, fr, boxes) == score
    assert clip.predict_clip_video(s3d_model, frames, boxes) == score          # a host video: 20 frames uploaded
    # the harness skips a video with fewer than 200 face frames
    short = boxes[boxes[:, 0] < 150]
    assert clip.predict_clip_video(s3d_model, fr[:150], short) is None
    assert clip.predict_clip_video(s3d_model, fr, boxes[boxes[:, 0] != 229][:-30]) is None
    assert clip.predict_clip_video(s3d_model, fr[:150], short, return_probs=True) == (None, None)


@pytest.mark.parametrize("name,srm", [("ca", "yes"), ("msca", "no")])
def test_the_other_models_score_the_same_clip(e2e, name, srm):
    from fac_fake_amd.ca_s3d import CA_S3D_v3
    from fac_fake_amd.msca_s3d import msca_S3D
    cls, make = {"ca": (CA_S3D_v3, make_ca_s3d_state_dict), "msca": (msca_S3D, make_msca_s3d_state_dict)}[name]
    m = _load(cls, make, srm)
    frames, boxes, want, _ = e2e
    with torch.no_grad():
        _, p_ref = m(torch.from_numpy(want).to(DEV), return_probs=True)
    score, probs = clip.predict_clip_video(m, torch.from_numpy(frames).to(DEV), boxes, return_probs=True)
    assert torch.equal(probs, p_ref) and score == float(p_ref.double().cpu()[0][0]) and 0.0 < score < 1.0


class _Counting:
    """The detector, counting the frames it is asked to search."""

    def __init__(self, det):
        self.det, self.frames = det, 0

    def detect(self, frames):
        self.frames += int(frames.shape[0])
        return self.det.detect(frames)


def test_predict_clip_video_detect(golden, s3d_model, built_lib):
    from fac_fake_amd import blazeface as bz
    det = bz.BlazeFace().to(DEV)
    det.load_weights(GOLDEN / "blazeface_weights.npz")
    det.load_anchors(GOLDEN / "blazeface_weights.npz")
    two = bz.fixture_input("video", golden("golden_real.npz")["crops"], golden("blazeface_golden.npz")["video_paste"])
    # the BlazeFace tests' 2 x 360 x 640 video (faces in frame 0 only) 205 times
    # over, each frame shifted by its own amount so the 20 clip frames differ
    fr = torch.from_numpy(two).to(DEV).repeat(205, 1, 1, 1)
    for k in range(0, 410, 2):
        fr[k] = torch.roll(fr[k], shifts=(k // 2) % 40, dims=1)
    boxes = video.detect_faces(det, fr)
    face_frames = np.unique(boxes[:, 0])
    assert len(face_frames) >= 200 and (face_frames % 2 == 0).all()
    want = clip.predict_clip_video(s3d_model, fr, boxes, return_probs=True)
    assert want[0] is not None
    cnt = _Counting(det)
    got = clip.predict_clip_video_detect(s3d_model, cnt, fr, chunk=50, return_probs=True)
    assert got[0] == want[0] and torch.equal(got[1], want[1])
    # the search stops with the chunk that holds the 200th face frame (25 face
    # frames per chunk when every even frame has one: 400 of the 410 frames)
    assert cnt.frames == min(410, (int(face_frames[199]) // 50 + 1) * 50) < 410
    assert clip.predict_clip_video_detect(s3d_model, det, fr) == want[0]                 # the default chunk
    assert clip.predict_clip_video_detect(s3d_model, det, fr.cpu().numpy(), chunk=128) == want[0]
    assert clip.predict_clip_video_detect(s3d_model, det, fr[:300]) is None              # 150 face frames
