"""S3D clip staging on the CPU: the numpy restatement the GPU kernel is held
to (tests/clip_stage_ref.py) against independent anchors, and the host half of
fac_fake_amd/clip.py (box squaring, frame schedule, box table)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import clip_stage_ref as R
from fac_fake_amd import clip
from oracle import video as ov


def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ------------------------------------------------------------ the area branch
@pytest.mark.parametrize("side", [224, 225, 300, 447])
def test_square_downscale_equals_the_crop_oracle(side):
    """A square box of >= 224 px resizes to 224 x 224 with no padding: the
    config-3 crop (oracle.video.crop_resize_area) without its channel swap."""
    frame = _noise(470, 500, side)
    box = (13, 9, 13 + side, 9 + side)
    assert R.iso_size(side, side) == (224, 224)
    got = R.stage_box(frame, box)
    assert np.array_equal(got, ov.crop_resize_area(frame, box)[:, :, ::-1])


@pytest.mark.parametrize("w,h,ow,oh", [(448, 336, 224, 168), (672, 224, 224, 224)])
def test_integer_ratio_area_equals_average_pooling(w, h, ow, oh):
    """With an integer ratio on both axes every area weight is 1: the area
    branch is average pooling, rounded half up.  448 x 336 -> 224 x 168 is the
    isotropic size (ratio 2, 2); 672 x 224's isotropic height is 74 (no integer
    ratio), so the branch is evaluated at 224 x 224 (ratio 3, 1), as a kernel
    table row could ask.  (Ratios 2 x 2 and 3 x 1: sum / 4 is exact in float64
    and sum / 3 is never within 1e-6 of a .5 tie.)"""
    src = _noise(h, w, w)
    x = torch.from_numpy(src.astype(np.float64)).permute(2, 0, 1)[None]
    want = torch.floor(F.adaptive_avg_pool2d(x, (oh, ow)) + 0.5)[0].permute(1, 2, 0).numpy().astype(np.uint8)
    assert np.array_equal(R.resize_area(src, ow, oh), want)
    if (ow, oh) == R.iso_size(w, h):       # and through the whole path: padded top and bottom
        frame = np.zeros((h + 7, w + 5, 3), np.uint8)
        frame[3:3 + h, 2:2 + w] = src
        got = R.stage_box(frame, (2, 3, 2 + w, 3 + h))
        top = (224 - oh) // 2
        assert np.array_equal(got[top:top + oh], want) and not got[:top].any() and not got[top + oh:].any()


# ---------------------------------------------------------- the cubic branch
CUBIC_SIZES = [(17, 23), (1, 1), (2, 5), (223, 223), (100, 37), (53, 200), (111, 112), (7, 222)]


@pytest.fixture(scope="module")
def cubic_diffs():
    """Per (w, h): |restatement - rounded torch bicubic| over the resized image."""
    out = {}
    for w, h in CUBIC_SIZES:
        src = _noise(h, w, 1000 * w + h)
        ow, oh = R.iso_size(w, h)
        x = torch.from_numpy(src.astype(np.float64)).permute(2, 0, 1)[None]
        y = F.interpolate(x, size=(oh, ow), mode="bicubic", align_corners=False)
        want = torch.round(y.clamp(0, 255))[0].permute(1, 2, 0).numpy().astype(np.int64)
        got = R.resize_cubic(src, ow, oh).astype(np.int64)
        assert got.shape == want.shape == (oh, ow, 3)
        out[(w, h)] = np.abs(got - want)
    return out


@pytest.mark.parametrize("w,h", CUBIC_SIZES)
def test_cubic_within_one_count_of_torch_bicubic(cubic_diffs, w, h):
    """torch's bicubic has the same coordinate map, A = -0.75 and edge clamp,
    in floating point.  The 8-bit scheme rounds each tap to 1/2048 (error
    <= 2^-12 per tap), over two 4-tap passes with sum|w| <= 1.375: the integer
    result lies within 1.18 counts of the exact value, so within 1 count of
    its rounding; and on uniform noise under 8 % of the pixels differ at all
    (a restatement of the scheme gave 3.4-4.4 % on most of these sizes)."""
    d = cubic_diffs[(w, h)]
    print(f"{w} x {h}: max |diff| {d.max()}, share differing {np.count_nonzero(d) / d.size:.4f}")
    assert d.max() <= 1
    assert np.count_nonzero(d) <= 0.08 * d.size


def test_cubic_share_of_differing_pixels_overall(cubic_diffs):
    n = sum(d.size for d in cubic_diffs.values())
    k = sum(int(np.count_nonzero(d)) for d in cubic_diffs.values())
    print(f"{k} of {n} pixels differ")
    assert k <= 0.08 * n


def test_cubic_taps_sum_to_one_and_copy_at_integer_positions():
    s, taps = R.cubic_coeffs(56, 224)
    assert np.all(np.abs(taps.sum(1) - 2048) <= 2)       # four roundings of a sum that is exactly 1
    s, taps = R.cubic_coeffs(37, 37)                      # scale 1: fx = d exactly, taps (0, 1, 0, 0)
    assert np.array_equal(s, np.arange(37)) and np.array_equal(taps, np.tile([0, 2048, 0, 0], (37, 1)))
    src = _noise(37, 37, 5)
    assert np.array_equal(R.resize_cubic(src, 37, 37), src)


# ------------------------------------------------------------- the box table
@pytest.mark.parametrize("w,h,ow,oh", [(300, 150, 224, 112), (150, 300, 112, 224), (223, 1, 224, 1),
                                       (1, 300, 0, 224), (224, 100, 224, 100)])
def test_box_table_sizes(w, h, ow, oh):
    big = max(w, h)
    want = (w, h) if big == 224 else (int(w * (224 / big)), int(h * (224 / big)))
    assert want == (ow, oh)
    assert R.iso_size(w, h) == (ow, oh)
    t = clip.box_table([[2, 10, 20, 10 + w, 20 + h]], 1000, 1000)
    assert t.dtype == np.int32 and t.shape == (1, 7)
    if ow == 0:
        assert tuple(t[0, 5:]) == (0, 224)
        frame = _noise(1000, 1000, 0)
        assert not R.stage_box(frame, (10, 20, 10 + w, 20 + h)).any()   # int() == 0: the empty case
    else:
        assert tuple(t[0]) == (2, 10, 20, 10 + w, 20 + h, ow, oh)


def test_box_table_equals_the_scalar_recipe_on_many_boxes():
    rng = np.random.default_rng(11)
    H, W = 700, 900
    n = 4000
    l, t = rng.integers(-60, W, n), rng.integers(-60, H, n)
    b = np.stack([rng.integers(0, 9, n), l, t, l + rng.integers(-5, 700, n), t + rng.integers(-5, 700, n)], 1)
    tab = clip.box_table(b, H, W)
    assert np.array_equal(tab[:, :5], b)
    for row in tab:
        w = min(row[3], W) - max(row[1], 0)
        h = min(row[4], H) - max(row[2], 0)
        want = R.iso_size(int(w), int(h)) if w > 0 and h > 0 else (0, 0)
        assert (row[5], row[6]) == want, row
    assert clip.box_table(np.zeros((0, 5)), H, W).shape == (0, 7)


# ------------------------------------------------------------------ padding
def test_padding_puts_the_odd_pixel_bottom_and_right():
    assert R.pad_offsets(151, 224) == (36, 37, 0, 0)
    assert R.pad_offsets(224, 99) == (0, 0, 62, 63)
    assert R.pad_offsets(1, 1) == (111, 112, 111, 112)
    frame = 1 + _noise(300, 300, 7) % 255                  # no zero pixel
    got = R.stage_box(frame, (5, 6, 5 + 151, 6 + 224))     # 151 x 224: a copy
    assert np.array_equal(got[:, 36:36 + 151], frame[6:230, 5:156])
    assert not got[:, :36].any() and not got[:, 187:].any() and got.shape == (224, 224, 3)
    frame = 100 + frame % 56                               # 100 .. 155: no cubic undershoot reaches 0
    got = R.stage_box(frame, (0, 0, 100, 45))              # cubic to 224 x 100: rows 62 .. 161
    assert R.iso_size(100, 45) == (224, 100)
    assert not got[:62].any() and not got[162:].any() and got[62:162].all()


# ------------------------------------------------------------ square_boxes
def test_square_boxes():
    H, W = 400, 600
    b = np.array([
        [0, 100, 100, 140, 200],     # tall: 40 x 100 -> pad x by 30
        [1, 100, 100, 201, 140],     # wide: 101 x 40 -> pad y by int(61 / 2) = 30
        [2, 50, 60, 150, 160],       # square: unchanged
        [3, 10, 100, 30, 300],       # tall at the left edge: 10 - 90 -> 0
        [4, 570, 100, 590, 300],     # tall at the right edge: 590 + 90 -> 600
        [5, 100, 5, 300, 25],        # wide at the top edge
        [6, 100, 380, 300, 398],     # wide at the bottom edge: 398 + 91 -> 400
        [7, -20, -10, 80, 50],       # negative coordinates
        [8, 700, 500, 800, 650],     # fully outside, beyond the far edges
        [9, -300, 50, -200, 100],    # fully outside, before the near edge
    ])
    want = np.array([
        [0, 70, 100, 170, 200],
        [1, 100, 70, 201, 170],
        [2, 50, 60, 150, 160],
        [3, 0, 100, 120, 300],
        [4, 480, 100, 600, 300],
        [5, 100, 0, 300, 115],
        [6, 100, 289, 300, 400],
        [7, 0, 0, 80, 70],
        [8, 675, 500, 600, 400],
        [9, 0, 25, 0, 125],
    ])
    got = clip.square_boxes(b, H, W)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    # the slice the harness takes (extract_crops.py:52-69), box by box
    frame = _noise(H, W, 3)
    for (_, x0, y0, x1, y1), (_, l, t, r, bt) in zip(b[:8], got[:8]):
        w, h = x1 - x0, y1 - y0
        p_w = int((h - w) / 2) if h > w else 0
        p_h = int((w - h) / 2) if h < w else 0
        crop = frame[max(y0 - p_h, 0):y1 + p_h, max(x0 - p_w, 0):x1 + p_w]
        assert np.array_equal(crop, frame[t:bt, l:r])
    # outside boxes are empty after the kernel's clip to the frame
    for row in clip.box_table(got[8:], H, W):
        assert tuple(row[5:]) == (0, 0)
    assert clip.square_boxes(np.zeros((0, 5), np.int32), H, W).shape == (0, 5)


# ------------------------------------------------------------ clip_schedule
def test_clip_schedule():
    assert clip.clip_schedule(np.arange(199)) is None
    assert clip.clip_schedule([]) is None
    got = clip.clip_schedule(np.arange(200))
    assert np.array_equal(got, np.arange(0, 200, 10)) and len(got) == 20
    # 450 frames with gaps: the 0th, 10th, ..., 190th of the FACE frames
    ff = np.array([f for f in range(450) if f % 7 != 3 and not 100 <= f < 130])
    got = clip.clip_schedule(ff)
    assert len(got) == 20 and np.array_equal(got, ff[:200][::10]) and got[19] == ff[190]
    assert not np.array_equal(got, np.arange(0, 200, 10))
    assert np.array_equal(clip.clip_schedule(np.arange(50), first=40, step=8), [0, 8, 16, 24, 32])


def test_first_faces_takes_face_0_of_each_frame_in_frame_order():
    b = np.array([[4, 1, 1, 9, 9], [2, 5, 5, 6, 6], [4, 2, 2, 3, 3], [2, 7, 7, 8, 8], [0, 0, 0, 1, 1]])
    assert np.array_equal(clip.first_faces(b), [[0, 0, 0, 1, 1], [2, 5, 5, 6, 6], [4, 1, 1, 9, 9]])


def test_stage_clips_ref_layout():
    """Box i is frame i % T of clip i // T, planar BGR."""
    frames = np.stack([_noise(240, 250, 20), _noise(240, 250, 21)])
    boxes = [[0, 0, 0, 224, 224], [1, 3, 4, 227, 228], [1, 0, 0, 224, 224], [5, 0, 0, 224, 224]]
    out = R.stage_clips_ref(frames, boxes, 2)
    assert out.shape == (2, 3, 2, 224, 224)
    assert np.array_equal(out[0, :, 0], frames[0, :224, :224].transpose(2, 0, 1))
    assert np.array_equal(out[0, :, 1], frames[1, 4:228, 3:227].transpose(2, 0, 1))
    assert np.array_equal(out[1, :, 0], frames[1, :224, :224].transpose(2, 0, 1))
    assert not out[1, :, 1].any()                          # bad frame index
