"""BlazeFace detector, host side (no GPU): the fixtures, the class's surface,
the window layout and the numpy restatement of the post-processing against
the reference's recorded results (tests/golden/blazeface_golden.npz)."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

from fac_fake_amd import blazeface as bz

REPO = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def G(golden):
    return golden("blazeface_golden.npz")


@pytest.fixture(scope="module")
def W(golden):
    return golden("blazeface_weights.npz")


def _split(flat, counts):
    o = np.concatenate([[0], np.cumsum(counts)])
    return [flat[o[i]:o[i + 1]] for i in range(len(counts))]


def test_weight_fixture_is_the_class_state_dict(W):
    m = bz.BlazeFace()
    sd = m.state_dict()
    assert len(sd) == 74 and set(sd) == set(W) - {"anchors"}
    for k, v in sd.items():
        assert tuple(v.shape) == W[k].shape and W[k].dtype == np.float32, k
    assert sum(v.numel() for v in sd.values()) == 101390
    assert list(sd)[:2] == ["backbone1.0.weight", "backbone1.0.bias"]
    assert tuple(sd["backbone1.4.convs.1.weight"].shape) == (32, 28, 1, 1)
    assert tuple(sd["regressor_16.weight"].shape) == (96, 96, 1, 1)


def test_anchors_and_reference_attributes(W):
    assert W["anchors"].shape == (896, 4) and W["anchors"].dtype == np.float32
    m = bz.BlazeFace()
    m.load_weights(REPO / "tests" / "golden" / "blazeface_weights.npz")
    assert tuple(m.anchors.shape) == (896, 4)
    assert m.input_size == (128, 128) and m.num_anchors == 896 and m.num_coords == 16 and m.num_classes == 1
    assert m.min_score_thresh == 0.75 and m.min_suppression_threshold == 0.3
    assert m.score_clipping_thresh == 100.0 and m.x_scale == m.y_scale == m.w_scale == m.h_scale == 128.0
    got = m.state_dict()
    assert all(np.array_equal(got[k].numpy(), W[k]) for k in got)
    with pytest.raises(RuntimeError):          # no CPU fallback
        m.predict_on_batch(np.zeros((1, 128, 128, 3), np.uint8))


@pytest.mark.parametrize("H,Wd,want", [(360, 640, (360, 140, 3)), (1080, 1920, (1080, 420, 3)),
                                       (640, 360, (360, 0, 1)), (128, 128, (128, 0, 1)), (300, 301, (300, 0, 3))])
def test_window_layout(H, Wd, want):
    assert bz.tile_windows(H, Wd) == want
    split, step, n = want
    fr = np.arange(H * Wd * 3, dtype=np.int64).reshape(1, H, Wd, 3).astype(np.uint8)
    tiles = bz.tile_frames_np(fr)
    assert tiles.shape == (n, 128, 128, 3)
    for h in range(n):
        assert np.array_equal(tiles[h], bz.area_resize_np(fr[0, :split, h * step:h * step + split]))


def test_area_resize_closed_forms():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)
    assert np.array_equal(bz.area_resize_np(img[:128, :128]), img[:128, :128])          # scale 1: identity
    blk = img.astype(np.int64).reshape(128, 2, 128, 2, 3).sum((1, 3))
    assert np.array_equal(bz.area_resize_np(img), ((2 * blk + 4) // 8).astype(np.uint8))  # 2x2 mean, half up
    with pytest.raises(ValueError):
        bz.area_resize_np(img[:100, :100])


@pytest.mark.parametrize("name", ["video", "portrait", "square"])
def test_fixture_inputs_rebuild(G, golden, name):
    import zlib
    fr = bz.fixture_input(name, golden("golden_real.npz")["crops"], G[f"{name}_paste"])
    assert zlib.crc32(fr.tobytes()) == int(G[f"{name}_frames_crc"])
    assert zlib.crc32(bz.tile_frames_np(fr).tobytes()) == int(G[f"{name}_tiles_crc"])
    m = G[f"{name}_margins"]    # the decision margins the generator asserted
    assert m[0] >= 1e-3 and m[1] >= 1e-2 and m[2] >= 1e-4 and m[3] >= 1e-2 and m[4] >= 1e-2


def test_restatement_reproduces_the_golden_postprocessing(G, W):
    """Golden fp32 raw tensors of the 6 video tiles -> the reference's tile
    detections, per-frame NMS, margin and int boxes."""
    r = np.zeros((6, 896, 16), np.float32)
    r[:, G["video_raw_rows"]] = G["video_raw_r"]
    tile_dets, nms, boxes, over = bz.postprocess_np(r, G["video_raw_c"], W["anchors"], 360, 640)
    counts = G["video_tile_counts"]
    assert [len(d) for d in tile_dets] == counts.tolist() and counts.sum() > 2
    for d, want in zip(tile_dets, _split(G["video_tile_dets"], counts)):
        assert np.allclose(d, want, rtol=0, atol=4 * np.finfo(np.float32).eps)
    assert [len(d) for d in nms] == G["video_nms_counts"].tolist() == [2, 0]
    got, want = np.concatenate(nms), G["video_nms"]
    assert np.abs(got - want).max() <= 16 * np.finfo(np.float32).eps * 640
    margin = np.concatenate([bz.add_margin_np(d, 360, 640) for d in nms])
    assert np.abs(margin - G["video_margin"]).max() <= 16 * np.finfo(np.float32).eps * 640
    assert np.array_equal(boxes, G["video_boxes"]) and not over.any()


def test_restatement_nms_on_the_other_fixtures(G):
    for name, (H, Wd) in (("portrait", (640, 360)), ("square", (128, 128))):
        frames = bz.untile_np(_split(G[f"{name}_tile_dets"], G[f"{name}_tile_counts"]), H, Wd)
        nms = [bz.weighted_nms_np(d)[0] for d in frames]
        assert [len(d) for d in nms] == G[f"{name}_nms_counts"].tolist()
        assert np.abs(np.concatenate(nms) - G[f"{name}_nms"]).max() <= 16 * np.finfo(np.float32).eps * max(H, Wd)
        assert np.array_equal(bz.int_boxes_np(nms, H, Wd), G[f"{name}_boxes"])


def test_nms_capacity_and_overflow_count():
    d = np.zeros((1500, 17), np.float32)
    d[:, 0] = d[:, 1] = np.arange(1500) * 10.0            # disjoint 5 x 5 boxes
    d[:, 2] = d[:, 3] = np.arange(1500) * 10.0 + 5.0
    d[:, 16] = np.linspace(0.76, 0.99, 1500)
    out, over = bz.weighted_nms_np(d, 0.3, capacity=1024)
    assert len(out) == 1024 and over == 476
    assert out[:, 16].min() == np.sort(d[:, 16])[-1024]


def test_helpers_drop_in_imports_blazeface():
    spec = importlib.util.spec_from_file_location("blazeface_dropin", REPO / "helpers" / "blazeface.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.BlazeFace is bz.BlazeFace


def test_cvit_prediction_keeps_boxed_files_and_needs_a_detector(tmp_path):
    import cvit_prediction as cp
    assert cp.detector is None
    fr = np.zeros((2, 130, 130, 3), np.uint8)
    np.savez(tmp_path / "a.npz", frames=fr, boxes=np.array([[0, 1, 2, 3, 4]], np.int32))
    np.savez(tmp_path / "b.npz", frames=fr)
    assert cp.read_video(str(tmp_path / "a.npz"))[1].tolist() == [[0, 1, 2, 3, 4]]
    with pytest.raises(KeyError):
        cp.read_video(str(tmp_path / "b.npz"))


def test_abi_argument_checks(built_lib):
    import ctypes
    from fac_fake_amd import _lib
    lib = _lib.load()
    assert lib.fac_bf_capacity() == bz.CAPACITY >= 1024
    assert lib.fac_bf_create(0, None) == -1
    assert lib.fac_bf_load(None, None, 0) == -1
    assert lib.fac_bf_detect(None, None, 1, 360, 640, 0.75, 0.3, None, None, None, None, None) == -1
    assert lib.fac_bf_debug_net(None, None, 1, None, None, None, None, None) == -1
    lib.fac_bf_destroy(None)
    h = ctypes.c_void_p()
    assert lib.fac_bf_create(0, ctypes.byref(h)) == 0
    t = torch.zeros(4)
    assert lib.fac_bf_tile_detections(h, t.data_ptr(), 1, 0.75, t.data_ptr(), t.data_ptr(), None) == -5  # not loaded
    # the one-kernel debug entries: null handle / pointer, tile count and block index are argument errors
    # (checked before the handle's state); good arguments on a handle without weights are "not loaded"
    p = t.data_ptr()
    assert lib.fac_bf_debug_stem(None, p, 1, p, None) == -1
    assert lib.fac_bf_debug_stem(h, None, 1, p, None) == -1
    assert lib.fac_bf_debug_stem(h, p, 1, None, None) == -1
    assert lib.fac_bf_debug_stem(h, p, 0, p, None) == -1
    assert lib.fac_bf_debug_stem(h, p, (1 << 20) + 1, p, None) == -1
    assert lib.fac_bf_debug_stem(h, p, 1, p, None) == -5
    assert lib.fac_bf_debug_block(None, 0, p, 1, p, None) == -1
    assert lib.fac_bf_debug_block(h, 0, None, 1, p, None) == -1
    assert lib.fac_bf_debug_block(h, 0, p, 1, None, None) == -1
    assert lib.fac_bf_debug_block(h, 0, p, 0, p, None) == -1
    assert lib.fac_bf_debug_block(h, 0, p, (1 << 20) + 1, p, None) == -1
    assert lib.fac_bf_debug_block(h, -1, p, 1, p, None) == -1
    assert lib.fac_bf_debug_block(h, 16, p, 1, p, None) == -1
    assert all(lib.fac_bf_debug_block(h, i, p, 1, p, None) == -5 for i in range(16))
    assert lib.fac_bf_debug_heads(None, p, p, 1, p, p, None) == -1
    for i in range(4):
        ptrs = [p, p, p, p]
        ptrs[i] = None
        assert lib.fac_bf_debug_heads(h, ptrs[0], ptrs[1], 1, ptrs[2], ptrs[3], None) == -1, i
    assert lib.fac_bf_debug_heads(h, p, p, 0, p, p, None) == -1
    assert lib.fac_bf_debug_heads(h, p, p, (1 << 20) + 1, p, p, None) == -1
    assert lib.fac_bf_debug_heads(h, p, p, 1, p, p, None) == -5
    d = _lib.TensorDesc()
    d.name, d.data, d.ndim = b"backbone1.0.weight", t.data_ptr(), 1
    d.shape[0] = 4
    arr = (_lib.TensorDesc * 1)(d)
    assert lib.fac_bf_load(h, ctypes.cast(arr, ctypes.c_void_p), 1) == -3                                 # keys missing
    lib.fac_bf_destroy(h)
