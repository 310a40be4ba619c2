"""Automatic mask generation without a GPU: the restated grid / crop / RLE helpers of automatic_mask_generator.py against hand-computed
values, the CPU NMS yardstick on hand-made boxes, and the argument checks of the new C-ABI entries (returned as codes)."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from amg_restate import nms_cpu, rle_encode  # noqa: E402


@pytest.fixture(scope="module")
def A():
    from medical_sam2_amd import automatic_mask_generator
    return automatic_mask_generator


def test_point_grids(A):
    assert np.array_equal(A.build_point_grid(1), [[0.5, 0.5]])
    assert np.array_equal(A.build_point_grid(2), [[0.25, 0.25], [0.75, 0.25], [0.25, 0.75], [0.75, 0.75]])
    g4 = A.build_point_grid(4)
    assert g4.shape == (16, 2) and np.allclose(g4[:4, 0], [0.125, 0.375, 0.625, 0.875]) and np.all(g4[:4, 1] == 0.125)
    layers = A.build_all_layer_point_grids(8, 2, 2)
    assert [len(g) for g in layers] == [64, 16, 4]
    assert [len(g) for g in A.build_all_layer_point_grids(32, 1, 1)] == [1024, 1024]


def test_crop_boxes(A):
    assert A.generate_crop_boxes((480, 640), 0, 512 / 1500) == ([[0, 0, 640, 480]], [0])
    # 300 x 500, one layer: overlap int(512/1500 * 300) = 102, crop 301 x 201, origins x {0, 199}, y {0, 99}, x-major
    boxes, layers = A.generate_crop_boxes((300, 500), 1, 512 / 1500)
    assert boxes == [[0, 0, 500, 300], [0, 0, 301, 201], [0, 99, 301, 300], [199, 0, 500, 201], [199, 99, 500, 300]]
    assert layers == [0, 1, 1, 1, 1]
    boxes, layers = A.generate_crop_boxes((256, 256), 2, 0.25)
    assert len(boxes) == 1 + 4 + 16 and layers == [0] + [1] * 4 + [2] * 16
    assert all(0 <= b[0] < b[2] <= 256 and 0 <= b[1] < b[3] <= 256 for b in boxes)


def test_box_helpers(A):
    import torch
    b = torch.tensor([[0, 0, 50, 50], [30, 30, 60, 60], [100, 100, 200, 200]])
    # crop (100, 100, 300, 300) inside a 400 x 400 image: box 0 ends up at its top-left border, box 2 at its bottom-right one, box 1
    # 30 pixels from both (atol 20)
    near = A.is_box_near_crop_edge(b, [100, 100, 300, 300], [0, 0, 400, 400])
    assert near.tolist() == [True, False, True]
    # at the image border the crop border does not count
    assert A.is_box_near_crop_edge(b, [0, 0, 300, 300], [0, 0, 300, 300]).tolist() == [False, False, False]
    assert A.box_xyxy_to_xywh(np.array([3, 4, 10, 20], dtype=np.float32)).tolist() == [3.0, 4.0, 7.0, 16.0]


def test_rle_round_trip(A):
    rng = np.random.default_rng(0)
    cases = [np.zeros((5, 7), bool), np.ones((5, 7), bool), rng.random((33, 17)) > 0.5, rng.random((1, 9)) > 0.3]
    m = np.zeros((6, 4), bool)
    m[0, 0] = True
    cases.append(m)
    m = np.zeros((6, 4), bool)
    m[-1, -1] = True
    cases.append(m)
    for mask in cases:
        rle = rle_encode(mask)
        assert rle["size"] == list(mask.shape) and sum(rle["counts"]) == mask.size
        assert np.array_equal(A.rle_to_mask(rle), mask)
        assert A.area_from_rle(rle) == int(mask.sum())
    assert rle_encode(np.ones((2, 2), bool))["counts"] == [0, 4]
    assert rle_encode(np.zeros((2, 2), bool))["counts"] == [4]
    # column-major: the first column is (0,0), (1,0)
    assert rle_encode(np.array([[0, 1], [1, 0]], bool))["counts"] == [1, 2, 1]


def test_nms_restatement_on_hand_made_boxes():
    boxes = np.array([[0, 0, 10, 10], [0, 0, 10, 10], [1, 0, 11, 10], [20, 20, 30, 30], [5, 5, 5, 5], [5, 5, 5, 5]], np.float32)
    # ties: equal scores keep the lower index first; box 1 duplicates box 0 (IoU 1)
    keep = nms_cpu(boxes, np.array([1, 1, 0.5, 0.9, 0.1, 0.1], np.float32), 0.7)
    # box 2 overlaps box 0 by 90 / 110 = 0.818 > 0.7: suppressed; zero-area boxes have IoU 0/0 (NaN) and are never suppressed
    assert keep == [0, 3, 4, 5]
    assert nms_cpu(boxes[[1, 0]], np.array([1, 1], np.float32), 0.7) == [0]
    # IoU exactly at the threshold is kept (strict >): two 10 x 10 boxes sharing half -> 50 / 150 = 1/3 in fp32
    pair = np.array([[0, 0, 10, 10], [5, 0, 15, 10]], np.float32)
    iou = np.float32(50) / (np.float32(100) + np.float32(100) - np.float32(50))
    assert nms_cpu(pair, np.array([1, 0.5], np.float32), float(iou)) == [0, 1]
    assert nms_cpu(pair, np.array([1, 0.5], np.float32), float(iou) - 1e-6) == [0]
    assert nms_cpu(np.zeros((0, 4), np.float32), np.zeros(0, np.float32), 0.5) == []


def test_new_abi_entries_return_codes():
    from medical_sam2_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    ptr = (ctypes.addressof(buf) + 15) & ~15
    cases = {
        "mask_stats: bad sizes": lambda: L.msam2_mask_stats(ptr, 2, 256, 256, 0, 10, 0.0, 1.0, -1.0, ptr, ptr, ptr, 4096, None),
        "mask_stats: workspace": lambda: L.msam2_mask_stats(ptr, 2, 256, 256, 10, 10, 0.0, 1.0, -1.0, ptr, ptr, ptr, 4, None),
        "mask_stats: null": lambda: L.msam2_mask_stats(None, 2, 256, 256, 10, 10, 0.0, 1.0, -1.0, ptr, ptr, ptr, 4096, None),
        "mask_rle_runs: crop": lambda: L.msam2_mask_rle_runs(ptr, 2, 256, 256, 100, 100, 50, 0, 120, 120, 0.0, ptr, None),
        "mask_rle: crop": lambda: L.msam2_mask_rle(ptr, 2, 256, 256, 100, 100, -1, 0, 120, 120, 0.0, ptr, ptr, None),
        "mask_rle: null": lambda: L.msam2_mask_rle(ptr, 2, 256, 256, 100, 100, 0, 0, 120, 120, 0.0, None, ptr, None),
        "box_nms: K": lambda: L.msam2_box_nms(ptr, ptr, 1 << 20, 0.5, ptr, ptr, ptr, 1 << 30, None),
        "box_nms: workspace": lambda: L.msam2_box_nms(ptr, ptr, 100, 0.5, ptr, ptr, ptr, 16, None),
        "box_nms: null": lambda: L.msam2_box_nms(None, ptr, 100, 0.5, ptr, ptr, ptr, 1 << 20, None),
        "convt2x2_shuffle_shared: C": lambda: L.msam2_convt2x2_shuffle_shared(ptr, ptr, ptr, 1, None, None, ptr, 2, 4, 4, 48, 0, None),
        "convt2x2_shuffle_shared: stride": lambda: L.msam2_convt2x2_shuffle_shared(ptr, ptr, ptr, 1, None, None, ptr, 2, 4, 4, 32, 7, None),
        "convt2x2_shuffle_shared: align": lambda: L.msam2_convt2x2_shuffle_shared(ptr + 4, ptr, ptr, 1, None, None, ptr, 2, 4, 4, 32, 0, None),
    }
    for what, call in cases.items():
        rc = call()
        msg = L.msam2_last_error().decode()
        assert rc < 0, (what, rc)
        assert what.split(":")[0] in msg, (what, msg)
    assert L.msam2_box_nms_workspace_bytes(0) == 0 and L.msam2_box_nms_workspace_bytes(65) >= 65 * 2 * 8
    assert L.msam2_mask_stats_workspace_bytes(3) == 48
