"""Per-organ measurements without a GPU: the restatement (tests/measure_restate.py) against known answers, the host half
(volume_labels.measurements_from_tables, measurement_errors) on the restatement's tables, and the argument refusals of msam2_label_measure
through the C ABI with fake pointers (a refused call launches nothing), code and full text."""
import ctypes
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import measure_restate as R  # noqa: E402

MSAM2_ERR_ARG = -1
QS = (0, 5, 25, 50, 75, 95, 100, 33.3)


def _sum(lo, hi, p=1):
    return sum(i ** p for i in range(lo, hi + 1))


def _cuboid_row(z, y, x):
    """the ten geometry columns of the cuboid [z0, z1] x [y0, y1] x [x0, x1] (inclusive), analytically"""
    nz, ny, nx = (b - a + 1 for a, b in (z, y, x))
    return [nz * ny * nx, _sum(*z) * ny * nx, _sum(*y) * nz * nx, _sum(*x) * nz * ny, _sum(*z, 2) * ny * nx, _sum(*y, 2) * nz * nx,
            _sum(*x, 2) * nz * ny, _sum(*z) * _sum(*y) * nx, _sum(*z) * _sum(*x) * ny, _sum(*y) * _sum(*x) * nz]


def test_restatement_on_a_cuboid():
    vol = np.zeros((6, 7, 9), dtype=np.uint8)
    vol[1:4, 2:6, 3:8] = 5
    t = R.tables(vol, [5, 8])
    assert t["moments"][0, :10].tolist() == _cuboid_row((1, 3), (2, 5), (3, 7)) and t["moments"][0, 0] == 60
    assert t["moments"][0, 10:].tolist() == [0, 0, 0, 0]
    assert t["extent"][0].tolist() == [1, 3, 2, 5, 3, 7]
    assert t["faces"][0].tolist() == [2 * 4 * 5, 2 * 3 * 5, 2 * 3 * 4, 0, 0, 0]
    assert t["moments"][1].tolist() == [0] * 14 and t["extent"][1].tolist() == [-1] * 6 and t["faces"][1].tolist() == [0] * 6
    assert t["vrange"].tolist() == [[R.INT32_MAX, R.INT32_MIN]] * 2


def test_restatement_on_two_touching_cuboids():
    vol = np.zeros((4, 6, 10), dtype=np.uint8)
    vol[1:3, 1:5, 2:5] = 5                                                # 2 x 4 x 3
    vol[1:3, 1:5, 5:9] = 9                                                # 2 x 4 x 4, shares the 2 x 4 face at x = 4 | 5
    vol[0, 0, 0] = 77                                                     # not listed: like the background
    t = R.tables(vol, [5, 9])
    assert t["moments"][0, :10].tolist() == _cuboid_row((1, 2), (1, 4), (2, 4))
    assert t["moments"][1, :10].tolist() == _cuboid_row((1, 2), (1, 4), (5, 8))
    assert t["faces"][0].tolist() == [2 * 4 * 3, 2 * 2 * 3, 2 * 2 * 4, 0, 0, 0]          # the shared face counts for both
    assert t["faces"][1].tolist() == [2 * 4 * 4, 2 * 2 * 4, 2 * 2 * 4, 0, 0, 0]


def test_restatement_on_an_organ_flush_with_every_frame():
    D, H, W = 3, 4, 5
    t = R.tables(np.full((D, H, W), 200, dtype=np.uint8), [200])
    assert t["moments"][0, :10].tolist() == _cuboid_row((0, D - 1), (0, H - 1), (0, W - 1))
    assert t["faces"][0].tolist() == [0, 0, 0, 2 * H * W, 2 * D * W, 2 * D * H]
    one = R.tables(np.full((1, 1, 1), 9, dtype=np.uint8), [9])
    assert one["faces"][0].tolist() == [0, 0, 0, 2, 2, 2]                 # an axis of length 1: the voxel is on both of its ends


@pytest.fixture(scope="module")
def organs():
    vol, ids = R.blobs((5, 40, 37), 6, 2)
    img = R.hu_image(vol.shape, 3, -200, 500)
    return vol, ids, img


def _report(vol, ids, img, lo, bins, qs=QS, spacing=(2.5, 0.8, 0.7)):
    from medical_sam2_amd.volume_labels import measurements_from_tables
    t = R.tables(vol, ids, img, lo, bins)
    return t, measurements_from_tables(t["moments"], t["extent"], t["vrange"], t["faces"], t["hist"], lo, spacing, qs)


def test_percentiles_and_moments_equal_numpy(organs):
    vol, ids, img = organs
    t, m = _report(vol, ids, img, -32768, 65536)                          # nothing clipped
    assert (m["clipped"] == 0).all() and m["hist_lo"] == -32768
    present = [j for j, v in enumerate(ids) if (vol == v).any()]
    assert len(present) >= 4 and len(present) < len(ids)
    for j in present:
        val = img[vol == ids[j]].astype(np.int64)
        pct, pair = R.order_statistics(vol, ids[j], img, QS)
        assert np.array_equal(m["percentile_bounds"][j], pair)            # the order statistics are np.sort's
        assert np.abs(m["percentiles"][j] - np.percentile(val, QS)).max() <= 1e-9 and np.abs(m["percentiles"][j] - pct).max() <= 1e-9
        sv, c = int(t["moments"][j, 10]), int(t["moments"][j, 0])
        assert m["mean"][j] == sv / c and abs(m["mean"][j] - np.mean(val)) <= 1e-9
        assert abs(m["std"][j] - np.std(val.astype(np.float64))) <= 1e-9 * max(1.0, np.std(val))
        assert m["min"][j] == val.min() and m["max"][j] == val.max() and m["voxels"][j] == len(val)
        z, y, x = np.nonzero(vol == ids[j])
        pts = np.stack([z * 2.5, y * 0.8, x * 0.7], axis=1)
        assert np.allclose(m["centroid_mm"][j], pts.mean(axis=0), rtol=0, atol=1e-9)
        assert np.allclose(m["covariance_mm2"][j], np.cov(pts.T, bias=True), rtol=1e-10, atol=1e-9)
        assert np.allclose(m["volume_mm3"][j], len(z) * 2.5 * 0.8 * 0.7) and np.allclose(m["volume_ml"][j] * 1000.0, m["volume_mm3"][j])
        assert np.allclose(m["extent_mm"][j], [(z.max() - z.min() + 1) * 2.5, (y.max() - y.min() + 1) * 0.8, (x.max() - x.min() + 1) * 0.7])
        ev = np.sort(np.linalg.eigvalsh(np.cov(pts.T, bias=True)))[::-1]
        assert np.allclose(m["principal_lengths_mm"][j], 4.0 * np.sqrt(np.maximum(ev, 0.0)), rtol=1e-9, atol=1e-9)
        ax = m["principal_axes"][j]
        assert np.allclose(ax @ ax.T, np.eye(3), atol=1e-9)
        assert np.allclose(ax @ m["covariance_mm2"][j] @ ax.T, np.diag(ev), atol=1e-7 * max(1.0, ev[0]))
        f = t["faces"][j]
        assert np.allclose(m["surface_mm2"][j], f[0] * 0.8 * 0.7 + f[1] * 2.5 * 0.7 + f[2] * 2.5 * 0.8)
        assert m["frame_faces"][j].tolist() == f[3:].tolist() and bool(m["touches_frame"][j]) == bool(f[3:].any())


def test_variance_of_a_constant_organ_at_the_type_minimum_is_zero():
    vol = np.full((2, 33, 31), 4, dtype=np.uint8)
    img = np.full(vol.shape, -32768, dtype=np.int16)
    t, m = _report(vol, [4], img, -32768, 4)
    c = vol.size
    assert t["moments"][0, 10] == -32768 * c and t["moments"][0, 11] == 2 ** 30 * c
    assert m["std"][0] == 0.0 and m["mean"][0] == -32768.0                # exactly: c Svv - Sv^2 == 0 in integers
    assert Fraction(c * int(t["moments"][0, 11]) - int(t["moments"][0, 10]) ** 2, c * c) == 0
    img2 = img.copy()
    img2[0, 0, 0] = -32767                                                # variance (c - 1) / c^2 = 4.9e-4 beside Svv / c = 2^30
    t2, m2 = _report(vol, [4], img2, -32768, 4)
    assert abs(m2["std"][0] - np.sqrt(c - 1) / c) <= 1e-15                # three roundings of a value near 0.022


def test_clipped_percentiles_are_nan_never_clamped(organs):
    vol, ids, img = organs
    lo, bins = -200, 500
    t, m = _report(vol, ids, img, lo, bins)
    seen_nan = seen_value = False
    for j, v in enumerate(ids):
        if not (vol == v).any():
            continue
        val = img[vol == v].astype(np.int64)
        assert m["clipped"][j].tolist() == [int((val < lo).sum()), int((val >= lo + bins).sum())] and m["clipped"][j].min() > 0
        assert m["hist"][j].sum() + m["clipped"][j].sum() == len(val)
        pct, pair = R.order_statistics(vol, v, img, QS)
        for i in range(len(QS)):
            inside = all(lo <= s < lo + bins for s in pair[i])
            if inside:
                assert np.array_equal(m["percentile_bounds"][j, i], pair[i]) and abs(m["percentiles"][j, i] - pct[i]) <= 1e-9
                seen_value = True
            else:
                assert np.isnan(m["percentiles"][j, i])
                seen_nan = True
        assert np.isnan(m["percentiles"][j, 0]) and np.isnan(m["percentiles"][j, QS.index(100)])      # min and max lie in the tails
        assert m["min"][j] == val.min() and m["max"][j] == val.max()       # ... and are reported by the range table
    assert seen_nan and seen_value


def test_absent_organs_and_skipped_tables(organs):
    from medical_sam2_amd.volume_labels import measurements_from_tables
    vol, ids, img = organs
    t, m = _report(vol, ids, img, -200, 500)
    j = next(j for j, v in enumerate(ids) if not (vol == v).any())
    assert m["voxels"][j] == 0 and m["volume_mm3"][j] == 0.0 and m["bbox"][j].tolist() == [-1] * 6
    assert m["clipped"][j].tolist() == [0, 0] and m["hist"][j].sum() == 0 and m["frame_faces"][j].tolist() == [0, 0, 0]
    assert not m["touches_frame"][j]
    for key in ("extent_mm", "centroid_vox", "centroid_mm", "covariance_mm2", "principal_lengths_mm", "principal_axes", "surface_mm2", "mean",
                "std", "min", "max", "percentiles"):
        assert np.isnan(m[key][j]).all(), key
    geometry = measurements_from_tables(t["moments"], t["extent"])
    assert "mean" not in geometry and "surface_mm2" not in geometry and np.array_equal(geometry["voxels"], m["voxels"])
    no_hist = measurements_from_tables(t["moments"], t["extent"], t["vrange"], t["faces"])
    assert "percentiles" not in no_hist and np.array_equal(no_hist["mean"], m["mean"], equal_nan=True)


def test_measurement_errors():
    from medical_sam2_amd.volume_labels import measurement_errors
    nan = float("nan")
    pred = {"volume_mm3": np.array([110.0, 50.0, 0.0, 7.0]), "centroid_mm": np.array([[1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [nan] * 3, [1.0, 1.0, 1.0]])}
    gt = {"volume_mm3": np.array([100.0, 100.0, 10.0, 0.0]), "centroid_mm": np.array([[1.0, 5.0, 7.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [nan] * 3])}
    e = measurement_errors(pred, gt)
    assert np.allclose(e["volume_rel_diff"][:3], [0.1, -0.5, -1.0]) and np.isnan(e["volume_rel_diff"][3])
    assert e["centroid_distance_mm"][:2].tolist() == [5.0, 0.0] and np.isnan(e["centroid_distance_mm"][2:]).all()


def _abi():
    from medical_sam2_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    ptr = (ctypes.addressof(buf) + 15) & ~15

    def measure(n=2, D=2, H=4, W=4, image=ptr, image_type=1, hist_lo=0, bins=16, moments=ptr, extent=ptr, vrange=ptr, faces=ptr, hist=ptr,
                labels=ptr, ids=ptr):
        return L.msam2_label_measure(labels, ids, image, image_type, D, H, W, n, hist_lo, bins, moments, extent, vrange, faces, hist, None)

    return L, measure, ptr


SIZES = "label_measure: bad sizes (D %d of 1 .. 65535, H x W %dx%d of 1 .. 8192, at most 2^31 - 2 voxels)"
REFUSALS = [
    (dict(labels=None), "label_measure: null labels / ids / moments / extent / vrange"),
    (dict(ids=None), "label_measure: null labels / ids / moments / extent / vrange"),
    (dict(moments=None), "label_measure: null labels / ids / moments / extent / vrange"),
    (dict(extent=None), "label_measure: null labels / ids / moments / extent / vrange"),
    (dict(vrange=None), "label_measure: null labels / ids / moments / extent / vrange"),
    (dict(n=0), "label_measure: n = 0 objects (1 .. 32 per call)"),
    (dict(n=33), "label_measure: n = 33 objects (1 .. 32 per call)"),
    (dict(D=0), SIZES % (0, 4, 4)),
    (dict(D=65536), SIZES % (65536, 4, 4)),
    (dict(H=0), SIZES % (2, 0, 4)),
    (dict(H=8193), SIZES % (2, 8193, 4)),
    (dict(W=0), SIZES % (2, 4, 0)),
    (dict(W=8193), SIZES % (2, 4, 8193)),
    (dict(D=33, H=8192, W=8192), SIZES % (33, 8192, 8192)),
    (dict(image_type=2), "label_measure: image_type 2 (0 uint8, 1 int16)"),
    (dict(image_type=-1), "label_measure: image_type -1 (0 uint8, 1 int16)"),
    (dict(image="odd"), "label_measure: an int16 image must be 2-byte aligned"),
    (dict(bins=0), "label_measure: bins = 0 (1 .. 65536 with a histogram, 0 .. 65536 without)"),
    (dict(bins=65537), "label_measure: bins = 65537 (1 .. 65536 with a histogram, 0 .. 65536 without)"),
    (dict(bins=-1, hist=None), "label_measure: bins = -1 (1 .. 65536 with a histogram, 0 .. 65536 without)"),
    (dict(bins=65537, hist=None), "label_measure: bins = 65537 (1 .. 65536 with a histogram, 0 .. 65536 without)"),
    (dict(image=None), "label_measure: a histogram needs an image"),
]


@pytest.mark.parametrize("bad, text", REFUSALS, ids=["-".join("%s=%s" % kv for kv in b.items()) for b, _ in REFUSALS])
def test_refusal_code_and_text(bad, text):
    L, measure, ptr = _abi()
    if bad.get("image") == "odd":
        bad = dict(bad, image=ptr + 1)
    rc = measure(**bad)
    assert rc == MSAM2_ERR_ARG, (rc, L.msam2_last_error().decode())
    assert L.msam2_last_error().decode() == text


def test_wrapper_refusals():
    import torch

    import medical_sam2_amd.ops as ops
    vol = torch.zeros(2, 4, 6, dtype=torch.uint8)
    cases = [                                                             # (those behind the device check: tests/test_label_measure_gpu.py)
        (lambda: ops.label_measure(vol.to(torch.int16), [1]), "label_measure: labels must be a uint8 contiguous [D, H, W] label volume"),
        (lambda: ops.label_measure(vol, [1]), "label_measure: the label volume must be on the GPU"),
    ]
    for call, text in cases:
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
