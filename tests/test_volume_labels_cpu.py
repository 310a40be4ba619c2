"""CPU checks of the label-volume path (ops.label_slices / volume_labels.py): the float64 restatement the GPU test compares with is itself
checked against torch's float64 F.interpolate on fixtures where both are exact and against known answers; the fixtures of the GPU test's
random-field comparison keep their undecided share under the stated cap; volume_scores is eval_seg's arithmetic; the entry's argument
checks run before anything touches a device."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import volume_labels_restate as R  # noqa: E402


def interpolate64(logits, H, W):
    return torch.nn.functional.interpolate(torch.as_tensor(logits, dtype=torch.float64), size=(H, W), mode="bilinear", align_corners=False).numpy()


@pytest.mark.parametrize("low,out", R.DYADIC_CASES)
@pytest.mark.parametrize("exclusive", [False, True])
def test_restatement_equals_float64_interpolate_on_dyadic_fixtures(low, out, exclusive):
    """integer logits, weights that are multiples of 1/8: the restatement's resize and torch's are both exact, so everything is equal"""
    T, (lh, lw), (H, W) = 2, low, out
    x = R.dyadic_logits(T, lh, lw, seed=H)
    ids = R.random_ids(6, seed=H)
    gt = R.random_gt(T, H, W, ids, seed=H).numpy()
    v = interpolate64(x, H, W)
    assert np.array_equal(R.resize64(x.numpy(), H, W), v)
    ref_labels, ref_counts, _ = R.apply_rule(v, ids, 0.0, R.DYADIC_THRESHOLDS, gt, exclusive)
    labels, counts, margin = R.restate(x.numpy(), ids, H, W, 0.0, R.DYADIC_THRESHOLDS, gt, exclusive)
    assert np.array_equal(labels, ref_labels) and np.array_equal(counts, ref_counts)
    # the fixture does what it is for: ties between the repeated planes, values at exactly label_thr, every label value in use
    assert (margin == 0).any() and (v[:, 0] == v[:, 2]).all()
    assert set(np.unique(labels)) <= set(ids) | {0} and 0 in labels and ids[2] not in labels and ids[5] not in labels
    assert counts[..., 1].sum() > 0 and counts[..., 0].sum() > 0 and (counts[..., 0] <= np.minimum(counts[..., 1], counts[..., 2])).all()
    if exclusive:                                      # on the label volume every voxel counts for at most one object
        assert (counts[:, :, :, 1].sum(axis=2) <= H * W).all()


def test_known_answers():
    ids = [7, 3, 9]
    # ties go to the lower index; a later, strictly larger plane takes over
    x = np.zeros((1, 3, 2, 2))
    x[0, 0], x[0, 1], x[0, 2] = 1.0, 1.0, 0.5
    labels, counts, margin = R.restate(x, ids, 4, 4, 0.0, [0.75], None, False)
    assert (labels == 7).all() and (margin == 0).all()
    assert counts[0, 0, :, 1].tolist() == [16, 16, 0] and counts[..., 0].sum() == 0 and counts[..., 2].sum() == 0       # no gt: |P| only
    x[0, 2] = 1.5
    assert (R.restate(x, ids, 4, 4)[0] == 9).all()
    # exclusive: only the winner counts
    _, counts, _ = R.restate(x, ids, 4, 4, 0.0, [0.75], np.full((1, 4, 4), 9, dtype=np.uint8), True)
    assert counts[0, 0].tolist() == [[0, 0, 0], [0, 0, 0], [16, 16, 16]]
    # a voxel at exactly label_thr is background, just above it is not
    x = np.full((1, 1, 3, 3), 0.25)
    assert (R.restate(x, [5], 6, 6, label_thr=0.25)[0] == 0).all()
    assert (R.restate(x, [5], 6, 6, label_thr=np.nextafter(0.25, 0))[0] == 5).all()
    # all-NaN gives background, and a NaN plane never beats a finite one
    x = np.full((2, 2, 4, 4), np.nan)
    labels, counts, _ = R.restate(x, [1, 2], 8, 8, 0.0, [0.5], None, False)
    assert (labels == 0).all() and counts.sum() == 0
    x[:, 1] = 2.0
    assert (R.restate(x, [1, 2], 8, 8)[0] == 2).all()
    # lh = lw = 1: the one value everywhere
    x = np.array([[[[3.0]], [[-1.0]]]])
    labels, counts, _ = R.restate(x, [4, 8], 5, 7, 0.0, [0.0, 3.0], np.full((1, 5, 7), 4, dtype=np.uint8), False)
    assert (labels == 4).all() and counts[:, 0, 0].tolist() == [[35, 35, 35], [0, 0, 35]] and counts[:, 0, 1].tolist() == [[0, 0, 0], [0, 0, 0]]


def test_source_coordinates_are_the_fp32_ones():
    """the fused multiply-add emulated in float64 is the exact value rounded once to fp32 (no neighbour is closer), and the clamps hold"""
    from fractions import Fraction
    for l, L in [(16, 37), (64, 40), (1, 5), (8, 23), (64, 256), (256, 1024), (256, 312)]:
        i0, i1, lam = R.source_coords(l, L)
        s = Fraction(float(np.float32(l) / np.float32(L)))
        for i in range(L):
            exact = (Fraction(i) + Fraction(1, 2)) * s - Fraction(1, 2)
            f = np.float32(i0[i]) + lam[i]                             # exact: lam = f - i0 loses nothing
            assert Fraction(float(f)) == Fraction(int(i0[i])) + Fraction(float(lam[i]))
            if exact <= 0:
                assert f == 0
                continue
            for nb in (np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))):
                assert abs(Fraction(float(f)) - exact) <= abs(Fraction(float(nb)) - exact), (l, L, i)
        assert i0.min() >= 0 and i1.max() == l - 1 and (i1 >= i0).all() and (lam >= 0).all() and (lam < 1).all()


@pytest.mark.parametrize("shape", R.RANDOM_FIELD_SHAPES)
@pytest.mark.parametrize("seed", R.SEEDS)
def test_random_field_fixtures_stay_under_the_undecided_cap(shape, seed):
    """the GPU test compares labels where the margin is >= MARGIN and bounds each count by the undecided voxels of its slice: that says
    something only while few voxels are undecided.  Measured here with torch's float64 resize as well as with the restatement's."""
    T, n, (lh, lw), (H, W) = shape
    x = R.random_logits(T, n, lh, lw, seed)
    for v in (interpolate64(x, H, W), R.resize64(x.numpy(), H, W)):
        share = (R.decision_margin(v, 0.0, R.REFERENCE_THRESHOLDS) < R.MARGIN).mean(axis=(1, 2))
        assert share.max() <= R.UNDECIDED_CAP, share
    # fp32 coordinates against float64 ones: f <= 64 carries half an ulp (3.8e-6) plus the rounding of the scale (f * 6e-8 = 3.8e-6), and a
    # value moves by at most the largest step between neighbouring logits (< 40 for randn * 4) times that: 3e-4, inside MARGIN / 2
    assert np.abs(R.resize64(x.numpy(), H, W) - interpolate64(x, H, W)).max() < R.MARGIN / 2


def test_volume_scores_is_eval_seg_arithmetic(monkeypatch):
    import medical_sam2_amd.metrics as metrics
    from medical_sam2_amd.volume_labels import volume_scores
    rng = np.random.RandomState(0)
    K, T, n = 5, 3, 2
    ps = rng.randint(0, 500, (K, T, n))
    gs = np.broadcast_to(rng.randint(0, 500, (1, T, n)), (K, T, n))
    inter = np.minimum(rng.randint(0, 500, (K, T, n)), np.minimum(ps, gs))
    counts = np.stack([inter, ps, gs], -1).astype(np.int32)
    counts[:, 1, 1] = 0                                              # an absent organ that is not predicted: eval_seg's smoothing gives 1
    s = volume_scores(counts)
    # eval_seg itself on each (slice, object), its device counts replaced by the hand-made ones
    iou = dice = 0.0
    for t in range(T):
        for o in range(n):
            monkeypatch.setattr(metrics, "seg_counts", lambda *a, t=t, o=o: counts[:, t, o].astype(np.int64).reshape(K, 1, 1, 3))
            r = metrics.eval_seg(None, None, (0.1, 0.3, 0.5, 0.7, 0.9))
            assert (s["iou_per_pair"][t, o], s["dice_per_pair"][t, o]) == r
            iou, dice = iou + r[0], dice + r[1]
    assert (s["iou"], s["dice"]) == (iou / (T * n), dice / (T * n))
    assert s["iou_per_pair"][1, 1] == 1.0 and np.isnan(s["volume_dice"][:, 1]).sum() == 0
    vol = counts.astype(np.int64).sum(axis=1)
    assert np.array_equal(s["volume_dice"], 2.0 * vol[..., 0] / (vol[..., 1] + vol[..., 2]))
    assert np.array_equal(s["volume_iou"], vol[..., 0] / (vol[..., 1] + vol[..., 2] - vol[..., 0]))
    # a torch tensor is accepted as well (the device path's one copy)
    assert volume_scores(torch.from_numpy(counts))["iou"] == s["iou"]


def test_volume_figures_differ_from_the_per_slice_mean():
    """two slices, one organ: a large well-segmented cut and a small missed one.  The per-slice mean weighs them equally, the volume
    figure by voxels."""
    from medical_sam2_amd.volume_labels import volume_scores
    counts = np.array([[[[900, 1000, 1000]], [[0, 10, 10]]]], dtype=np.int32)         # [K=1, T=2, n=1, 3]
    s = volume_scores(counts)
    assert s["dice_per_pair"][:, 0] == pytest.approx([0.9, 0.0], abs=1e-5)
    assert s["dice"] == pytest.approx(0.45, abs=1e-5)
    assert s["volume_dice"][0, 0] == 2 * 900 / 2020 and s["volume_iou"][0, 0] == 900 / 1120
    assert abs(s["volume_dice"][0, 0] - s["dice"]) > 0.4
    absent = volume_scores(np.zeros((1, 2, 1, 3), dtype=np.int32))
    assert np.isnan(absent["volume_dice"]).all() and absent["dice"] == 1.0


def test_label_ids_are_checked_on_the_host():
    import medical_sam2_amd.ops as ops
    assert ops.label_ids([3, 1, 255], "cpu").tolist() == [3, 1, 255] and ops.label_ids(torch.tensor([2, 9]), "cpu").dtype == torch.uint8
    for bad in ([1, 1], [0, 2], [256], [], [-1]):
        with pytest.raises(ValueError):
            ops.label_ids(bad, "cpu")


def test_labels_from_pack():
    from medical_sam2_amd.volume_labels import labels_from_pack
    a = torch.zeros(1, 4, 4, dtype=torch.int32)
    a[0, :2] = 1
    b = torch.zeros(1, 4, 4, dtype=torch.int32)
    b[0, 1:3, 1:3] = 1
    vol = labels_from_pack({0: {2: a, 5: b}, 1: {5: b}, 2: {}}, [2, 5])
    assert vol.dtype == torch.uint8 and vol.shape == (3, 4, 4)
    assert vol[0].tolist() == [[2, 2, 2, 2], [2, 5, 5, 2], [0, 5, 5, 0], [0, 0, 0, 0]]
    assert (vol[1] == 5).sum() == 4 and vol[2].sum() == 0
    with pytest.raises(AssertionError):
        labels_from_pack({0: {300: a}}, [300])


def test_argument_errors_cross_the_abi_as_codes():
    """the limits of msam2_label_slices are refused on the host, before the device is touched, with a message naming the entry"""
    from medical_sam2_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    ptr = (ctypes.addressof(buf) + 15) & ~15                 # a valid host address: never dereferenced by the checks
    ok = dict(logits=ptr, ids=ptr, T=1, n=2, lh=4, lw=4, H=8, W=8, thr=ptr, K=5, gt=None, labels=ptr, counts=ptr)

    def call(**kw):
        a = dict(ok, **kw)
        return L.msam2_label_slices(a["logits"], a["ids"], a["T"], a["n"], a["lh"], a["lw"], a["H"], a["W"], 0.0, a["thr"], a["K"], a["gt"], 0,
                                    a["labels"], a["counts"], None)
    cases = {"n = 33": dict(n=33), "K = 9": dict(K=9), "null logits": dict(logits=None), "neither": dict(labels=None, counts=None),
             "counts need": dict(K=0, thr=None), "bad sizes": dict(H=1 << 16, W=1 << 15)}
    for what, kw in cases.items():
        rc = call(**kw)
        msg = L.msam2_last_error().decode()
        assert rc < 0, (what, rc)
        assert "label_slices" in msg and what in msg, (what, msg)
