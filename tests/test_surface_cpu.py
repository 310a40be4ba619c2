"""CPU checks of the surface-distance feature: the restatement the GPU tests compare against (tests/surface_restate.py) is itself checked
against a neighbour loop and scipy's distance transform, volume_labels.surface_scores_from_distances against the restatement's scores, and
the host-side argument checks of msam2_label_edt / msam2_label_surface_distances return codes with messages before any device access."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import components_restate as C  # noqa: E402
import surface_restate as R  # noqa: E402


def loop_surface(vol, v):
    D, H, W = vol.shape
    out = np.zeros(vol.shape, dtype=bool)
    offs = [(0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)] + ([(-1, 0, 0), (1, 0, 0)] if D >= 2 else [])
    for z, y, x in itertools.product(range(D), range(H), range(W)):
        if vol[z, y, x] != v:
            continue
        for dz, dy, dx in offs:
            a, b, c = z + dz, y + dy, x + dx
            if not (0 <= a < D and 0 <= b < H and 0 <= c < W) or vol[a, b, c] != v:
                out[z, y, x] = True
                break
    return out


def small_volumes():
    full = np.full((3, 4, 5), 7, dtype=np.uint8)                           # an organ that is the whole volume: the border is its surface
    return [C.ellipsoids((5, 12, 20), 3, 2)[0], C.ellipsoids((1, 12, 66), 2, 3)[0], C.ellipsoids((4, 1, 30), 2, 4)[0], C.noise((3, 2, 9), 3, 5), full,
            R.specials()[0][:, :12, :12].copy()]


def test_the_surface_is_the_neighbour_loop_surface():
    seen = 0
    for vol in small_volumes():
        for v in np.unique(vol):
            got, want = R.surface(vol, v), loop_surface(vol, v)
            assert np.array_equal(got, want), (vol.shape, v)
            seen += int(want.sum())
    assert seen > 500
    full = small_volumes()[4]
    assert R.surface(full, 7).sum() == 60 - 3 * 2 * 1 and not R.surface(full, 7)[1, 1:3, 1:4].any()
    flat = np.full((1, 4, 5), 7, dtype=np.uint8)                          # D == 1: the z neighbours do not count
    assert R.surface(flat, 7).sum() == 20 - 2 * 3


@pytest.mark.parametrize("k", range(3))
def test_brute_force_d2_against_scipy(k):
    vol = small_volumes()[k]
    every = np.argwhere(np.ones(vol.shape, dtype=bool))
    for v in np.unique(vol)[:3]:
        feat = R.surface(vol, v)
        assert feat.any()
        got = R.d2(every, np.argwhere(feat), (1.0, 1.0, 1.0)).reshape(vol.shape)
        _, idx = ndimage.distance_transform_edt(~feat, return_indices=True)
        want = sum((idx[a] - np.indices(vol.shape)[a]).astype(np.int64) ** 2 for a in range(3))
        assert np.array_equal(got, want.astype(np.float64)) and np.array_equal(got, R.edt(vol, v, (1.0, 1.0, 1.0)))
        for sp in R.SPACINGS[1:]:
            got = np.sqrt(R.d2(every, np.argwhere(feat), sp)).reshape(vol.shape)
            want = ndimage.distance_transform_edt(~feat, sampling=sp)
            err = np.abs(got - want) / np.maximum(want, 1e-300)
            print("spacing", sp, "max relative difference", err[want > 0].max())
            assert (err[want > 0] <= 1e-14).all() and np.array_equal(got == 0, want == 0)
    assert np.isinf(R.d2(every[:5], np.zeros((0, 3), dtype=np.int64), (1.0, 2.0, 3.0))).all()


HAND = {
    "one element": ([4.0], [9.0]),
    "two elements": ([1.0, 4.0], [0.0, 2.25]),
    "all zeros": ([0.0] * 7, [0.0] * 5),
    "position on an element": ([float(i * i) for i in range(21)], [float(i) for i in range(41)]),     # 0.95 * 20 = 19, 0.95 * 40 = 38
    "mixed": (sorted(np.random.RandomState(1).uniform(0, 50, 37).tolist()), sorted(np.random.RandomState(2).uniform(0, 90, 11).tolist())),
    "absent in gt": ([1.0, 2.0], []),
    "absent in both": ([], []),
}


def check_scores(got, want, where=""):
    assert sorted(got) == sorted(want)
    assert np.array_equal(got["surface_voxels"], want["surface_voxels"]) and got["surface_voxels"].dtype == np.int64, where
    assert np.array_equal(got["hd"], want["hd"], equal_nan=True), (where, got["hd"], want["hd"])
    assert np.array_equal(got["nsd"], want["nsd"], equal_nan=True), (where, got["nsd"], want["nsd"])
    for k in ("hd95", "assd"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), (where, k)
        ok = ~np.isnan(want[k])
        err = np.abs(got[k][ok] - want[k][ok])
        print(where, k, "max relative difference", (err / np.maximum(np.abs(want[k][ok]), 1e-300)).max() if ok.any() else 0.0)
        assert (err <= 1e-12 * np.abs(want[k][ok])).all(), (where, k, got[k], want[k])


def test_scores_from_distances_on_hand_made_lists():
    from medical_sam2_amd.volume_labels import surface_scores_from_distances
    lists = list(HAND.values())
    for pct, tol in ((95.0, (1.0,)), (95.0, (0.0, 1.5, 2.0, 100.0)), (50.0, (3.0,)), (100.0, (1.0,)), (0.0, (1.0,))):
        got = surface_scores_from_distances(lists, pct, tol)
        want = R.scores(lists, pct, tol)
        assert got["nsd"].shape == (len(lists), len(tol)) and got["hd"].dtype == np.float64
        check_scores(got, want, f"percentile {pct}, tolerances {tol}")
    got = surface_scores_from_distances(lists)
    names = list(HAND)
    j = names.index("position on an element")
    assert got["hd95"][j] == 19.0 and got["hd"][j] == 20.0                                              # max(sqrt(19^2), sqrt(38)); max(20, sqrt(40))
    j = names.index("all zeros")
    assert (got["hd"][j], got["hd95"][j], got["assd"][j], got["nsd"][j, 0]) == (0.0, 0.0, 0.0, 1.0)
    j = names.index("one element")
    assert (got["hd"][j], got["hd95"][j], got["assd"][j], got["nsd"][j, 0]) == (3.0, 3.0, 2.5, 0.0)
    for name in ("absent in gt", "absent in both"):
        j = names.index(name)
        assert all(np.isnan(got[k][j]).all() for k in ("hd", "hd95", "assd", "nsd"))
    assert got["surface_voxels"][names.index("absent in gt")].tolist() == [2, 0]
    # a tolerance that a distance meets exactly counts; one ulp below does not
    d = np.sqrt(np.float64(2.0))
    assert surface_scores_from_distances([([2.0], [2.0])], 95.0, (d, np.nextafter(d, 0)))["nsd"].tolist() == [[1.0, 0.0]]


def test_known_answers():
    from medical_sam2_amd.volume_labels import surface_scores_from_distances
    pred, gt, ids = R.shifted((5, 12, 20), 2, 7)
    same = surface_scores_from_distances([R.surface_distances(gt, gt, v, (3.0, 0.76, 0.76)) for v in ids])
    assert (same["hd"] == 0).all() and (same["hd95"] == 0).all() and (same["assd"] == 0).all() and (same["nsd"] == 1).all()
    for dz, dy, dx in ((1, 0, 0), (0, 2, 0), (0, 0, 3), (2, -3, 4)):
        a, b = np.zeros((4, 8, 9), dtype=np.uint8), np.zeros((4, 8, 9), dtype=np.uint8)
        a[1, 4, 2] = b[1 + dz, 4 + dy, 2 + dx] = 5
        for sp in R.SPACINGS:
            sz, sy, sx = (np.float64(s) for s in sp)
            want = np.sqrt((sx * sx * np.float64(dx * dx) + sy * sy * np.float64(dy * dy)) + sz * sz * np.float64(dz * dz))
            got = surface_scores_from_distances([R.surface_distances(a, b, 5, sp)], 95.0, (float(want),))
            assert got["hd"][0] == want and got["hd95"][0] == want and got["assd"][0] == want and got["nsd"][0, 0] == 1.0
            assert got["surface_voxels"].tolist() == [[1, 1]]
    absent = surface_scores_from_distances([R.surface_distances(a, np.zeros_like(a), 5, (1, 1, 1))])
    assert np.isnan(absent["hd"][0]) and np.isnan(absent["hd95"][0]) and np.isnan(absent["assd"][0]) and np.isnan(absent["nsd"][0, 0])
    # the anisotropy and tie organs of the shared fixture are what they claim
    pred, gt, ids = R.specials()
    assert R.surface_distances(pred, gt, 5, (1, 1, 1))[0].tolist() == [1.0]
    assert R.surface_distances(pred, gt, 5, (3.0, 0.76, 0.76))[0].tolist() == [np.float64(0.76) * np.float64(0.76) * 4.0]
    assert R.surface_distances(pred, gt, 6, (1, 1, 1))[0].tolist() == [9.0]


def test_argument_errors_of_the_surface_entries_are_codes_with_messages():
    """every check is made on the host before the device is touched: the pointers are host addresses that are never dereferenced"""
    from medical_sam2_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    ptr = (ctypes.addressof(buf) + 15) & ~15
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)                                                         # noqa: E731
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)                                                         # noqa: E731
    big = 1 << 40
    nan = float("nan")

    def edt(D=4, H=8, W=16, value=1, features=0, box=None, sp=(1.0, 1.0, 1.0), ws=big):
        return L.msam2_label_edt(ptr, D, H, W, value, features, box, sp[0], sp[1], sp[2], ptr, ptr, ws, None)

    def batch(n=2, D=4, H=8, W=16, boxes=None, offs=None, caps=None, sp=(1.0, 1.0, 1.0), ws=big, length=1000):
        boxes = boxes if boxes is not None else i32(*([0, 3, 0, 7, 0, 15] * n))
        offs = offs if offs is not None else i64(*[10 * k for k in range(2 * n)])
        caps = caps if caps is not None else i32(*([10] * (2 * n)))
        ids = (ctypes.c_uint8 * max(n, 1))(*range(1, max(n, 1) + 1))
        return L.msam2_label_surface_distances(ptr, ptr, D, H, W, ids, boxes, offs, caps, n, sp[0], sp[1], sp[2], ptr, length, ptr, ptr, ws, None)

    cases = {
        "label_edt: box outside the volume": (lambda: edt(box=i32(0, 4, 0, 7, 0, 15)), "outside"),
        "label_edt: box outside the volume (columns)": (lambda: edt(box=i32(0, 3, 0, 7, -1, 15)), "outside"),
        "label_edt: inverted box": (lambda: edt(box=i32(2, 1, 0, 7, 0, 15)), "inverted"),
        "label_edt: spacing 0": (lambda: edt(sp=(1.0, 0.0, 1.0)), "spacing"),
        "label_edt: negative spacing": (lambda: edt(sp=(-1.0, 1.0, 1.0)), "spacing"),
        "label_edt: NaN spacing": (lambda: edt(sp=(1.0, 1.0, nan)), "spacing"),
        "label_edt: infinite spacing": (lambda: edt(sp=(float("inf"), 1.0, 1.0)), "spacing"),
        "label_edt: spacing whose square overflows": (lambda: edt(sp=(1.0, 1e150, 1.0)), "spacing"),
        "label_edt: spacing whose square is subnormal": (lambda: edt(sp=(1.0, 1.0, 1e-155)), "spacing"),
        "label_edt: more than 2^25 rows": (lambda: edt(D=65535, H=8192, W=2), "2^25 rows"),
        "label_edt: H = 1": (lambda: edt(H=1), "bad sizes"),
        "label_edt: W = 1": (lambda: edt(W=1), "bad sizes"),
        "label_edt: features": (lambda: edt(features=2), "features"),
        "label_edt: workspace too small": (lambda: edt(ws=L.msam2_label_edt_workspace_bytes(4, 8, 16) - 1), "workspace too small"),
        "label_surface_distances: 33 organs": (lambda: batch(n=33), "33 objects"),
        "label_surface_distances: no organ": (lambda: batch(n=0), "0 objects"),
        "label_surface_distances: box outside the volume": (lambda: batch(boxes=i32(0, 3, 0, 7, 0, 15, 0, 3, 0, 8, 0, 15)), "box 1"),
        "label_surface_distances: inverted box": (lambda: batch(boxes=i32(0, 3, 5, 4, 0, 15, 0, 3, 0, 7, 0, 15)), "box 0"),
        "label_surface_distances: spacing 0": (lambda: batch(sp=(0.0, 1.0, 1.0)), "spacing"),
        "label_surface_distances: negative spacing": (lambda: batch(sp=(1.0, 1.0, -0.5)), "spacing"),
        "label_surface_distances: NaN spacing": (lambda: batch(sp=(1.0, nan, 1.0)), "spacing"),
        "label_surface_distances: spacing whose square overflows": (lambda: batch(sp=(1e150, 1.0, 1.0)), "spacing"),
        "label_surface_distances: more than 2^25 rows": (lambda: batch(n=1, D=65535, H=8192, W=2, boxes=i32(0, 65534, 0, 8191, 0, 1)), "2^25 rows"),
        "label_surface_distances: H = 1": (lambda: batch(H=1, boxes=i32(*([0, 3, 0, 0, 0, 15] * 2))), "bad sizes"),
        "label_surface_distances: W = 1": (lambda: batch(W=1, boxes=i32(*([0, 3, 0, 7, 0, 0] * 2))), "bad sizes"),
        "label_surface_distances: segment beyond dist": (lambda: batch(length=39), "leaves dist"),
        "label_surface_distances: negative capacity": (lambda: batch(caps=i32(10, -1, 10, 10)), "leaves dist"),
        "label_surface_distances: workspace too small": (lambda: batch(ws=2 * 2 * L.msam2_label_edt_workspace_bytes(4, 8, 16) - 1), "workspace too small"),
    }
    for what, (call, word) in cases.items():
        rc = call()
        msg = L.msam2_last_error().decode()
        assert rc < 0, (what, rc)
        assert what.split(":")[0] in msg and word in msg, (what, msg)
    one = L.msam2_label_edt_workspace_bytes(4, 8, 16)
    assert one == 4 * 8 * 16 * 10 + 16 and L.msam2_label_surface_distances_workspace_bytes(i32(*([0, 3, 0, 7, 0, 15] * 2)), 2) == 4 * one
    assert L.msam2_label_edt_workspace_bytes(0, 8, 16) == 0 and L.msam2_label_edt_workspace_bytes(4, 8193, 16) == 0
    assert L.msam2_label_edt_workspace_bytes(65535, 8192, 2) == 0 and L.msam2_label_edt_workspace_bytes(4096, 8192, 2) > 0   # 2^25 rows pass
    assert edt(sp=(1e-150, 1e145, 1.0), ws=0) < 0 and "workspace too small" in L.msam2_last_error().decode()                  # usable spacings
    assert L.msam2_label_surface_distances_workspace_bytes(i32(*([0, 3, 0, 7, 0, 15] * 33)), 33) == 0
    assert L.msam2_label_surface_distances_workspace_bytes(i32(0, 3, 7, 0, 0, 15), 1) == 0


def test_workspace_sizes_are_zero_exactly_beyond_the_limits():
    """the two workspace-size entries return 0 for the boxes their entries refuse and only for them: every dimension at its limit and one
    beyond (a box may be one row or column thin), 2^25 and 2^25 + 1 = 8283 x 4051 rows, 2^31 - 2 = 77 x 4681 x 5958 and 2^31 voxels, 32 and
    33 boxes"""
    from medical_sam2_amd import _lib
    L = _lib.lib()
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)                                                         # noqa: E731
    one, many = L.msam2_label_edt_workspace_bytes, L.msam2_label_surface_distances_workspace_bytes
    assert one(1, 1, 1) == 8 + 8 + 8 and one(0, 1, 1) == 0 and one(1, 0, 1) == 0 and one(1, 1, 0) == 0
    assert one(65535, 1, 1) > 0 and one(65536, 1, 1) == 0
    assert one(1, 8192, 1) > 0 and one(1, 8193, 1) == 0
    assert one(1, 1, 8192) > 0 and one(1, 1, 8193) == 0
    assert one(4096, 8192, 1) > 0 and one(8283, 4051, 1) == 0
    assert one(77, 4681, 5958) == (2 ** 31 - 2) * 10 + 4 + 312 and one(128, 4096, 4096) == 0
    assert many(i32(0, 65534, 0, 0, 0, 0), 1) == 2 * one(65535, 1, 1) and many(i32(0, 65535, 0, 0, 0, 0), 1) == 0
    assert many(i32(0, 0, 0, 8191, 0, 0), 1) == 2 * one(1, 8192, 1) and many(i32(0, 0, 0, 8192, 0, 0), 1) == 0
    assert many(i32(0, 0, 0, 0, 0, 8191), 1) == 2 * one(1, 1, 8192) and many(i32(0, 0, 0, 0, 0, 8192), 1) == 0
    assert many(i32(*([0, 3, 0, 7, 0, 15] * 32)), 32) == 64 * one(4, 8, 16) and many(i32(*([0, 3, 0, 7, 0, 15] * 33)), 33) == 0
    assert many(i32(0, 3, 0, 7, 0, 15), 0) == 0 and many(None, 1) == 0


def test_wrapper_argument_checks_need_no_device():
    import torch
    import medical_sam2_amd.ops as ops
    vol = torch.zeros(2, 4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="on the GPU"):
        ops.label_edt(vol, 1)
    for sp in ((1.0, 0.0, 1.0), (1.0, float("nan"), 1.0), (1.0, 1.0), (1.0, 1e150, 1.0), (1e-155, 1.0, 1.0), (float("inf"), 1.0, 1.0)):
        with pytest.raises(ValueError, match="spacing"):
            ops._spacing("label_edt", sp)
    assert ops._spacing("label_edt", (3, 0.76, 1e-150)) == (3.0, 0.76, 1e-150)
    from medical_sam2_amd.volume_labels import surface_scores_from_distances
    for pct in (-1.0, 100.5, float("nan")):
        with pytest.raises(ValueError, match="percentile"):
            surface_scores_from_distances([([1.0], [1.0])], pct)
