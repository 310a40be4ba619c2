"""CPU checks of the corrective-click path (ops.label_error_clicks / prompts.corrective_clicks / prompts.worst_slices): the numpy restatement
the GPU test compares with is scipy's zero-padded distance transform, squared, with np.argmax's first maximum -- SAM 2's
sample_one_point_from_error_center; every fixture group tells its simulated mistake from the rule; worst_slices' order on CPU tensors; the
entry's limits and the wrappers' checks act before anything touches a device."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clicks_restate as R  # noqa: E402

CASES = list(R.cases())


@pytest.mark.parametrize("name,pred,gt,ids", CASES, ids=[c[0] for c in CASES])
def test_restatement_is_the_padded_scipy_transform(name, pred, gt, ids):
    from scipy.ndimage import distance_transform_edt
    ref = R.reference(name, pred, gt, ids)
    W = pred.shape[2]
    for d in range(pred.shape[0]):
        for j, v in enumerate(ids):
            for kind, reg in enumerate(R.regions(pred[d], gt[d], v)):
                mine = R.d2_brute(reg)
                theirs = np.rint(distance_transform_edt(np.pad(reg, 1))[1:-1, 1:-1] ** 2).astype(np.int64)
                assert np.array_equal(mine, theirs), (d, j, kind)
                assert ref[d, j, 3 + kind] == reg.sum() and ref[d, j, 5 + kind] == mine.max(initial=0)
                if reg.any():
                    assert (mine[reg] >= 1).all()
                    assert np.array_equal(R.d2_chunked(reg), mine), (d, j, kind)      # the model the carry defects are cut from
                    wins = ref[d, j, 2] == 1 - kind
                    at = int(np.argmax(distance_transform_edt(np.pad(reg, 1))[1:-1, 1:-1]))
                    # scipy's float map and the integer map have their first maximum at the same voxel
                    assert at == int(np.argmax(mine)) and (not wins or (ref[d, j, 1] * W + ref[d, j, 0]) == at), (d, j, kind)
            fn, fp = R.regions(pred[d], gt[d], v)
            if not (fn.any() or fp.any()):
                assert ref[d, j].tolist() == [-1, -1, -1, 0, 0, 0, 0, 0]
            else:
                assert ref[d, j, 2] == int(ref[d, j, 5] > ref[d, j, 6]) and ref[d, j, 7] == 0


def _tables(defect, name, pred, gt, ids):
    """(centre, uniform at u = 0, uniform at the last voxel) under a defect"""
    counts = R.reference(name, pred, gt, ids)[..., 3:5].sum(-1)
    zeros = np.zeros_like(counts)
    return (R.table(pred, gt, ids, defect=defect) if defect != "u_off_by_one" else None,
            R.table(pred, gt, ids, "uniform", u=zeros, defect=defect), R.table(pred, gt, ids, "uniform", k=np.maximum(counts - 1, 0), defect=defect))


@pytest.mark.parametrize("defect", sorted(R.DEFECTS))
def test_every_fixture_group_detects_its_defect(defect):
    group = [c for c in CASES if c[0].startswith(R.DEFECTS[defect])]
    assert group, defect
    changed = []
    for name, pred, gt, ids in group:
        good, bad = _tables(None, name, pred, gt, ids), _tables(defect, name, pred, gt, ids)
        if defect != "u_off_by_one":
            assert np.array_equal(good[0], R.reference(name, pred, gt, ids))
        if any(b is not None and not np.array_equal(g, b) for g, b in zip(good, bad)):
            changed.append(name)
    assert changed, (defect, "no fixture of group", R.DEFECTS[defect], "shows it")


def test_fixtures_do_what_they_are_for():
    seen = {name: (pred, gt, ids) for name, pred, gt, ids in CASES}
    shapes = {pred.shape for pred, _, _ in seen.values()}
    assert {s[2] for s in shapes} >= {1, 63, 64, 65, 130, 200} and {s[1] for s in shapes} >= {1, 2, 37} and {s[0] for s in shapes} == {1, 5}
    for name, (pred, gt, ids) in seen.items():
        assert pred.dtype == gt.dtype == np.uint8 and pred.shape == gt.shape and 1 <= len(ids) <= 32 and len(set(ids)) == len(ids), name
    assert {len(ids) for _, _, ids in seen.values()} >= {1, 3, R.MAX_OBJ}
    ref = {name: R.reference(name, *seen[name]) for name in ("edges_5x37x200", "edges_5x37x130", "ties_5x37x65", "blobs_5x37x65", "equal_5x37x65",
                                                             "stray_1x37x130")}
    for name in ("edges_5x37x200", "edges_5x37x130"):
        pred, gt, ids = seen[name]
        t, (H, W) = ref[name], pred.shape[1:]
        assert t[0, 0, 3] == W + H - 2 and t[0, 1, 3] == W                              # regions that span every 64-column chunk: the carry
        assert (t[1, :, 4] == [2, 1, 1]).all() and t[1, 0, :3].tolist() == [0, 0, 0]  # corners, the first in raster order
        assert H < W and t[2, 1].tolist() == [(H - 1) // 2, (H - 1) // 2, 1, H * W, 0, ((H + 1) // 2) ** 2, 0, 0]   # a region that fills the slice
        assert t[3, 0, 3] == H * W and t[3, 1, 4] == H * W and t[3, 0, 2] == 1 and t[3, 1, 2] == 0        # every voxel FN of 3 and FP of 200
    t = ref["ties_5x37x65"]
    assert t[1, 2, 5] == t[1, 2, 6] > 0 and t[1, 2, 2] == 0                             # equal maxima: negative
    assert t[3, 2, 2] == 1 and t[4, 1, 3] > 0
    pred, gt, ids = seen["ties_5x37x65"]
    m = R.d2_brute(R.regions(pred[0], gt[0], 3)[0])
    assert (m == m.max()).sum() > 1                                                     # several voxels share the maximum
    t = ref["blobs_5x37x65"]
    assert (t[:, 2, 2] == -1).all() and (t[1, :, 2] == -1).all()                        # absent everywhere; a slice without error
    assert (t[:, :2, 2] >= 0).any() and {0, 1} <= set(t[..., 2].reshape(-1).tolist())
    pred, gt, ids = seen["blobs_5x37x65"]
    both = (pred != gt) & np.isin(pred, ids) & np.isin(gt, ids)
    assert both.any()                                                                   # voxels that are FP of one id and FN of another
    assert R.STRAY in np.unique(gt) and R.STRAY not in ids
    assert (ref["equal_5x37x65"][..., 2] == -1).all() and (ref["equal_5x37x65"][..., 3:] == 0).all()
    # the carry group: maxima decided by a row distance across a 64-column boundary, in chunks 0, 1 and 2
    for name in ("carry_5x37x130", "carry_5x37x200"):
        t = R.reference(name, *seen[name])
        assert t[0, 0].tolist() == [57, 17, 1, 37 * 36, 0, 18 * 18, 0, 0] and t[1, 1].tolist() == [70, 15, 0, 0, 37 * 31, 0, 16 * 16, 0]
        assert t[3, 0, :3].tolist() == [24, 17, 1] and t[3, 0, 5] == 15 * 15 and t[4, 2, 2] == 0
    assert R.reference("carry_5x37x200", *seen["carry_5x37x200"])[2, 2].tolist() == [135, 15, 1, 37 * 31, 0, 16 * 16, 0, 0]


def test_each_carry_defect_is_shown_by_the_slice_built_for_it():
    """which slice of the carry fixtures tells which broken carry of the row pass from the rule"""
    shown = {}
    for name, pred, gt, ids in (c for c in CASES if c[0].startswith("carry")):
        good = R.reference(name, pred, gt, ids)
        for defect in R.CARRY:
            bad = R.table(pred, gt, ids, defect=defect)
            shown.setdefault(defect, set()).update((name[-3:], int(d)) for d in np.unique(np.argwhere(bad != good)[:, 0]))
    assert {("130", 0), ("200", 0)} <= shown["next_w"] and {("130", 0), ("200", 0)} <= shown["next_chunk"]
    assert {("130", 1), ("200", 1)} <= shown["start_chunk"] and ("200", 2) in shown["start_stale"]


def test_u_to_k_and_the_union_order():
    pred, gt, ids = next(c[1:] for c in CASES if c[0] == "blobs_5x37x65")
    counts = R.reference("blobs_5x37x65", pred, gt, ids)[..., 3:5].sum(-1)
    choices = R.k_choices(counts, 3)
    t = {c: R.table(pred, gt, ids, "uniform", **{kind: tab}) for c, (kind, tab) in choices.items()}
    for a, b in (("u_zero", "first"), ("u_max", "last"), ("beyond", "last"), ("negative", "last")):
        assert np.array_equal(t[a], t[b]), (a, b)
    assert (t["first"][..., 5:7] == -1).all() and (t["first"][counts == 0][:, :3] == -1).all()
    for d, j in zip(*np.nonzero(counts)):
        fn, fp = R.regions(pred[d], gt[d], ids[j])
        for c in ("first", "last", "u_random", "inside"):
            x, y, label = t[c][d, j, :3]
            assert (fn | fp)[y, x] and label == int(fn[y, x])
        x, y, _ = t["first"][d, j, :3]
        assert (y, x) == tuple(np.argwhere(fn | fp)[0])
    assert R.k_from_u(2 ** 32 - 1, 5) == 4 and R.k_from_u(0, 5) == 0 and R.k_from_u(2 ** 31, 3) == 1


def test_worst_slices_on_cpu_tensors():
    from medical_sam2_amd.prompts import worst_slices
    errors = torch.tensor([[[1, 2], [0, 0], [0, 5]],
                           [[3, 0], [0, 0], [5, 0]],
                           [[0, 0], [0, 0], [2, 2]],
                           [[2, 1], [0, 0], [4, 1]]], dtype=torch.int32)               # [D = 4, n = 3, 2]
    assert worst_slices(errors).tolist() == [[0], [-1], [0]]                            # ties (3 = 3 = 3; 5 = 5 = 5) go to the lower slice
    assert worst_slices(errors, 3).tolist() == [[0, 1, 3], [-1, -1, -1], [0, 1, 3]]
    assert worst_slices(errors, 6).tolist() == [[0, 1, 3, -1, -1, -1], [-1] * 6, [0, 1, 3, 2, -1, -1]]
    assert worst_slices(errors, 2).dtype == torch.int64 and worst_slices(errors, 2).shape == (3, 2)
    rng = np.random.RandomState(0)
    e = rng.randint(0, 4, (9, 5, 2))
    got = worst_slices(torch.from_numpy(e), 4).numpy()
    total = e.sum(-1)
    for j in range(5):
        order = sorted((d for d in range(9) if total[d, j] > 0), key=lambda d: (-total[d, j], d))[:4]
        assert got[j].tolist() == order + [-1] * (4 - len(order))
    big = torch.zeros(3, 1, 2, dtype=torch.int32)
    big[2, 0, 0] = big[2, 0, 1] = 8192 * 8192 // 2                                      # the key does not overflow at a full slice
    assert worst_slices(big).tolist() == [[2]]


def test_argument_errors_cross_the_abi_as_codes():
    """the limits of msam2_label_error_clicks are refused on the host, before the device is touched, naming the entry"""
    from medical_sam2_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    ptr = (ctypes.addressof(buf) + 15) & ~15                 # a valid host address: never dereferenced by the checks
    ok = dict(pred=ptr, gt=ptr, ids=ptr, k=None, u=None, D=1, H=8, W=8, n=2, mode=0, clicks=ptr, ws=ptr, nb=1 << 20)

    def call(a):
        return L.msam2_label_error_clicks(a["pred"], a["gt"], a["ids"], a["k"], a["u"], a["D"], a["H"], a["W"], a["n"], a["mode"], a["clicks"],
                                          a["ws"], a["nb"], None)
    for what, kw in {"n = 0": dict(n=0), "n = 33": dict(n=33), "D 0 ": dict(D=0), "D 65536": dict(D=65536), "0x8": dict(H=0), "8193x8": dict(H=8193),
                     "8x0": dict(W=0), "8x8193": dict(W=8193), "2^31 - 2": dict(D=33, H=8192, W=8192), "null": dict(pred=None), "null ": dict(gt=None),
                     " null": dict(ids=None), "null  ": dict(clicks=None), "  null": dict(ws=None), "mode 2": dict(mode=2), "mode -1": dict(mode=-1),
                     "exactly one": dict(mode=1), "exactly one ": dict(mode=1, k=ptr, u=ptr), "neither": dict(k=ptr), "neither ": dict(u=ptr),
                     "too small": dict(nb=8 * 8 * 4 + 2 * 16 - 1), "too small ": dict(mode=1, k=ptr, nb=2 * 8 * 4 - 1),
                     "aligned": dict(ws=ptr + 4), "aligned ": dict(clicks=ptr + 2)}.items():
        rc = call(dict(ok, **kw))
        msg = L.msam2_last_error().decode()
        assert rc < 0, (what, rc)
        assert msg.startswith("label_error_clicks:") and what.strip() in msg, (what, msg)
    sizes = L.msam2_label_error_clicks_workspace_bytes
    assert sizes(1, 8, 8, 2, 0) == 8 * 8 * 4 + 2 * 16 and sizes(3, 8, 5, 2, 1) == 3 * 2 * 8 * 4
    assert sizes(0, 8, 8, 2, 0) == 0 and sizes(1, 8, 8, 33, 0) == 0 and sizes(1, 8, 8, 2, 2) == 0 and sizes(1, 8193, 8, 2, 1) == 0


def test_wrappers_refuse_bad_arguments():
    import medical_sam2_amd.ops as ops
    from medical_sam2_amd import prompts
    vol = torch.zeros(2, 8, 8, dtype=torch.uint8)
    for what, call in {
        "uint8": lambda: ops.label_error_clicks(vol.int(), vol, [1, 2]),
        "contiguous": lambda: ops.label_error_clicks(vol.transpose(1, 2), vol, [1, 2]),
        r"\[D, H, W\]": lambda: ops.label_error_clicks(vol[0], vol[0], [1, 2]),
        "distinct": lambda: ops.label_error_clicks(vol, vol, [4, 4]),
        "1 .. 32": lambda: ops.label_error_clicks(vol, vol, list(range(1, 34))),
        "on the GPU": lambda: ops.label_error_clicks(vol, vol, [1, 2]),
        "mode 'middle'": lambda: ops.label_error_clicks_workspace_bytes(1, 8, 8, 2, "middle"),
    }.items():
        with pytest.raises(ValueError, match=what.strip()):
            call()
    assert ops.CLICK_MODES == {"center": 0, "uniform": 1}
    with pytest.raises(ValueError, match="Mode not recognized"):
        prompts.corrective_clicks(vol, vol, [1], mode="middle")
    with pytest.raises(AssertionError, match="uint8"):
        prompts.corrective_clicks(vol.float(), vol, [1])
    with pytest.raises(AssertionError, match="one shape"):
        prompts.corrective_clicks(vol, vol[:1], [1])
    with pytest.raises(AssertionError, match="uniform"):
        prompts.corrective_clicks(vol, vol, [1], k=torch.zeros(2, 1, dtype=torch.int32))
