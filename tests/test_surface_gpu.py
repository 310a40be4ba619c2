"""msam2_label_edt / msam2_label_surface_distances, their ops wrappers and volume_labels.surface_scores on the MI355X.

Every squared distance has a definition down to the bit, so every d2 comparison is exact float64 equality with the brute-force
restatement (tests/surface_restate.py, itself checked against a neighbour loop and scipy in tests/test_surface_cpu.py), after sorting for the
batch entry; nothing is excluded.  The entries are called through the C ABI with the volumes inside 0xAB-padded buffers (also one byte off
any alignment) and d2, dist, counts and the workspace inside sentinel canvases of -7: an over-read would find 0xAB voxels, a stray store is
seen.

Borders of the kernels: a wave owns one row of the box 64 columns at a time (volumes of 100, 66 and 65 columns; boxes that start and end at
columns that are no multiples of 64, so the carry from chunk to chunk works in both sweeps), the column and z passes own 256 consecutive box
voxels per workgroup, so waves straddle rows and slices of every box here."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import surface_restate as R  # noqa: E402
from test_surface_cpu import check_scores  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64
ANISO = R.SPACINGS[1]


@pytest.fixture(autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with torch.no_grad():
        yield


def padded(x, fill, shift=0):
    """x inside a canvas of `fill`: (canvas, view of x's place).  shift: extra elements in front (1 = an unaligned label volume)."""
    canvas = torch.full((x.numel() + 2 * PAD + shift,), fill, dtype=x.dtype, device=DEV)
    view = canvas[PAD + shift: PAD + shift + x.numel()].view(x.shape)
    return canvas, view


def intact(canvas, view, fill):
    rest = torch.ones_like(canvas, dtype=torch.bool)
    start = (view.data_ptr() - canvas.data_ptr()) // canvas.element_size()
    rest[start: start + view.numel()] = False
    return bool((canvas[rest] == fill).all())


def device_volume(host, shift):
    host = np.array(host, dtype=np.uint8)                                 # a writable copy of the shared fixture
    can, vol = padded(torch.from_numpy(host), 0xAB, shift)
    vol.copy_(torch.from_numpy(host))
    return can, vol


def lib():
    import medical_sam2_amd.ops as ops
    from medical_sam2_amd import _lib
    return ops, _lib.lib()


def i32(values):
    import ctypes
    return (ctypes.c_int32 * len(values))(*[int(v) for v in values])


def i64(values):
    import ctypes
    return (ctypes.c_int64 * len(values))(*[int(v) for v in values])


def abi_edt(host, value, features, box, spacing, shift=0):
    """msam2_label_edt through the ABI -> float64 numpy of the box's shape"""
    ops, L = lib()
    D, H, W = host.shape
    bx = R.whole(host.shape) if box is None else box
    shape = (bx[1] - bx[0] + 1, bx[3] - bx[2] + 1, bx[5] - bx[4] + 1)
    vcan, vol = device_volume(host, shift)
    ocan, out = padded(torch.empty(shape, dtype=torch.float64), -7.0)
    nb = L.msam2_label_edt_workspace_bytes(*shape)
    assert nb == 10 * out.numel() + (-2 * out.numel()) % 8 + 4 * shape[0] + (-4 * shape[0]) % 8
    wcan, ws = padded(torch.empty(nb // 8, dtype=torch.int64), -7)
    torch.cuda.synchronize()
    rc = L.msam2_label_edt(ops._p(vol), D, H, W, int(value), {"surface": 0, "outside": 1}[features], None if box is None else i32(box),
                           spacing[0], spacing[1], spacing[2], ops._p(out), ops._p(ws), nb, ops._stream())
    assert rc == 0, L.msam2_last_error().decode()
    torch.cuda.synchronize()
    assert intact(ocan, out, -7.0) and intact(wcan, ws, -7) and intact(vcan, vol, 0xAB), "stray store"
    return out.cpu().numpy()


class Batch:
    """two volumes on the device and msam2_label_surface_distances on padded buffers; segments laid out one after the other, each with the
    capacity given (default: the organ's voxel count in the query volume)"""

    def __init__(self, pred, gt, ids, boxes, shift=0, stream=None, capacity=None):
        self.ops, self.L = lib()
        self.pred, self.gt, self.ids, self.boxes, self.stream = pred, gt, list(ids), [tuple(b) for b in boxes], stream
        self.n = len(self.ids)
        self.pcan, self.p = device_volume(pred, shift)
        self.gcan, self.g = device_volume(gt, 1 - shift)
        self.caps = capacity if capacity is not None else [[int((pred == v).sum()), int((gt == v).sum())] for v in self.ids]
        flat = [c for pair in self.caps for c in pair]
        self.offs = np.concatenate([[0], np.cumsum(flat)[:-1]]).reshape(self.n, 2)
        self.dcan, self.dist = padded(torch.empty(max(sum(flat), 1), dtype=torch.float64), -7.0)
        self.dist.fill_(-7.0)
        self.ccan, self.counts = padded(torch.empty(self.n, 2, dtype=torch.int32), -7)
        self.nb = self.L.msam2_label_surface_distances_workspace_bytes(i32([v for b in self.boxes for v in b]), self.n)
        assert self.nb > 0 and self.nb % 8 == 0
        self.wcan, self.ws = padded(torch.empty(self.nb // 8, dtype=torch.int64), -7)
        torch.cuda.synchronize()

    def run(self, spacing, sync=True):
        import ctypes
        p = self.ops._p
        s = self.ops._stream() if self.stream is None else self.stream.cuda_stream
        rc = self.L.msam2_label_surface_distances(p(self.p), p(self.g), *self.pred.shape, (ctypes.c_uint8 * self.n)(*self.ids),
                                                  i32([v for b in self.boxes for v in b]), i64(self.offs.reshape(-1)),
                                                  i32([c for pair in self.caps for c in pair]), self.n, spacing[0], spacing[1], spacing[2],
                                                  p(self.dist), self.dist.numel(), p(self.counts), p(self.ws), self.nb, s)
        assert rc == 0, self.L.msam2_last_error().decode()
        return self.result() if sync else None

    def result(self):
        """(counts int64 [n, 2], per organ and direction the sorted stored values, the rest of the segment)"""
        torch.cuda.synchronize()
        assert intact(self.dcan, self.dist, -7.0) and intact(self.ccan, self.counts, -7) and intact(self.wcan, self.ws, -7), "stray store"
        assert intact(self.pcan, self.p, 0xAB) and intact(self.gcan, self.g, 0xAB)
        counts, dist = self.counts.cpu().numpy().astype(np.int64), self.dist.cpu().numpy()
        segs = [[None, None] for _ in range(self.n)]
        for j in range(self.n):
            for d in range(2):
                a, cap, m = int(self.offs[j, d]), self.caps[j][d], int(counts[j, d])
                segs[j][d] = (np.sort(dist[a: a + min(m, cap)]), dist[a + min(m, cap): a + cap])
        return counts, segs


@functools.lru_cache(maxsize=None)
def fixture(name):
    pred, gt, ids = dict(R.cases())[name]
    pred.setflags(write=False), gt.setflags(write=False)
    return pred, gt, tuple(ids)


@functools.lru_cache(maxsize=None)
def batch_reference(name, spacing, boxes):
    """per organ the two sorted lists; computed once, shared, never written to"""
    pred, gt, ids = fixture(name)
    out = []
    for v, box in zip(ids, boxes):
        a, b = R.surface_distances(pred, gt, v, spacing, box)
        a.setflags(write=False), b.setflags(write=False)
        out.append((a, b))
    return out


def union_boxes(name):
    pred, gt, ids = fixture(name)
    return tuple(R.union_box(pred, gt, v) for v in ids)


# ---- the dense entry -------------------------------------------------------------------------------------------------------------------
def _dense_cases():
    S = (0, 8, 0, 32, 0, 99)
    big, small, flat, noise, wide = "shifted3_9x33x100", "specials_9x33x100", "shifted3_1x12x66", "noise_3x2x65", "wide_9x33x100"
    v3 = dict(R.cases())[big][2]
    vf = dict(R.cases())[flat][2]
    # (fixture, which volume, value, features, box or None)
    yield "organ_whole_default_box", (big, 1, v3[0], "surface", None)
    yield "organ_whole_box", (big, 0, v3[1], "surface", S)
    yield "wide_box_5_70", (wide, 1, 77, "surface", (1, 7, 3, 30, 5, 70))
    yield "wide_box_5_70_outside", (wide, 1, 77, "outside", (3, 5, 10, 22, 5, 70))
    yield "wide_box_63_64", (wide, 0, 77, "surface", (0, 8, 0, 32, 63, 64))
    yield "wide_box_64_99_outside", (wide, 0, 77, "outside", (2, 4, 12, 18, 64, 99))
    yield "wide_box_256_voxels", (wide, 1, 77, "surface", (0, 7, 0, 7, 0, 3))          # 64 rows, 256 voxels: whole workgroups in every launch
    yield "wide_one_row", (wide, 1, 77, "surface", (4, 4, 16, 16, 3, 99))
    yield "wide_one_row_outside", (wide, 1, 77, "outside", (4, 4, 13, 13, 3, 99))
    yield "wide_one_column_of_slices", (wide, 1, 77, "outside", (0, 8, 16, 16, 50, 50))
    yield "wide_inner_value", (wide, 1, 3, "surface", (0, 8, 0, 32, 20, 99))
    yield "three_faces", (small, 0, 40, "surface", None)
    yield "three_faces_outside_box", (small, 0, 40, "outside", (0, 5, 0, 9, 0, 12))
    yield "gaps_between_slices_and_rows", (small, 1, 30, "surface", None)
    yield "opposite_corner", (small, 1, 21, "surface", None)
    yield "single_voxel", (small, 0, 9, "surface", None)
    yield "tie", (small, 1, 6, "surface", (0, 4, 0, 12, 70, 90))
    yield "no_feature_absent_value", (small, 0, 123, "surface", None)
    yield "no_feature_box_inside_the_organ", (small, 0, 30, "outside", (2, 6, 12, 20, 41, 42))
    yield "no_surface_in_box_inside_the_organ", (small, 0, 30, "surface", (2, 6, 12, 20, 41, 42))
    yield "one_slice_whole", (flat, 1, vf[0], "surface", None)
    yield "one_slice_whole_outside", (flat, 0, vf[1], "outside", None)
    yield "one_slice_box", (flat, 1, vf[2], "surface", (0, 0, 1, 10, 1, 64))
    yield "two_rows_noise", (noise, 0, 2, "surface", None)
    yield "two_rows_noise_outside", (noise, 1, 1, "outside", None)
    yield "background_of_noise", (noise, 1, 0, "surface", (0, 2, 0, 1, 1, 64))


DENSE = dict(_dense_cases())


@pytest.mark.parametrize("name", list(DENSE))
def test_dense_transform_equals_the_restatement_through_the_abi(name):
    fx, which, value, features, box = DENSE[name]
    vol = fixture(fx)[which]
    bx = R.whole(vol.shape) if box is None else box
    feat = R.feature_mask(vol, value, features, bx)[R.box_slices(bx)]
    for k, spacing in enumerate(R.SPACINGS):
        want = R.edt(vol, value, spacing, features, box)
        got = abi_edt(vol, value, features, box, spacing, shift=k % 2)
        assert got.shape == want.shape and np.array_equal(got, want), (spacing, np.argwhere(got != want)[:4].tolist())
        if not feat.any():
            assert np.isposinf(got).all()
        elif k == 0:                                                       # unit spacing: the integers of scipy's index output
            _, idx = ndimage.distance_transform_edt(~feat, return_indices=True)
            ints = sum((idx[a] - np.indices(feat.shape)[a]).astype(np.int64) ** 2 for a in range(3))
            assert np.array_equal(got, ints.astype(np.float64))
    if name.startswith("no_"):
        assert not feat.any()


def test_dense_outside_mode_on_the_whole_volume_equals_scipy_at_unit_spacing():
    """the classic in-mask distance over all of [9, 33, 100], where the brute force would take too long: exact integers"""
    for fx, which in (("shifted3_9x33x100", 1), ("specials_9x33x100", 0)):
        pred_gt_ids = fixture(fx)
        vol, value = pred_gt_ids[which], pred_gt_ids[2][0]
        got = abi_edt(vol, value, "outside", None, (1.0, 1.0, 1.0), shift=1)
        _, idx = ndimage.distance_transform_edt(vol == value, return_indices=True)
        ints = sum((idx[a] - np.indices(vol.shape)[a]).astype(np.int64) ** 2 for a in range(3))
        assert np.array_equal(got, ints.astype(np.float64)) and (got > 0).sum() == (vol == value).sum() > 0


# ---- the batch entry -------------------------------------------------------------------------------------------------------------------
def check_batch(got, want, where):
    counts, segs = got
    for j, (a, b) in enumerate(want):
        assert counts[j].tolist() == [len(a), len(b)], (where, j, counts[j].tolist(), len(a), len(b))
        for d, ref in enumerate((a, b)):
            stored, rest = segs[j][d]
            assert np.array_equal(stored, ref), (where, j, d, stored[:4], ref[:4])
            assert (rest == -7.0).all(), (where, j, d, "a store past the count")


@pytest.mark.parametrize("name", [n for n, _ in R.cases()])
def test_surface_distances_equal_the_restatement_through_the_abi(name):
    pred, gt, ids = fixture(name)
    assert len(ids) == 1 or list(ids) != sorted(ids), "ids in non-ascending order"
    boxes = union_boxes(name)
    for shift in (0, 1):
        run = Batch(pred, gt, ids, boxes, shift)
        for spacing in R.SPACINGS:
            check_batch(run.run(spacing), batch_reference(name, spacing, boxes), (name, shift, spacing))


def test_one_three_and_thirty_two_organs():
    sizes = {name: len(fixture(name)[2]) for name in ("shifted1_1x12x66", "shifted3_9x33x100", "shifted32_9x33x100")}
    assert sorted(sizes.values()) == [1, 3, 32]


def test_the_special_organs_are_what_they_claim():
    pred, gt, ids = fixture("specials_9x33x100")
    boxes = union_boxes("specials_9x33x100")
    counts, segs = Batch(pred, gt, ids, boxes).run(ANISO)
    at = {v: j for j, v in enumerate(ids)}
    assert counts[at[8]].tolist() == [int(R.surface(pred, 8).sum()), 0] and counts[at[7]].tolist() == [0, int(R.surface(gt, 7).sum())]
    assert np.isposinf(segs[at[8]][0][0]).all() and len(segs[at[7]][0][0]) == 0       # absent features: +inf; absent queries: nothing
    assert segs[at[5]][0][0].tolist() == [np.float64(0.76) * np.float64(0.76) * 4.0]   # two columns away, not one slice away
    assert segs[at[6]][0][0].tolist() == [np.float64(0.76) * np.float64(0.76) * 9.0]   # the tie
    assert counts[at[9]].tolist() == [1, 1] and segs[at[9]][0][0].tolist() == segs[at[9]][1][0].tolist()
    far = R.surface_distances(pred, gt, 20, ANISO)[0]
    assert segs[at[20]][0][0].tolist() == far.tolist() and far.min() > 8 * 8 * 9.0     # opposite corners: the scans run their full length


def test_boxes_cut_queries_and_features():
    """whole-volume boxes give what the union boxes give; a box through the organs cuts both surfaces (which stay surfaces of the volume)"""
    name = "shifted3_9x33x100"
    pred, gt, ids = fixture(name)
    whole = tuple(R.whole(pred.shape) for _ in ids)
    cut = ((1, 4, 3, 18, 2, 9), (0, 8, 9, 9, 0, 99), (5, 7, 20, 32, 25, 30))
    full = ((0, 7, 8, 23, 10, 25), (0, 7, 0, 7, 0, 3), (0, 7, 8, 23, 10, 25))          # the largest: 2048 voxels, one whole workgroup of the z pass
    for boxes in (whole, cut, full):
        run = Batch(pred, gt, ids, boxes, shift=1)
        for spacing in R.SPACINGS[:2]:
            check_batch(run.run(spacing), batch_reference(name, spacing, boxes), (boxes, spacing))
    assert all(np.array_equal(a, b) for x, y in zip(batch_reference(name, ANISO, whole), batch_reference(name, ANISO, union_boxes(name)))
               for a, b in zip(x, y))


def test_a_segment_that_is_too_small_is_counted_and_not_overrun():
    name = "shifted3_9x33x100"
    pred, gt, ids = fixture(name)
    boxes = union_boxes(name)
    want = batch_reference(name, ANISO, boxes)
    caps = [[max(len(a) // 2, 1), len(b)] for a, b in want]
    caps[1] = [0, 3]
    counts, segs = Batch(pred, gt, ids, boxes, capacity=caps).run(ANISO)          # result(): the canvases around dist are intact
    for j, (a, b) in enumerate(want):
        assert counts[j].tolist() == [len(a), len(b)]
        for d, ref in enumerate((a, b)):
            stored, rest = segs[j][d]
            assert len(stored) == min(caps[j][d], len(ref))                 # all of them written: none is the sentinel (below)
            assert (rest == -7.0).all()
            assert np.isin(stored, ref).all()
    assert np.array_equal(segs[0][1][0], want[0][1])


def test_second_run_beside_other_work_gives_the_same_bits():
    name = "shifted32_9x33x100"
    pred, gt, ids = fixture(name)
    boxes = union_boxes(name)
    side = torch.cuda.Stream()
    first = Batch(pred, gt, ids, boxes).run(ANISO)
    again = Batch(pred, gt, ids, boxes, shift=1, stream=side)
    noise = fixture("noise_4x9x70")
    other = Batch(noise[0], noise[1], noise[2], union_boxes("noise_4x9x70"))
    x = torch.randn(512, 512, device=DEV)
    for _ in range(3):                                                              # the two streams' workgroups share the device
        other.run(R.SPACINGS[2], sync=False)
        x = x @ x * 1e-3
        with torch.cuda.stream(side):                                               # the re-fill is ordered with the run that overwrites it
            again.dist.fill_(-7.0)
        again.run(ANISO, sync=False)
    second = again.result()
    check_batch(second, batch_reference(name, ANISO, boxes), "second stream")
    assert np.array_equal(first[0], second[0])
    assert all(a[d][0].tobytes() == b[d][0].tobytes() for a, b in zip(first[1], second[1]) for d in range(2))
    check_batch(other.result(), batch_reference("noise_4x9x70", R.SPACINGS[2], union_boxes("noise_4x9x70")), "noise")


# ---- the wrappers ----------------------------------------------------------------------------------------------------------------------
def test_label_edt_wrapper():
    import medical_sam2_amd.ops as ops
    pred, gt, ids = fixture("shifted3_9x33x100")
    labels = torch.from_numpy(np.array(gt)).to(DEV)
    for features, box in (("surface", None), ("outside", (1, 7, 3, 30, 5, 70))):
        got = ops.label_edt(labels, ids[0], ANISO, features, box)
        want = R.edt(gt, ids[0], ANISO, features, box)
        assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(ops.label_edt(labels, ids[0]).cpu().numpy(), R.edt(gt, ids[0], (1.0, 1.0, 1.0)))
    for bad in (dict(box=(0, 9, 0, 32, 0, 99)), dict(box=(3, 2, 0, 32, 0, 99)), dict(spacing=(1.0, 0.0, 1.0)), dict(features="inside")):
        with pytest.raises(ValueError, match="label_edt"):
            ops.label_edt(labels, ids[0], **bad)
    with pytest.raises(ValueError, match="at least 2"):
        ops.label_edt(labels[:, :1].contiguous(), ids[0])


def test_label_surface_distances_wrapper():
    import medical_sam2_amd.ops as ops
    name = "specials_9x33x100"
    pred, gt, ids = fixture(name)
    p, g = torch.from_numpy(np.array(pred)).to(DEV), torch.from_numpy(np.array(gt)).to(DEV)
    dist, offs, caps, counts = ops.label_surface_distances(p, g, list(ids), ANISO)
    assert dist.is_cuda and dist.dtype == torch.float64 and counts.is_cuda and counts.dtype == torch.int32
    assert offs.is_cuda and offs.dtype == torch.int64 and caps.is_cuda and caps.dtype == torch.int32 and offs.shape == caps.shape == (len(ids), 2)
    offs, caps = offs.cpu(), caps.cpu()
    want = batch_reference(name, ANISO, union_boxes(name))
    dist, counts = dist.cpu().numpy(), counts.cpu().numpy()
    for j, v in enumerate(ids):
        absent = not (pred == v).any() or not (gt == v).any()
        assert caps[j].tolist() == ([0, 0] if absent else [int((pred == v).sum()), int((gt == v).sum())])
        assert counts[j].tolist() == [len(want[j][0]), len(want[j][1])]
        for d in range(2):
            seg = np.sort(dist[int(offs[j, d]): int(offs[j, d]) + int(caps[j, d])])
            if not absent:
                assert np.array_equal(seg[: counts[j, d]], want[j][d]) and np.isposinf(seg[counts[j, d]:]).all()
    assert int(caps.sum()) == len(dist)
    same = ops.label_surface_distances(p, g, ops.label_ids(list(ids), DEV), ANISO)                       # the ids as a device tensor
    assert torch.equal(same[3].cpu(), torch.from_numpy(counts)) and torch.equal(same[1].cpu(), offs)
    with pytest.raises(ValueError, match="gt must be uint8"):
        ops.label_surface_distances(p, g[:-1].contiguous(), list(ids))


@pytest.mark.parametrize("name", ["shifted3_9x33x100", "shifted32_9x33x100", "specials_9x33x100", "shifted3_1x12x66"])
def test_surface_scores_equal_the_restatement(name):
    """bars as in tests/test_surface_cpu.py: hd, the nsd counts and surface_voxels exactly, hd95 and assd to 1e-12 relative"""
    from medical_sam2_amd.volume_labels import surface_scores
    pred, gt, ids = fixture(name)
    p, g = torch.from_numpy(np.array(pred)).to(DEV), torch.from_numpy(np.array(gt)).to(DEV)
    boxes = union_boxes(name)
    for spacing, pct, tol in ((R.SPACINGS[1], 95.0, (1.0,)), (R.SPACINGS[2], 95.0, (0.5, 1.0, 3.0)), (R.SPACINGS[1], 50.0, (2.28,))):
        lists = batch_reference(name, spacing, boxes)
        want = R.scores(lists, pct, tol)
        got = surface_scores(p, g, list(ids), spacing, pct, tol)
        check_scores(got, want, f"{name} {spacing} {pct} {tol}")
        assert got["nsd"].shape == (len(ids), len(tol))
    if name == "specials_9x33x100":
        at = {v: j for j, v in enumerate(ids)}
        assert np.isnan(got["hd"][at[8]]) and np.isnan(got["hd95"][at[7]]) and np.isnan(got["nsd"][at[8]]).all() and not np.isnan(got["hd"][at[9]])
        assert got["surface_voxels"][at[8]].tolist() == [int(R.surface(pred, 8).sum()), 0]


def test_surface_scores_in_several_organ_groups_have_the_same_bits():
    import medical_sam2_amd.ops as ops
    from medical_sam2_amd import _lib
    from medical_sam2_amd.volume_labels import surface_scores
    name = "shifted32_9x33x100"
    pred, gt, ids = fixture(name)
    p, g = torch.from_numpy(np.array(pred)).to(DEV), torch.from_numpy(np.array(gt)).to(DEV)
    need = [_lib.lib().msam2_label_surface_distances_workspace_bytes(i32(b), 1) for b in union_boxes(name)]
    assert sum(need) > 3 * max(need)                                                                    # max(need): at least three groups
    one = surface_scores(p, g, list(ids), ANISO, 95.0, (1.0, 2.0))
    for budget in (max(need), max(need) + min(need), sum(need) - 1):
        many = surface_scores(p, g, list(ids), ANISO, 95.0, (1.0, 2.0), workspace_bytes=budget)
        assert sorted(one) == sorted(many) and all(np.asarray(one[k]).tobytes() == np.asarray(many[k]).tobytes() for k in one), budget
        a, b = ops.surface_segments(p, g, list(ids), ANISO), ops.surface_segments(p, g, list(ids), ANISO, budget)
        assert torch.equal(a[3], b[3]) and a[1] == b[1] and a[2] == b[2]
        for j in range(len(ids)):
            for d in range(2):
                lo, hi = a[1][j][d], a[1][j][d] + a[2][j][d]
                assert torch.equal(torch.sort(a[0][lo:hi]).values, torch.sort(b[0][lo:hi]).values)
    with pytest.raises(ValueError, match=f"needs a workspace of {max(need)} bytes"):
        surface_scores(p, g, list(ids), ANISO, workspace_bytes=max(need) - 1)
