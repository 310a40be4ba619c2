"""msam2_instance_remap / _apply / _pairs / _paint, their ops wrappers, instances.instance_scores and volume_labels.lesion_scores on the MI355X.

Every table is an integer with a canonical definition, so every comparison is exact equality with the brute-force restatement
(tests/instances_restate.py, itself held against the reference's results in tests/test_instances_cpu.py), nothing excluded.  The entries
are called through the C ABI with the maps inside buffers padded with an out-of-range id (an over-read would be counted in info) and every
output inside a sentinel canvas of -7 that is checked intact (a stray store is seen).

Borders of the kernels: a wave owns 64 consecutive voxels in raster order through the whole volume, a workgroup 4 rounds of 256, so runs are
cut at linear indices that are multiples of 64, 256 and 1024; the scans go through tiles of 1024 items, 256 tiles per trip of the second
level; the flat fill takes a second trip beyond 2048 x 256 elements."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import instances_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64
FAR = 0x7F7F7F7F                                             # the padding of the maps: an id outside every range used here


@pytest.fixture(autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with torch.no_grad():
        yield


@pytest.fixture(scope="module")
def G():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "instances_cases.npz")))


def padded(x, fill):
    """a copy of the host tensor x inside a device canvas of `fill`: (canvas, view of x's place)"""
    canvas = torch.full((x.numel() + 2 * PAD,), fill, dtype=x.dtype, device=DEV)
    view = canvas[PAD: PAD + x.numel()].view(x.shape)
    view.copy_(x)
    return canvas, view


def sentinel(shape, dtype=torch.int32):
    canvas = torch.full((int(np.prod(shape)) + 2 * PAD,), -7, dtype=dtype, device=DEV)
    return canvas, canvas[PAD: PAD + int(np.prod(shape))].view(shape)


def intact(canvas, view, fill=-7):
    rest = torch.ones_like(canvas, dtype=torch.bool)
    start = (view.data_ptr() - canvas.data_ptr()) // canvas.element_size()
    rest[start: start + view.numel()] = False
    return bool((canvas[rest] == fill).all())


def lib():
    import medical_sam2_amd.ops as ops
    from medical_sam2_amd import _lib
    return ops, _lib.lib()


def dims(shape):
    return (1, *shape) if len(shape) == 2 else tuple(shape)


def np64(t):
    return t.cpu().numpy().astype(np.int64)


def abi_remap(m, id_bound, cap, labels=None, in_place=False, stream=None):
    """-> (out, orig, size, cls, info) as int64 numpy, sentinels and paddings checked"""
    ops, L = lib()
    p = ops._p
    D, H, W = dims(m.shape)
    mcan, md = padded(torch.from_numpy(np.ascontiguousarray(m, dtype=np.int32)), FAR)
    lcan = ld = None
    if labels is not None:
        lcan, ld = padded(torch.from_numpy(np.ascontiguousarray(labels, dtype=np.uint8)), 0xAB)
    ocan, out = (mcan, md) if in_place else sentinel(m.shape)
    tabs = [sentinel((cap,)) for _ in range(3)] + [sentinel((4,))]
    nb = L.msam2_instance_remap_workspace_bytes(id_bound)
    assert nb > 0
    ws = torch.empty(nb // 4, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    rc = L.msam2_instance_remap(p(md), p(ld), D, H, W, id_bound, p(out), p(tabs[0][1]), p(tabs[1][1]), p(tabs[2][1]), cap, p(tabs[3][1]), p(ws), nb,
                                ops._stream() if stream is None else stream.cuda_stream)
    assert rc == 0, L.msam2_last_error().decode()
    torch.cuda.synchronize()
    assert intact(ocan, out, FAR if in_place else -7) and all(intact(c, v) for c, v in tabs), "stray store"
    assert in_place or intact(mcan, md, FAR)
    assert lcan is None or intact(lcan, ld, 0xAB)
    return (np64(out),) + tuple(np64(v) for _, v in tabs)


def check_remap(m, id_bound, cap, labels=None, in_place=False):
    out, orig, size, cls, info = abi_remap(m, id_bound, cap, labels, in_place)
    r_out, r_orig, r_size, r_cls, r_bad = R.remap(m, id_bound, labels)
    n = len(r_orig)
    assert info.tolist() == [n, r_bad, int(n > cap), 0]
    assert np.array_equal(out, r_out)
    k = min(n, cap)
    for got, want in ((orig, r_orig), (size, r_size), (cls, r_cls)):
        assert np.array_equal(got[:k], want[:k]) and not got[k:].any()
    return n


def abi_pairs(a, b, na, nb, cap, stream=None):
    """-> (pairs, area_a, area_b, info) as int64 numpy"""
    ops, L = lib()
    p = ops._p
    D, H, W = dims(a.shape)
    acan, ad = padded(torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)), FAR)
    bcan, bd = padded(torch.from_numpy(np.ascontiguousarray(b, dtype=np.int32)), FAR)
    tabs = [sentinel((cap, 3)), sentinel((na,)), sentinel((nb,)), sentinel((4,))]
    need = L.msam2_instance_pairs_workspace_bytes(na, cap)
    assert need > 0 and need % 8 == 0
    wcan, ws = sentinel((need // 8,), torch.int64)
    torch.cuda.synchronize()
    rc = L.msam2_instance_pairs(p(ad), p(bd), D, H, W, na, nb, p(tabs[0][1]), cap, p(tabs[1][1]), p(tabs[2][1]), p(tabs[3][1]), p(ws), need,
                                ops._stream() if stream is None else stream.cuda_stream)
    assert rc == 0, L.msam2_last_error().decode()
    torch.cuda.synchronize()
    assert all(intact(c, v) for c, v in tabs) and intact(wcan, ws) and intact(acan, ad, FAR) and intact(bcan, bd, FAR), "stray store"
    return tuple(np64(v) for _, v in tabs)


def check_pairs(a, b, na, nb, cap=None):
    rows, area_a, area_b, bad_a, bad_b = R.pairs(a, b, na, nb)
    cap = max(1, len(rows)) if cap is None else cap          # the exact count must fit
    pairs, ga, gb, info = abi_pairs(a, b, na, nb, cap)
    assert np.array_equal(ga, area_a) and np.array_equal(gb, area_b)
    if len(rows) > cap:
        assert info.tolist() == [0, 1, bad_a, bad_b] and not pairs.any()
    else:
        assert info.tolist() == [len(rows), 0, bad_a, bad_b]
        assert np.array_equal(pairs[: len(rows)], rows) and not pairs[len(rows):].any()
    return len(rows)


# ---- shapes -----------------------------------------------------------------------------------------------------------------------------
def stripes(cuts_a, cuts_b, shape=(9, 33, 100)):
    """two maps whose ids change along the raster order at the given linear indices"""
    n = int(np.prod(shape))
    a = np.searchsorted(np.asarray(cuts_a), np.arange(n), side="right").astype(np.int32)
    b = np.searchsorted(np.asarray(cuts_b), np.arange(n), side="right").astype(np.int32)
    return a.reshape(shape), b.reshape(shape)


@functools.lru_cache(maxsize=None)
def cells(shape=(2, 256, 320), seed=3):
    """about 300 instances per map: two shifted grids of cells with a tenth of them background, b with one instance merged over many cells"""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    a = (z * 12 + y // 22) * 14 + x // 23 + 1
    b = (z * 14 + (y + 7) // 19) * 11 + (x + 5) // 31 + 1
    for m in (a, b):
        ids = np.unique(m)
        m[np.isin(m, rng.choice(ids, len(ids) // 10, replace=False))] = 0
    b[:, 100:180, 40:300][b[:, 100:180, 40:300] > 0] = 1     # one pred over dozens of true instances
    return R.remap(a)[0].astype(np.int32), R.remap(b)[0].astype(np.int32)


def map_pairs(G):
    out = {n: (R.remap(G[f"{n}_true"])[0], R.remap(G[f"{n}_pred"])[0]) for n in ("a", "b", "c", "d", "e", "g", "h")}
    out["cuts_64_256_1024"] = stripes([64, 256, 1024, 5000], [64, 300, 1024, 20000])       # the key changes exactly at 64, 256 and 1024
    a, b = stripes([10, 2000], [3000])
    out["one_run_over_the_cuts"] = (np.where(a == 1, 5, 0).astype(np.int32), np.where(b == 0, 1, 0).astype(np.int32))
    out["w53_runs_across_row_ends"] = stripes([40, 200, 211, 1500], [100, 212, 1400], (3, 21, 53))
    out["cells_300"] = cells()
    return out


# ---- remap and apply ----------------------------------------------------------------------------------------------------------------------
def test_remap_equals_the_restatement(G):
    rng = np.random.default_rng(5)
    for name in ("a", "b", "d", "f"):                        # ids 3k + 2 and a merged id; a map without instances among them
        for side in ("true", "pred"):
            m = G[f"{name}_{side}"]
            check_remap(m, 256, 64)
            assert np.array_equal(abi_remap(m, m.size + 1, 64)[0], G[f"{name}_remap_{side}"])
    for name, (a, b) in map_pairs(G).items():
        if name in ("a", "b", "c", "d", "e", "g", "h"):
            continue
        for m in (a, b):
            names = np.r_[0, rng.choice(np.arange(1, 99990), int(m.max()), replace=False)].astype(np.int32)     # random ids
            labels = (1 + (np.arange(m.size).reshape(m.shape) // 7) % 5).astype(np.uint8)
            assert check_remap(names[m], 100000, 512, labels) == len(np.unique(m)) - 1


def test_remap_ignores_ids_outside_the_bound_and_stops_at_cap():
    m = stripes([64, 256, 1024, 5000], [7])[0] * 10
    m[2, 3, 4:9], m[5, 0, 0], m[8, 32, 99] = -3, 41, 2 ** 31 - 1
    assert check_remap(m, 41, 8) == 4                        # 40 is inside the bound, 41 and the others are not
    assert check_remap(m, 42, 3) == 5                        # more instances than rows: the first three, flagged
    assert check_remap(m, 42, 5, in_place=True) == 5


def test_remap_second_trip_of_the_scan_and_of_the_fill():
    m = stripes([64, 256, 1024, 5000], [7], (2, 33, 100))[0].astype(np.int64) * 2_249_999      # ids up to 8 999 996
    m[1, 2, 3] = 8_999_999
    assert check_remap(m, 9_000_000, 600_000) == 5           # 281 250 bitmap words: 275 tiles, two trips; tables beyond 524 288 rows


def test_remap_of_label_components_with_classes():
    ops, _ = lib()
    rng = np.random.default_rng(11)
    vol = (rng.random((5, 40, 53)) < 0.35).astype(np.uint8) * rng.integers(1, 4, (5, 40, 53)).astype(np.uint8)
    comp, _ = ops.label_components(torch.from_numpy(vol).to(DEV), 6)
    comp = comp.cpu().numpy()
    n = check_remap(comp, comp.size + 1, 4096, vol)
    out, orig, size, cls, info = abi_remap(comp, comp.size + 1, 4096, vol)
    assert n > 100 and all(vol.reshape(-1)[orig[k] - 1] == cls[k] for k in range(n))      # the class is the value at the canonical voxel


def test_apply_in_place_and_out_of_range():
    ops, L = lib()
    m = stripes([64, 256, 1024, 5000], [7], (3, 21, 53))[0]
    m[1, 1, 1], m[2, 2, 2] = -1, 5
    table = np.array([0, 9, 0, 7, 3], dtype=np.int32)
    want = np.where((m >= 0) & (m <= 4), table[np.clip(m, 0, 4)], 0)
    mcan, md = padded(torch.from_numpy(m), FAR)
    tcan, td = padded(torch.from_numpy(table), FAR)
    ocan, out = sentinel(m.shape)
    assert L.msam2_instance_apply(ops._p(md), ops._p(td), 4, m.size, ops._p(out), ops._stream()) == 0
    assert L.msam2_instance_apply(ops._p(md), ops._p(td), 4, m.size, ops._p(md), ops._stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(np64(out), want) and np.array_equal(np64(md), want)
    assert intact(ocan, out) and intact(mcan, md, FAR) and intact(tcan, td, FAR)
    assert torch.equal(ops.instance_apply(torch.from_numpy(m).to(DEV), torch.from_numpy(table).to(DEV)), out)


# ---- pairs --------------------------------------------------------------------------------------------------------------------------------
def test_pairs_equal_the_restatement_at_the_exact_cap_and_overflow_below_it(G):
    for name, (a, b) in map_pairs(G).items():
        na, nb = max(1, int(a.max())), max(1, int(b.max()))
        n = check_pairs(a, b, na, nb)
        if n > 1:
            check_pairs(a, b, na, nb, n - 1)                  # one row short: flagged, no row written, the sentinels intact
        if name == "cells_300":
            assert n > 600 and np.bincount(R.pairs(a, b, na, nb)[0][:, 1]).max() > 30
            check_pairs(a, b, na + 7, nb + 1, 4 * n)          # roomy tables


def test_pairs_ignore_ids_outside_the_range():
    a, b = stripes([64, 256, 1024, 5000], [64, 300, 1024, 20000])
    a, b = a.copy(), b.copy()
    a[0, 0, 3:6], a[4, 4, 4], b[0, 0, 5], b[8, 32, 99] = 9, -1, -2 ** 31, 5
    assert check_pairs(a, b, 4, 4) >= 5
    assert check_pairs(a, b, 3, 2) >= 2                       # the instances above na / nb are background now, and counted


def test_pairs_second_trip_of_the_scan_and_of_the_fill():
    a, b = stripes([64, 256, 1024, 5000], [64, 300, 1024, 20000], (2, 33, 100))
    a = (a.astype(np.int64) * 74_999).astype(np.int32)       # ids up to 299 996 of na = 300 000: 293 tiles, two trips
    assert check_pairs(a, b, 300_000, 5, 200_000) >= 5       # 600 000 ints of pair rows: beyond one trip of the fill


def test_python_raises_on_overflow_and_on_ids_outside(G):
    import medical_sam2_amd.instances as I
    t, p = (torch.from_numpy(G[f"a_{s}"]).to(DEV) for s in ("true", "pred"))
    n = len(R.tables(G["a_true"], G["a_pred"])[0])
    rows, at, ap, _, _ = I.instance_tables(t, p, max_pairs=n)
    ref = R.tables(G["a_true"], G["a_pred"])
    assert np.array_equal(rows, ref[0]) and np.array_equal(at, ref[1]) and np.array_equal(ap, ref[2])
    with pytest.raises(ValueError, match="max_pairs"):
        I.instance_tables(t, p, max_pairs=n - 1)
    with pytest.raises(ValueError, match="max_instances"):
        I.instance_tables(t, p, max_instances=len(ref[1]) - 1)
    with pytest.raises(ValueError, match="outside"):
        I.instance_tables(t - 1, p)


# ---- paint --------------------------------------------------------------------------------------------------------------------------------
def abi_paint(masks, order=None, boxes=None, skip=True):
    ops, L = lib()
    p = ops._p
    n, H, W = masks.shape
    mcan, md = padded(torch.from_numpy(masks), 0xAB)
    od = None if order is None else padded(torch.tensor(order, dtype=torch.int32), FAR)[1]
    bd = None if boxes is None else padded(torch.tensor(boxes, dtype=torch.int32), FAR)[1]
    ocan, out = sentinel((H, W))
    nb = L.msam2_instance_paint_workspace_bytes(n)
    wcan, ws = sentinel((nb // 4,))
    rc = L.msam2_instance_paint(p(md), n, H, W, p(od), p(bd), int(skip), p(out), p(ws), nb, ops._stream())
    assert rc == 0, L.msam2_last_error().decode()
    torch.cuda.synchronize()
    assert intact(ocan, out) and intact(wcan, ws) and intact(mcan, md, 0xAB), "stray store"
    return np64(out)


def test_paint_covered_empty_and_overwriting_masks():
    rng = np.random.default_rng(2)
    H, W = 37, 53                                            # two workgroups, rows that are no multiple of the wave
    masks = np.zeros((9, H, W), dtype=np.uint8)
    masks[0, 2:20, 3:30] = 1
    masks[1, 5:10, 5:12] = 255                               # inside mask 0: skipped
    masks[3, 15:30, 20:50] = 1                               # (mask 2 is empty) sees zeros: overwrites a corner of 0
    masks[4, 2:30, 3:50] = 1                                 # sees zeros between 0 and 3: overwrites both entirely
    masks[5, 4:8, 4:8] = 1                                   # covered by 4
    masks[6] = rng.random((H, W)) < 0.02
    masks[7, 36, 52] = 1                                     # the last pixel
    masks[8] = masks[6]                                      # covered by 6 (if 6 was painted)
    boxes = [[0, 0, W - 1, H - 1]] * 9
    boxes[4] = [10, 5, 40, 25]                               # mask 4 cut to a box: 0 and 3 keep what lies outside it
    boxes[6] = [0, 0, 25, 36]
    boxes[8] = [20, 0, 52, 36]                               # 8 reaches beyond 6's box: painted
    order = [7, 4, 0, 1, 9, -1, 3, 8, 6]                     # two positions name no mask
    for o in (None, order):
        for b in (None, boxes):
            for skip in (True, False):
                got, want = abi_paint(masks, o, b, skip), R.paint(masks, o, b, skip)
                assert np.array_equal(got, want), (o, b is not None, skip)
    assert set(np.unique(R.paint(masks)).tolist()) == {0, 5, 7, 8}                 # 2, 3, 6, 9 skipped; 1 and 4 painted over
    assert set(np.unique(R.paint(masks, None, boxes)).tolist()) == {0, 1, 4, 5, 7, 8, 9}
    import medical_sam2_amd.instances as I
    assert np.array_equal(np64(I.paint_instances(torch.from_numpy(masks).to(DEV) != 0, order, boxes)), R.paint(masks, order, boxes))


# ---- streams and graphs -------------------------------------------------------------------------------------------------------------------
def test_relaunch_beside_another_streams_work_gives_the_same_bytes():
    a, b = cells()
    na, nb = int(a.max()), int(b.max())
    n = len(R.pairs(a, b, na, nb)[0])
    first = abi_pairs(a, b, na, nb, n)
    first_r = abi_remap(a * 3, 3 * na + 1, 512)
    side = torch.cuda.Stream()
    busy = torch.randn(1024, 1024, device=DEV)
    with torch.cuda.stream(side):
        for _ in range(20):
            busy = busy @ busy * 1e-3
    main = torch.cuda.Stream()
    again = abi_pairs(a, b, na, nb, n, stream=main)
    again_r = abi_remap(a * 3, 3 * na + 1, 512, stream=main)
    torch.cuda.synchronize()
    assert all(np.array_equal(x, y) for x, y in zip(first + first_r, again + again_r))


def test_graph_capture_of_pairs_with_caller_owned_tables(G):
    ops, _ = lib()
    a0, b0 = map_pairs(G)["cuts_64_256_1024"]
    a1, b1 = b0[::-1].copy(), a0[:, ::-1].copy()             # other contents of the same buffers
    na = nb = 5
    a, b = torch.from_numpy(a0).to(DEV), torch.from_numpy(b0).to(DEV)
    cap = 64
    ws = ops.instance_pairs_workspace(na, cap, a.device)
    out = ops.instance_pairs(a, b, na, nb, cap, workspace=ws)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        same = ops.instance_pairs(a, b, na, nb, cap, out=out, workspace=ws)
    assert all(x is y for x, y in zip(same, out))
    for x, y in ((a1, b1), (a0, b0)) * 2:
        a.copy_(torch.from_numpy(x).to(DEV))
        b.copy_(torch.from_numpy(y).to(DEV))
        for t in out:
            t.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        rows, ra, rb, _, _ = R.pairs(x, y, na, nb)
        assert np64(out[3]).tolist() == [len(rows), 0, 0, 0]
        assert np.array_equal(np64(out[0])[: len(rows)], rows) and not np64(out[0])[len(rows):].any()
        assert np.array_equal(np64(out[1]), ra) and np.array_equal(np64(out[2]), rb)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def test_instance_scores_on_the_golden_maps_equal_the_reference(G):
    import medical_sam2_amd.instances as I
    for name in ("a", "b", "c", "d", "e", "f", "g", "h"):
        t, p = (torch.from_numpy(G[f"{name}_{s}"]).to(DEV) for s in ("true", "pred"))
        for thr, tag in ((0.5, "pq05"), (0.3, "pq03")):
            assert R.golden_mismatches(I.instance_scores(t, p, thr), G, name, tag) == [], (name, tag)
        for side, m in (("true", t), ("pred", p)):
            out, orig, size, _, info = I.remap_instances(m, by_size=True)
            assert np.array_equal(np64(out), G[f"{name}_bysize_{side}"])
            n = int(info[0])
            assert np.array_equal(np64(size)[:n], R.remap(G[f"{name}_{side}"], by_size=True)[2])
    t, p = (torch.from_numpy(G[f"a_{s}"]).to(DEV) for s in ("true", "pred"))
    lt, lp = (torch.from_numpy(G[f"cls_labels_{s}"]).to(DEV) for s in ("true", "pred"))
    got = I.instance_scores(t, p, 0.5, lt, lp)
    assert R.golden_mismatches(got, G, "clsall", "pq05") == [] and sorted(got["per_class"]) == [1, 2]
    for c in (1, 2):
        assert abs(got["per_class"][c]["pq"] - G[f"cls{c}_pq05"][2]) <= 1e-12 * G[f"cls{c}_pq05"][2]


def test_lesion_scores_found_missed_spurious_and_merged():
    from medical_sam2_amd.volume_labels import lesion_scores
    gt = np.zeros((6, 40, 48), dtype=np.uint8)
    pred = np.zeros_like(gt)

    def box(vol, v, z, y, x, d=2, h=6, w=6):
        vol[z: z + d, y: y + h, x: x + w] = v

    box(gt, 1, 0, 2, 2), box(pred, 1, 0, 2, 3)               # organ 1: found (IoU 5/7)
    box(gt, 1, 0, 2, 20), box(pred, 1, 0, 2, 20)             #          found exactly
    box(gt, 1, 3, 20, 4)                                     #          missed: 72 voxels
    box(pred, 1, 3, 30, 30, 1, 3, 3)                         #          spurious: 9 voxels
    box(gt, 2, 0, 20, 20), box(gt, 2, 0, 20, 30)             # organ 2: two true lesions ...
    box(pred, 2, 0, 20, 20, 2, 6, 16)                        #          ... merged by one prediction: IoU 72/192 with each
    box(gt, 2, 4, 2, 2, 1, 1, 1)                             #          a 1-voxel true lesion, dropped by min_voxels
    box(pred, 3, 4, 30, 4)                                   # organ 3: only predicted
    s = lesion_scores(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), [1, 2, 3, 4], min_voxels=2)
    assert (s["tp"], s["fp"], s["fn"]) == ([2, 0, 0, 0], [1, 1, 1, 0], [1, 2, 0, 0])
    assert s["missed"] == [[72], [72, 72], [], []] and s["spurious"] == [[9], [192], [72], []]
    assert abs(s["f1"][0] - 2 / 3) < 1e-12 and s["f1"][1] == 0.0 and np.isnan(s["f1"][2]) and np.isnan(s["f1"][3])
    assert abs(s["pq"][0] - (2 / 3) * ((60 / 84 + 1.0) / (2 + 1e-6))) < 1e-12
    assert s["true_lesions"] == [3, 2, 0, 0] and s["pred_lesions"] == [3, 1, 1, 0]
    mm = lesion_scores(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), [2], spacing=(2.0, 0.5, 0.5))
    assert mm["fn"] == [3] and mm["missed"] == [[36.0, 36.0, 0.5]]
