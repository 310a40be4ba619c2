"""msam2_label_stats / msam2_label_pick, ops.label_stats / ops.label_pick and prompts.py on the MI355X.

Every result is an integer, so every comparison is exact equality with the per-pair np.argwhere restatement (tests/prompts_restate.py),
nothing excluded.  The entries are called through the C ABI with the volume inside a 0xAB-padded buffer (also one byte off any alignment)
and stats, the per-row table and xy inside sentinel canvases of -7: an over-read would count padding (0xAB is an id of no fixture, but the
extents and counts of an object next to it would still be exact, so the canvases are what shows it), a stray store is seen."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import prompts_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64


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


class Abi:
    """one volume on the device, the two entries on padded buffers; everything comes back as int64 numpy"""

    def __init__(self, vol, ids, shift=0, stream=None):
        import medical_sam2_amd.ops as ops
        from medical_sam2_amd import _lib
        self.ops, self.L = ops, _lib.lib()
        self.D, self.H, self.W = vol.shape
        self.n = len(ids)
        self.stream = stream
        self.vcan, self.vol = padded(torch.from_numpy(vol), 0xAB, shift)
        self.vol.copy_(torch.from_numpy(vol))
        self.ids = torch.tensor(ids, dtype=torch.uint8, device=DEV)
        self.scan, self.stats = padded(torch.empty(self.D, self.n, 5, dtype=torch.int32), -7)
        self.rcan, self.rows = padded(torch.empty(self.D, self.n, self.H, dtype=torch.int32), -7)
        self.xcan, self.xy = padded(torch.empty(self.D, self.n, 2, dtype=torch.int32), -7)
        torch.cuda.synchronize()                             # the buffers are ready whichever stream the entries run on

    def _s(self):
        return self.ops._stream() if self.stream is None else self.stream.cuda_stream

    def run_stats(self, sync=True):
        p = self.ops._p
        rc = self.L.msam2_label_stats(p(self.vol), p(self.ids), self.D, self.H, self.W, self.n, p(self.stats), p(self.rows), self._s())
        assert rc == 0, self.L.msam2_last_error().decode()
        if sync:
            torch.cuda.synchronize()
            assert intact(self.scan, self.stats, -7) and intact(self.rcan, self.rows, -7), "stray store"
            return self.stats.cpu().numpy().astype(np.int64), self.rows.cpu().numpy().astype(np.int64)

    @staticmethod
    def table(kind, table):
        """a k or u table [D, n] of integers as the int32 device tensor the entry reads (u: the same 32 bits)"""
        t = np.ascontiguousarray(table, dtype=np.int64)
        t = t if kind == "k" else t - (t >= 2 ** 31) * 2 ** 32
        assert (np.abs(t) < 2 ** 31 + (kind == "u")).all()
        t = torch.from_numpy(t.astype(np.int32)).to(DEV)
        torch.cuda.synchronize()
        return t

    def run_pick(self, kind, table, sync=True):
        p = self.ops._p
        t = table if isinstance(table, torch.Tensor) else self.table(kind, table)
        rc = self.L.msam2_label_pick(p(self.vol), p(self.ids), p(self.stats), p(self.rows), p(t) if kind == "k" else None,
                                     p(t) if kind == "u" else None, self.D, self.H, self.W, self.n, p(self.xy), self._s())
        assert rc == 0, self.L.msam2_last_error().decode()
        if sync:
            torch.cuda.synchronize()
            assert intact(self.xcan, self.xy, -7), "stray store"
            return self.xy.cpu().numpy().astype(np.int64)


CASES = list(R.cases())


@pytest.mark.parametrize("name,vol,ids", CASES, ids=[c[0] for c in CASES])
def test_equal_to_the_restatement_through_the_abi(name, vol, ids):
    ref_stats, ref_rows = R.stats(vol, ids)
    count = ref_stats[..., 0]
    choices = R.k_choices(ref_stats, seed=len(name))
    ref_xy = {c: R.pick(vol, ids, t if kind == "k" else R.k_from_u(t, count)) for c, (kind, t) in choices.items()}
    assert (ref_xy["u_zero"] == ref_xy["first"]).all() and (ref_xy["u_max"] == ref_xy["last"]).all() and (ref_xy["beyond"] == ref_xy["last"]).all()
    for shift in (0, 1):
        a = Abi(vol, ids, shift)
        stats, rows = a.run_stats()
        assert np.array_equal(stats, ref_stats), (shift, np.argwhere(stats != ref_stats)[:4].tolist())
        assert np.array_equal(rows, ref_rows), (shift, np.argwhere(rows != ref_rows)[:4].tolist())
        assert (stats[count == 0] == [0, -1, -1, -1, -1]).all()
        for c, (kind, t) in choices.items():
            xy = a.run_pick(kind, t)
            assert np.array_equal(xy, ref_xy[c]), (shift, c, np.argwhere(xy != ref_xy[c])[:4].tolist())
            assert (xy[count == 0] == -1).all()
        assert intact(a.vcan, a.vol, 0xAB)


@pytest.mark.parametrize("name", ["blobs13_3x64x64", "blobs1_2x700x48", "lines_2x700x48", "checkerboard_2x5x37"])     # lines: a column of 699 rows
def test_first_and_last_voxel_of_every_occupied_row(name):
    vol, ids = next((v, i) for n, v, i in CASES if n == name)
    d, j = max(((d, j) for d in range(vol.shape[0]) for j in range(len(ids))), key=lambda p: len(np.unique(np.nonzero(vol[p[0]] == ids[p[1]])[0])))
    copies, k = R.row_edges(vol[d], ids[j])
    assert len(k) >= 2 and (name != "lines_2x700x48" or len(k) > 2 * 512)            # more rows than one round of the pick kernel's scan
    a = Abi(copies, [ids[j]])
    a.run_stats()
    xy = a.run_pick("k", k)
    assert np.array_equal(xy, R.pick(copies, [ids[j]], k))
    rows_hit = np.unique(xy[:, 0, 1])
    assert len(rows_hit) == len(k) // 2 and (xy[0::2, 0, 0] <= xy[1::2, 0, 0]).all()


def test_second_stream_gives_the_same_bits():
    vol, ids = R.blobs((9, 130, 100), 13, 3)
    ref_stats, ref_rows = R.stats(vol, ids)
    u = R.k_choices(ref_stats, 1)["u_random"][1]
    ref_xy = R.pick(vol, ids, R.k_from_u(u, ref_stats[..., 0]))
    side = torch.cuda.Stream()
    a, b = Abi(vol, ids), Abi(vol, ids, shift=1, stream=side)
    u = Abi.table("u", u)
    for _ in range(3):                                                                 # the two streams' workgroups share the device
        a.run_stats(sync=False)
        b.run_stats(sync=False)
        a.run_pick("u", u, sync=False)
        b.run_pick("u", u, sync=False)
    torch.cuda.synchronize()
    for x in (a, b):
        assert np.array_equal(x.stats.cpu().numpy(), ref_stats) and np.array_equal(x.rows.cpu().numpy(), ref_rows)
        assert np.array_equal(x.xy.cpu().numpy(), ref_xy)
        assert intact(x.scan, x.stats, -7) and intact(x.rcan, x.rows, -7) and intact(x.xcan, x.xy, -7)


def test_graph_capture_and_replay():
    import medical_sam2_amd.ops as ops
    vol, ids = R.blobs((3, 64, 64), 4, 9)
    other, _ = R.blobs((3, 64, 64), 4, 10)
    other[other > 0] = np.array(ids, dtype=np.uint8)[other[other > 0] % 4]             # another volume on the same ids
    labels = torch.from_numpy(vol).to(DEV)
    ids_d = ops.label_ids(ids, DEV)
    u = torch.randint(-2 ** 31, 2 ** 31, (3, 4), dtype=torch.int64).to(torch.int32).to(DEV)
    eager_stats, eager_rows = ops.label_stats(labels, ids_d)
    eager_xy = ops.label_pick(labels, ids_d, eager_stats, eager_rows, u=u)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        stats, rows = ops.label_stats(labels, ids_d)
        xy = ops.label_pick(labels, ids_d, stats, rows, u=u)
    for v in (other, vol, other, vol):                                                 # the replay reads what the buffers hold now
        labels.copy_(torch.from_numpy(v).to(DEV))
        stats.fill_(-7), rows.fill_(-7), xy.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        ref_stats, ref_rows = R.stats(v, ids)
        un = u.cpu().numpy().astype(np.int64) % 2 ** 32
        assert np.array_equal(stats.cpu().numpy(), ref_stats) and np.array_equal(rows.cpu().numpy(), ref_rows)
        assert np.array_equal(xy.cpu().numpy(), R.pick(v, ids, R.k_from_u(un, ref_stats[..., 0])))
    assert torch.equal(stats, eager_stats) and torch.equal(rows, eager_rows) and torch.equal(xy, eager_xy)


def _same_dicts(got, want):
    assert sorted(got) == sorted(want)
    for f in want:
        assert sorted(int(o) for o in got[f]) == sorted(int(o) for o in want[f]), f
        for o in want[f]:
            assert got[f][o].dtype == want[f][o].dtype and got[f][o].shape == want[f][o].shape and torch.equal(got[f][o], want[f][o]), (f, o)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """a synthetic case in the dataset's layout: 3 organs that come and go over the 5 labelled slices of 10, 96^2"""
    import medical_sam2_amd.data as data
    root = str(tmp_path_factory.mktemp("btcv"))
    data.write_synthetic_case(root, "case0", n_slices=10, size=96, n_objects=3, seed=0)
    return root


def _pack_and_labels(case, **kw):
    import medical_sam2_amd.data as data
    from medical_sam2_amd.volume_labels import labels_from_pack
    pack = data.BTCVVolumes(case, image_size=96, mode="Test", video_length=10, **kw)[0]
    obj_list = sorted({o for f in pack["label"] for o in pack["label"][f]})
    assert len(obj_list) >= 2 and len(pack["label"]) >= 3
    for f in pack["label"]:                                                            # no two object masks of the pack overlap
        cover = sum((m > 0).int() for m in pack["label"][f].values())
        assert not pack["label"][f] or int(cover.max()) <= 1, f
    return pack, obj_list, labels_from_pack(pack["label"], obj_list, DEV)


def test_prompts_pack_equals_the_dataset(case):
    from medical_sam2_amd.prompts import prompts_pack
    pack, obj_list, labels = _pack_and_labels(case, prompt="bbox")
    assert any(len(pack["bbox"][f]) < len(obj_list) for f in pack["bbox"]) and any(pack["bbox"][f] for f in pack["bbox"])
    _same_dicts(prompts_pack(labels, obj_list, "bbox"), pack["bbox"])
    _same_dicts(prompts_pack(labels, obj_list, "bbox", slices_per_call=3), pack["bbox"])
    every_third = prompts_pack(labels, obj_list, "bbox", prompt_freq=3)
    _same_dicts(every_third, {f: pack["bbox"][f] for f in pack["bbox"] if f % 3 == 0})
    for seed in (0, 11):
        pack_c, obj_c, labels_c = _pack_and_labels(case, prompt="click", seed=seed)
        assert obj_c == obj_list and torch.equal(labels_c, labels)
        pt, p_label = prompts_pack(labels, obj_list, "click", seed=seed)
        _same_dicts(pt, pack_c["pt"])
        _same_dicts(p_label, pack_c["p_label"])
    pack_v, _, _ = _pack_and_labels(case, prompt="bbox", seed=5, variation=0.2)
    jittered = prompts_pack(labels, obj_list, "bbox", seed=5, variation=0.2)
    _same_dicts(jittered, pack_v["bbox"])
    f, o = next((f, o) for f in pack["bbox"] for o in pack["bbox"][f])
    assert not torch.equal(jittered[f][o], pack["bbox"][f][o])


def test_label_prompts_draws_on_the_device(case):
    from medical_sam2_amd.prompts import label_prompts
    pack, obj_list, labels = _pack_and_labels(case, prompt="bbox")
    vol = labels.cpu().numpy()
    ids = [int(o) for o in obj_list]
    ref_stats, _ = R.stats(vol, ids)
    boxes, present = label_prompts(labels, obj_list, "bbox", slices_per_call=4)
    assert boxes.is_cuda and boxes.dtype == torch.float32 and boxes.shape == (vol.shape[0], len(ids), 4) and present.dtype == torch.bool
    assert np.array_equal(boxes.cpu().numpy(), ref_stats[..., [3, 1, 4, 2]].astype(np.float32))
    keys = torch.tensor([[o in pack["label"][f] for o in obj_list] for f in range(vol.shape[0])])
    assert torch.equal(present.cpu(), keys)
    g = torch.Generator(device=DEV).manual_seed(1)
    points, point_labels, present_c = label_prompts(labels, obj_list, "click", generator=g)
    assert points.is_cuda and points.dtype == torch.float32 and points.shape == (vol.shape[0], len(ids), 1, 2)
    assert point_labels.dtype == torch.int32 and point_labels.shape == (vol.shape[0], len(ids), 1) and torch.equal(present_c.cpu(), keys)
    xy, point_labels = points.cpu().numpy()[:, :, 0].astype(np.int64), point_labels.cpu()
    for d, j in np.ndindex(*keys.shape):
        if keys[d, j]:
            assert vol[d, xy[d, j, 1], xy[d, j, 0]] == ids[j] and point_labels[d, j, 0] == 1          # a voxel of the object
        else:
            assert xy[d, j].tolist() == [-1, -1] and point_labels[d, j, 0] == -1
    again = label_prompts(labels, obj_list, "click", generator=torch.Generator(device=DEV).manual_seed(1))[0]
    more = [label_prompts(labels, obj_list, "click", generator=g)[0] for _ in range(4)]
    assert torch.equal(again, points) and any(not torch.equal(m, points) for m in more)             # the generator's stream, and it moves
    # explicit tables: u and k give the restatement's voxels
    u = R.k_choices(ref_stats, 4)["u_random"][1]
    k = R.k_from_u(u, ref_stats[..., 0])
    by_u = label_prompts(labels, obj_list, "click", u=torch.from_numpy(u).to(torch.uint32), slices_per_call=3)[0]
    by_k = label_prompts(labels, obj_list, "click", k=torch.from_numpy(k))[0]
    assert np.array_equal(by_u.cpu().numpy()[:, :, 0], R.pick(vol, ids, k).astype(np.float32)) and torch.equal(by_u, by_k)
    # the 2-D use: a batch of binary masks, one object
    masks = (labels == ids[0]).to(torch.uint8)
    b2, p2 = label_prompts(masks, [1], "bbox")
    assert torch.equal(b2[:, 0], boxes[:, 0]) and torch.equal(p2[:, 0], present[:, 0])


def test_segment_prompts_names_an_absent_pair(case):
    from medical_sam2_amd.prompts import segment_prompts, targets_from_labels
    pack, obj_list, labels = _pack_and_labels(case, prompt="bbox")
    keys = [[o in pack["label"][f] for o in obj_list] for f in range(labels.shape[0])]
    t, j = next((t, j) for t in range(0, labels.shape[0], 2) for j in range(len(obj_list)) if not keys[t][j])
    with pytest.raises(ValueError, match=f"object {int(obj_list[j])} is absent on conditioning slice {t}"):
        segment_prompts(labels, obj_list, "bbox", prompt_freq=2)
    whole = [f for f in range(labels.shape[0]) if all(keys[f])]
    assert whole
    sub = labels[whole[0]: whole[0] + 1].repeat(3, 1, 1)
    pr = segment_prompts(sub, obj_list, "click", prompt_freq=2, k=torch.zeros(3, len(obj_list), dtype=torch.int32))
    assert sorted(pr) == [0, 2] and pr[0]["point_coords"].shape == (len(obj_list), 1, 2) and pr[0]["point_labels"].shape == (len(obj_list), 1)
    assert pr[2]["point_labels"].dtype == torch.int32 and bool((pr[2]["point_labels"] == 1).all())
    tg = targets_from_labels(sub, obj_list)
    assert sorted(tg) == [0, 1, 2] and tg[1].shape == (len(obj_list), 1, 96, 96) and tg[1].is_cuda
    assert torch.equal(tg[1][:, 0].sum(0), (sub[1] > 0).float())


def test_end_to_end_masks_equal_host_built_boxes():
    """hiera_t at 256^2, seeded weights, a 4-slice blob volume with 2 organs drawn on every slice, box prompts on slices 0 and 2: the masks
    of segment_volume from segment_prompts' device boxes are the masks from data.generate_bbox's boxes, bit for bit."""
    import medical_sam2_amd.build_sam as bs
    import medical_sam2_amd.data as data
    import medical_sam2_amd.synthetic as syn
    import medical_sam2_amd.volume as vol
    import medical_sam2_amd.weights as wts
    from medical_sam2_amd.prompts import segment_prompts
    S, T, n = 256, 4, 2
    m = bs.build_sam2("sam2_hiera_t", device="cpu", hydra_overrides_extra=[f"++model.image_size={S}"])
    m.load_state_dict(wts.init_weights("hiera_t", 0), strict=True)
    m = m.to(DEV).eval()
    volume, _ = syn.blob_volume(3, n_slices=T, size=S, n_objects=n)
    ys, xs = np.mgrid[0:S, 0:S]
    gt = np.zeros((T, S, S), dtype=np.uint8)
    for t in range(T):
        for o in range(n):
            cx, cy, rx, ry = S * (0.3 + 0.35 * o) + 3 * t, S * 0.45 - 5 * t, S * 0.11 + t, S * 0.2 - 2 * o
            gt[t][((xs - cx) / rx) ** 2 + ((ys - cy) / ry) ** 2 <= 1.0] = o + 1
    host = {t: {"boxes": torch.tensor(np.stack([data.generate_bbox((gt[t] == o + 1).astype(np.uint8)) for o in range(n)]), dtype=torch.float32).to(DEV)}
            for t in (0, 2)}
    device = segment_prompts(torch.from_numpy(gt).to(DEV), [1, 2], "bbox", prompt_freq=2)
    assert sorted(device) == [0, 2] and all(torch.equal(device[t]["boxes"], host[t]["boxes"]) for t in (0, 2))
    want = vol.segment_volume(m, volume.to(DEV), host, fill_hole_area=8)
    got = vol.segment_volume(m, volume.to(DEV), device, fill_hole_area=8)
    assert sorted(got) == list(range(T)) and all(torch.equal(got[t], want[t]) for t in range(T))
    assert any(bool((want[t] > 0).any()) for t in range(T))
