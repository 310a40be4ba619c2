"""msam2_label_slices / ops.label_slices / volume_labels.py on the MI355X.

The entry is called through the C ABI with the logits inside a NaN-padded buffer and labels / counts inside sentinel canvases (bytes 0xAB,
ints -7): an over-read poisons a result, a stray store is seen.

1. bit equality with the composition the kernel replaces: ops.bilinear_upsample's output moved to numpy, the label / count rule applied there
   (tests/volume_labels_restate.py: apply_rule) -- labels and every count equal, integer for integer;
2. exact against the float64 restatement on dyadic fixtures (ties, values at exactly label_thr), nothing excluded;
3. random fields against the float64 restatement: labels equal on every voxel whose decision margin is >= 1e-3, each count within the
   number of undecided voxels of its slice, at most 5 % of a slice undecided (checked on the CPU for the same fixtures);
4. the limits cross the ABI as codes; 5. the Python layer; 6. the end of the real path behind volume.segment_volume."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import volume_labels_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64                       # elements of padding either side of every buffer (a multiple of 4: the canvases keep the 4-voxel path)


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
    start = view.data_ptr() - canvas.data_ptr()
    rest[start // canvas.element_size(): start // canvas.element_size() + view.numel()] = False
    return bool((canvas[rest] == fill).all())


def call_abi(logits, ids, H, W, label_thr=0.0, thresholds=None, gt=None, exclusive=False, want_labels=True, want_counts=True, shift=0):
    """msam2_label_slices on padded buffers -> (labels uint8 numpy | None, counts int64 numpy | None)"""
    import medical_sam2_amd.ops as ops
    from medical_sam2_amd import _lib
    T, n, lh, lw = logits.shape
    lcan, lview = padded(logits.float(), float("nan"))
    lview.copy_(logits)
    ids_d = torch.tensor(ids, dtype=torch.uint8, device=DEV)
    thr_d = None if thresholds is None else torch.tensor(R.f32_thresholds(thresholds), dtype=torch.float32, device=DEV)
    K = 0 if thr_d is None else thr_d.numel()
    lab_can = lab = cnt_can = cnt = gt_d = None
    if want_labels:
        lab_can, lab = padded(torch.empty(T, H, W, dtype=torch.uint8), 0xAB, shift)
    if want_counts:
        cnt_can, cnt = padded(torch.empty(K, T, n, 3, dtype=torch.int32), -7)
    if gt is not None:
        _, gt_d = padded(torch.as_tensor(gt), 0xAB, shift)
        gt_d.copy_(torch.as_tensor(gt))
    rc = _lib.lib().msam2_label_slices(ops._p(lview), ops._p(ids_d), T, n, lh, lw, H, W, float(np.float32(label_thr)), ops._p(thr_d), K, ops._p(gt_d),
                                       int(exclusive), ops._p(lab), ops._p(cnt), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().msam2_last_error().decode()
    if want_labels:
        assert intact(lab_can, lab, 0xAB), "stray label store"
    if want_counts:
        assert intact(cnt_can, cnt, -7), "stray count store"
    return (lab.cpu().numpy() if want_labels else None), (cnt.cpu().numpy().astype(np.int64) if want_counts else None)


_COMPOSITION = {}


def composition(shape, seed):
    """(logits on the device, ops.bilinear_upsample's output as numpy [T, n, H, W], ids, gt): computed once per case"""
    import medical_sam2_amd.ops as ops
    key = (tuple(shape[:2]) + shape[2] + shape[3], seed)
    if key not in _COMPOSITION:
        T, n, (lh, lw), (H, W) = shape
        x = R.random_logits(T, n, lh, lw, seed).to(DEV)
        up = ops.bilinear_upsample(x.view(T * n, lh, lw), H, W).view(T, n, H, W).cpu().numpy()
        ids = R.random_ids(n, seed)
        _COMPOSITION[key] = (x, up, ids, R.random_gt(T, H, W, ids, seed).numpy())
    return _COMPOSITION[key]


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d_%dx%d_to_%dx%d" % (s[0], s[1], *s[2], *s[3]))
@pytest.mark.parametrize("seed", R.SEEDS)
def test_bit_equal_to_upsample_then_rule(shape, seed):
    x, up, ids, gt = composition(shape, seed)
    H, W = shape[3]
    assert up.dtype == np.float32
    for thresholds in (R.REFERENCE_THRESHOLDS, R.EIGHT_THRESHOLDS):
        for exclusive in (False, True):
            ref_labels, ref_counts, _ = R.apply_rule(up, ids, 0.0, thresholds, gt, exclusive)
            labels, counts = call_abi(x, ids, H, W, 0.0, thresholds, gt, exclusive)
            assert np.array_equal(labels, ref_labels), (thresholds, exclusive, int((labels != ref_labels).sum()))
            assert np.array_equal(counts, ref_counts), (thresholds, exclusive, np.abs(counts - ref_counts).max())
    ref_labels, ref_counts, _ = R.apply_rule(up, ids, 0.0, R.REFERENCE_THRESHOLDS, None, False)
    labels, _ = call_abi(x, ids, H, W, want_counts=False)                                   # labels only
    assert np.array_equal(labels, ref_labels)
    _, counts = call_abi(x, ids, H, W, 0.0, R.REFERENCE_THRESHOLDS, want_labels=False)    # counts only, gt absent: |P| alone
    assert np.array_equal(counts, ref_counts) and counts[..., 1].sum() > 0 and counts[..., 0].sum() == 0 and counts[..., 2].sum() == 0
    # another label threshold, and label / gt volumes that are not 4-byte aligned (the one-voxel path also where W % 4 == 0)
    ref_labels, ref_counts, _ = R.apply_rule(up, ids, 1.5, R.REFERENCE_THRESHOLDS, gt, True)
    labels, counts = call_abi(x, ids, H, W, 1.5, R.REFERENCE_THRESHOLDS, gt, True, shift=1)
    assert np.array_equal(labels, ref_labels) and np.array_equal(counts, ref_counts)
    # not vacuous: background and several objects in the labels, hits in the intersections
    if shape[2] != (1, 1) and 1 < shape[1] <= 13:       # (one value per plane, or 32 objects of which one is nearly always above 1.5, do not show it)
        assert 0 in ref_labels and len(np.unique(ref_labels)) > 2 and ref_counts[..., 0].sum() > 0


@pytest.mark.parametrize("low,out", R.DYADIC_CASES)
def test_exact_against_float64_on_dyadic_fixtures(low, out):
    T, (lh, lw), (H, W) = 2, low, out
    x = R.dyadic_logits(T, lh, lw, seed=H)
    ids = R.random_ids(6, seed=H)
    gt = R.random_gt(T, H, W, ids, seed=H).numpy()
    for exclusive in (False, True):
        ref_labels, ref_counts, margin = R.restate(x.numpy(), ids, H, W, 0.0, R.DYADIC_THRESHOLDS, gt, exclusive)
        labels, counts = call_abi(x.to(DEV), ids, H, W, 0.0, R.DYADIC_THRESHOLDS, gt, exclusive)
        assert np.array_equal(labels, ref_labels) and np.array_equal(counts, ref_counts)
    assert (margin == 0).mean() > 0.2                    # ties and values at exactly a threshold are most of this fixture


@pytest.mark.parametrize("shape", R.RANDOM_FIELD_SHAPES, ids=lambda s: "%dx%d_%dx%d_to_%dx%d" % (s[0], s[1], *s[2], *s[3]))
@pytest.mark.parametrize("seed", R.SEEDS)
def test_random_fields_against_float64(shape, seed):
    x, _, ids, gt = composition(shape, seed)
    H, W = shape[3]
    for exclusive in (False, True):
        ref_labels, ref_counts, margin = R.restate(x.cpu().numpy(), ids, H, W, 0.0, R.REFERENCE_THRESHOLDS, gt, exclusive)
        labels, counts = call_abi(x, ids, H, W, 0.0, R.REFERENCE_THRESHOLDS, gt, exclusive)
        decided = margin >= R.MARGIN
        undecided = (~decided).sum(axis=(1, 2))                                            # per slice
        assert (undecided <= R.UNDECIDED_CAP * H * W).all(), undecided
        assert np.array_equal(labels[decided], ref_labels[decided])
        assert (np.abs(counts - ref_counts) <= undecided[None, :, None, None]).all(), np.abs(counts - ref_counts).max()
        assert np.array_equal(counts[..., 2], ref_counts[..., 2])                          # |G| does not depend on the logits


@pytest.mark.parametrize("out", [(32, 32), (30, 30)], ids=["4_voxel_path", "scalar_path"])
def test_graph_capture_and_replay(out):
    """Four replays over two logit sets into caller-owned labels and counts, poisoned before every replay: the pre-set of counts is a node of
    the graph, and a replay that did not run it in order would add to the poison or to the replay before."""
    import medical_sam2_amd.ops as ops
    from medical_sam2_amd import _lib
    T, n, (lh, lw), (H, W) = 2, 3, (8, 8), out
    ids = R.random_ids(n, 11)
    thresholds = R.REFERENCE_THRESHOLDS[1:3]
    gt = R.random_gt(T, H, W, ids, 11)
    sets = [R.random_logits(T, n, lh, lw, seed) for seed in (11, 12)]
    x, gt_d = sets[0].to(DEV), gt.to(DEV)
    ids_d = torch.tensor(ids, dtype=torch.uint8, device=DEV)
    thr_d = torch.tensor(R.f32_thresholds(thresholds), dtype=torch.float32, device=DEV)
    labels = torch.empty(T, H, W, dtype=torch.uint8, device=DEV)
    counts = torch.empty(len(thresholds), T, n, 3, dtype=torch.int32, device=DEV)

    def call():
        rc = _lib.lib().msam2_label_slices(ops._p(x), ops._p(ids_d), T, n, lh, lw, H, W, 0.0, ops._p(thr_d), len(thresholds), ops._p(gt_d), 0,
                                           ops._p(labels), ops._p(counts), ops._stream())
        assert rc == 0, _lib.lib().msam2_last_error().decode()
    call()                                                                                  # eager first: nothing is set up inside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for logits in (sets[1], sets[0], sets[1], sets[0]):                                    # the replay reads what the buffer holds now
        x.copy_(logits.to(DEV))
        labels.fill_(0xAB), counts.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        up = ops.bilinear_upsample(x.view(T * n, lh, lw), H, W).view(T, n, H, W).cpu().numpy()
        ref_labels, ref_counts, _ = R.apply_rule(up, ids, 0.0, thresholds, gt.numpy(), False)
        assert np.array_equal(labels.cpu().numpy(), ref_labels)
        assert np.array_equal(counts.cpu().numpy().astype(np.int64), ref_counts)
        assert ref_counts[..., 0].sum() > 0 and len(np.unique(ref_labels)) > 2             # not vacuous


def test_argument_errors_cross_the_abi_as_codes():
    import medical_sam2_amd.ops as ops
    from medical_sam2_amd import _lib
    L = _lib.lib()
    x = torch.zeros(1, 33, 4, 4, device=DEV)
    ids = torch.arange(1, 34, dtype=torch.uint8, device=DEV)
    thr = torch.zeros(9, device=DEV)
    lab = torch.zeros(1, 8, 8, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(9, 1, 33, 3, dtype=torch.int32, device=DEV)
    p = ops._p

    def call(n=2, K=5, logits=x, labels=lab, counts=cnt):
        return L.msam2_label_slices(p(logits), p(ids), 1, n, 4, 4, 8, 8, 0.0, p(thr), K, None, 0, p(labels), p(counts), ops._stream())
    assert call() == 0
    for what, kw in {"n = 33": dict(n=33), "K = 9": dict(K=9), "null logits": dict(logits=None), "neither": dict(labels=None, counts=None)}.items():
        rc = call(**kw)
        msg = L.msam2_last_error().decode()
        assert rc < 0 and "label_slices" in msg and what in msg, (what, rc, msg)
    with pytest.raises(_lib.Msam2Error, match="label_slices"):
        ops.label_slices(x, list(range(1, 34)), 8, 8)
    with pytest.raises(ValueError, match="distinct"):
        ops.label_slices(x[:, :2].contiguous(), [4, 4], 8, 8)
    torch.cuda.synchronize()


def _eval_seg_per_pair(up, ids, gt, thresholds):
    """validate_volume's scoring loop on the composition's up-sampled maps: metrics.eval_seg per (slice, object)"""
    from medical_sam2_amd.metrics import eval_seg
    T, n = up.shape[:2]
    iou = dice = 0.0
    per = np.zeros((2, T, n))
    for t in range(T):
        for o in range(n):
            r = eval_seg(up[t, o][None, None], (gt[t] == ids[o]).float()[None, None], thresholds)
            per[0, t, o], per[1, t, o] = r
            iou, dice = iou + r[0], dice + r[1]
    return iou / (T * n), dice / (T * n), per


def test_python_layer(tmp_path):
    import medical_sam2_amd.data as data
    import medical_sam2_amd.ops as ops
    from medical_sam2_amd.volume_labels import label_volume, labels_from_pack, volume_scores
    T, n, (lh, lw), (H, W) = 5, 3, (16, 16), (64, 48)
    x = R.random_logits(T, n, lh, lw, 7).to(DEV)
    ids = [9, 2, 200]
    gt = R.random_gt(T, H, W, ids, 7).to(DEV)
    up = ops.bilinear_upsample(x.view(T * n, lh, lw), H, W).view(T, n, H, W)
    ref_labels, ref_counts, _ = R.apply_rule(up.cpu().numpy(), ids, 0.0, R.REFERENCE_THRESHOLDS, gt.cpu().numpy(), False)
    as_dict = {10 * t: x[t][:, None] for t in reversed(range(T))}                          # keys in ascending order are the slices
    runs = [label_volume(x, H, W, ids, gt), label_volume(as_dict, H, W, ids, gt), label_volume(x, H, W, ids, gt, slices_per_call=1),
            label_volume(as_dict, H, W, ids, gt, slices_per_call=T), label_volume(x, H, W, ids, gt, slices_per_call=2)]
    for labels, counts in runs:
        assert labels.dtype == torch.uint8 and labels.is_cuda and counts.dtype == torch.int32 and counts.is_cuda
        assert np.array_equal(labels.cpu().numpy(), ref_labels) and np.array_equal(counts.cpu().numpy(), ref_counts)
    only = label_volume(as_dict, H, W, ids)
    assert isinstance(only, torch.Tensor) and np.array_equal(only.cpu().numpy(), ref_labels)
    assert np.array_equal(label_volume(x, H, W).cpu().numpy(), R.apply_rule(up.cpu().numpy(), [1, 2, 3], 0.0)[0])       # default ids 1 .. n
    # more than 8 thresholds go through in two launches; the exclusive counts are those of the rule on the label volume
    many = tuple(np.linspace(-2, 2, 11))
    _, counts = label_volume(x, H, W, ids, gt, thresholds=many, exclusive=True, slices_per_call=3)
    assert np.array_equal(counts.cpu().numpy(), R.apply_rule(up.cpu().numpy(), ids, 0.0, many, gt.cpu().numpy(), True)[1])
    # the scores: eval_seg called per (slice, object) on the up-sampled maps, to the last bit of the floats it returns
    s = volume_scores(runs[0][1])
    iou, dice, per = _eval_seg_per_pair(up, ids, gt, R.REFERENCE_THRESHOLDS)
    assert s["iou"] == iou and s["dice"] == dice
    assert np.array_equal(s["iou_per_pair"], per[0]) and np.array_equal(s["dice_per_pair"], per[1])
    vol = ref_counts.sum(axis=1).astype(np.float64)
    assert np.array_equal(s["volume_dice"], 2 * vol[..., 0] / (vol[..., 1] + vol[..., 2])) and s["volume_dice"].shape == (5, n)
    # ground truth of the data contract -> label volume -> the same masks
    data.write_synthetic_case(str(tmp_path), "case0", n_slices=6, size=64, n_objects=2, seed=1)
    pack = data.BTCVVolumes(str(tmp_path), image_size=64, mode="Test", video_length=6)[0]
    obj_list = sorted({o for f in pack["label"] for o in pack["label"][f]})
    vol = labels_from_pack(pack["label"], obj_list, DEV)
    assert vol.is_cuda and vol.dtype == torch.uint8 and vol.shape[1:] == (64, 64) and obj_list and set(vol.unique().tolist()) == {0, *[int(o) for o in obj_list]}
    for f in pack["label"]:
        for o in obj_list:
            m = pack["label"][f].get(o)
            want = torch.zeros(64, 64, dtype=torch.bool) if m is None else m[0] > 0
            assert torch.equal(vol[f].cpu() == int(o), want), (f, o)                       # the synthetic organs do not overlap in the label maps


def test_end_of_the_real_path():
    """hiera_t at 256^2, seeded weights, a 4-slice blob volume with 2 objects, box prompts on slices 0 and 2: segment_volume, then
    label_volume to the video resolution and to another size."""
    import medical_sam2_amd.build_sam as bs
    import medical_sam2_amd.ops as ops
    import medical_sam2_amd.synthetic as syn
    import medical_sam2_amd.volume as vol
    import medical_sam2_amd.weights as wts
    from medical_sam2_amd.volume_labels import label_volume, volume_scores
    S, T, n = 256, 4, 2
    m = bs.build_sam2("sam2_hiera_t", device="cpu", hydra_overrides_extra=[f"++model.image_size={S}"])
    m.load_state_dict(wts.init_weights("hiera_t", 0), strict=True)
    m = m.to(DEV).eval()
    volume, boxes = syn.blob_volume(3, n_slices=T, size=S, n_objects=n)
    box_at = lambda t: torch.tensor([[float(v) for v in (boxes[o][t] or (S * 0.3, S * 0.3, S * 0.6, S * 0.6))] for o in range(n)])
    masks = vol.segment_volume(m, volume.to(DEV), {t: {"boxes": box_at(t).to(DEV)} for t in (0, 2)}, fill_hole_area=8)
    assert sorted(masks) == list(range(T)) and masks[0].shape == (n, 1, S // 4, S // 4)
    # the synthetic case's ground truth, as data.write_synthetic_case draws it: the ellipse inscribed in each organ's box
    ys, xs = np.mgrid[0:S, 0:S]
    gt = np.zeros((T, S, S), dtype=np.uint8)
    for t in range(T):
        for o in range(n):
            b = boxes[o][t]
            if b is not None:
                cx, cy, rx, ry = (b[0] + b[2]) / 2, (b[1] + b[3]) / 2, max((b[2] - b[0]) / 2, 0.5), max((b[3] - b[1]) / 2, 0.5)
                gt[t][((xs - cx) / rx) ** 2 + ((ys - cy) / ry) ** 2 <= 1.0] = o + 1
    present = set(np.unique(gt).tolist()) - {0}
    assert present
    x = torch.stack([masks[t][:, 0] for t in range(T)]).float().contiguous()
    for (H, W) in ((S, S), (200, 312)):
        g = torch.from_numpy(gt).to(DEV) if (H, W) == (S, S) else torch.from_numpy(gt[:, :H, :].repeat(2, axis=2)[:, :, :W].copy()).to(DEV)
        labels, counts = label_volume(masks, H, W, gt=g)
        up = ops.bilinear_upsample(x.view(T * n, S // 4, S // 4), H, W).view(T, n, H, W).cpu().numpy()
        ref_labels, ref_counts, _ = R.apply_rule(up, [1, 2], 0.0, R.REFERENCE_THRESHOLDS, g.cpu().numpy(), False)
        assert np.array_equal(labels.cpu().numpy(), ref_labels) and np.array_equal(counts.cpu().numpy(), ref_counts)
        assert present <= set(np.unique(ref_labels).tolist()), (present, np.unique(ref_labels))
        s = volume_scores(counts)
        assert np.isfinite([s["iou"], s["dice"]]).all() and np.isfinite(s["iou_per_pair"]).all() and np.isfinite(s["dice_per_pair"]).all()
        if (H, W) == (S, S):
            assert all(np.isfinite(s["volume_dice"][:, o - 1]).all() for o in present)
