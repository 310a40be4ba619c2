"""interactive.refine_volume on the MI355X: hiera_t at 256^2 with seeded random weights (the setting of test_video_predictor_state_machine),
6 synthetic slices, 2 objects, a synthetic blob label volume as ground truth, first clicks on slice 1 (so every round also propagates in
reverse).  With random weights the masks are arbitrary: this pins the driver's bookkeeping, not the segmentation quality."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
DEV = "cuda"
S, T, IDS, FIRST = 256, 6, [1, 2], 1


def _centre(t, o):
    return S * (0.3 + 0.35 * o) + 3 * t, S * 0.45 - 5 * t


@pytest.fixture(scope="module")
def world():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import medical_sam2_amd.build_sam as bs
    import medical_sam2_amd.synthetic as syn
    import medical_sam2_amd.weights as wts
    m = bs.build_sam2_video_predictor("sam2_hiera_t", device="cpu", hydra_overrides_extra=[f"++model.image_size={S}"])
    m.load_state_dict(wts.init_weights("hiera_t", 0), strict=True)
    m = m.to(DEV).eval()
    vol = torch.stack([syn.blob_image(20 + t, S)[0] for t in range(T)])
    ys, xs = np.mgrid[0:S, 0:S]
    gt = np.zeros((T, S, S), dtype=np.uint8)
    for t in range(T):
        for o in range(2):
            (cx, cy), rx, ry = _centre(t, o), S * 0.11 + t, S * 0.2 - 2 * o
            gt[t][((xs - cx) / rx) ** 2 + ((ys - cy) / ry) ** 2 <= 1.0] = IDS[o]
    return m, vol, gt


def _prompted_state(m, vol):
    st = m.val_init_state(vol)
    for o in range(2):
        m.add_new_points(st, FIRST, IDS[o], [list(_centre(FIRST, o))], [1])
    return st


def _propagate(m, st):
    for _ in m.propagate_in_video(st):
        pass
    for _ in m.propagate_in_video(st, start_frame_idx=FIRST, reverse=True):
        pass


def _stored(st):
    od = st["output_dict"]
    return [(od["cond_frame_outputs"].get(t) or od["non_cond_frame_outputs"][t])["pred_masks"] for t in range(T)]


def _n_points(st):
    return {(j, t): int(p["point_labels"].shape[1]) for j, per in st["point_inputs_per_obj"].items() for t, p in per.items()}


@pytest.fixture(scope="module")
def refined(world):
    from medical_sam2_amd.interactive import refine_volume
    m, vol, gt = world
    st = _prompted_state(m, vol)
    before = _n_points(st)
    records = refine_volume(m, st, torch.from_numpy(gt).to(DEV), IDS, rounds=2, keep_labels=True)
    return st, before, records


def test_clicks_lie_in_the_error_regions_of_the_worst_slices(world, refined):
    from scipy.ndimage import distance_transform_edt
    from medical_sam2_amd.volume_labels import volume_scores
    _, _, gt = world
    _, _, records = refined
    assert 1 <= len(records) <= 3 and records[-1]["clicks"] == []
    assert records[0]["clicks"], "random weights reproduce the ground truth?"
    for rec in records:
        labels = rec["labels"].cpu().numpy()
        assert labels.shape == gt.shape and labels.dtype == np.uint8
        counts = rec["counts"].cpu().numpy()
        assert rec["counts"].is_cuda and counts.shape == (T, 2, 3) and counts.dtype == np.int32
        for j, o in enumerate(IDS):
            p, g = labels == o, gt == o
            assert counts[:, j].tolist() == [[int((p[t] & g[t]).sum()), int(p[t].sum()), int(g[t].sum())] for t in range(T)]
        assert np.array_equal(rec["volume_dice"], volume_scores(counts[None])["volume_dice"][0], equal_nan=True)
        errors = np.array([[((labels[t] == o) != (gt[t] == o)).sum() for o in IDS] for t in range(T)])
        if rec is records[-1] and len(records) == 3:
            continue                                                                    # the last propagation of a full run is only scored
        # one click per object that has an error voxel, on the first slice with the most of them
        assert [c[0] for c in rec["clicks"]] == [o for j, o in enumerate(IDS) if errors[:, j].max() > 0]
        for o, t, x, y, label in rec["clicks"]:
            j = IDS.index(o)
            assert t == int(np.argmax(errors[:, j])) and errors[t, j] > 0
            fn, fp = (gt[t] == o) & (labels[t] != o), (labels[t] == o) & (gt[t] != o)
            assert label in (0, 1) and (fn if label else fp)[y, x]
            d_fn, d_fp = (distance_transform_edt(np.pad(r, 1))[1:-1, 1:-1] for r in (fn, fp))
            assert label == int(d_fn.max() > d_fp.max())
            assert (y, x) == np.unravel_index(int(np.argmax(d_fn if label else d_fp)), fn.shape)


def test_the_state_grew_by_exactly_the_reported_clicks(refined):
    st, before, records = refined
    want = dict(before)
    for rec in records:
        for o, t, x, y, label in rec["clicks"]:
            j = st["obj_id_to_idx"][o]
            want[(j, t)] = want.get((j, t), 0) + 1
    assert _n_points(st) == want and sum(want.values()) == sum(before.values()) + sum(len(r["clicks"]) for r in records)
    for rec in records:                                                                 # the last click of every (object, slice) is stored as sent
        for o, t, x, y, label in rec["clicks"]:
            p = st["point_inputs_per_obj"][st["obj_id_to_idx"][o]][t]
            assert [x, y, label] in [[round(float(a)), round(float(b)), int(c)] for (a, b), c in zip(p["point_coords"][0].tolist(),
                                                                                                      p["point_labels"][0].tolist())]


def test_a_state_driven_by_hand_stores_the_same_logits(world, refined):
    m, vol, _ = world
    st, _, records = refined
    by_hand = _prompted_state(m, vol)
    for rec in records:
        _propagate(m, by_hand)
        for o, t, x, y, label in rec["clicks"]:
            m.add_new_points(by_hand, t, o, [[float(x), float(y)]], [label], clear_old_points=False)
    a, b = _stored(st), _stored(by_hand)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert sorted(st["output_dict"]["cond_frame_outputs"]) == sorted(by_hand["output_dict"]["cond_frame_outputs"])


def test_its_own_label_volume_needs_no_click(world, refined):
    from medical_sam2_amd.interactive import refine_volume
    m, vol, _ = world
    _, _, records = refined
    out = refine_volume(m, _prompted_state(m, vol), records[0]["labels"], IDS, rounds=2)
    assert len(out) == 1 and out[0]["clicks"] == [] and "labels" not in out[0]
    c = out[0]["counts"].cpu().numpy().astype(np.int64)
    assert (c[..., 1] + c[..., 2] - 2 * c[..., 0] == 0).all() and np.array_equal(c[..., 1], records[0]["counts"].cpu().numpy()[..., 1])
    assert (out[0]["volume_dice"] == 1.0).all()


def test_refine_volume_checks_its_preconditions(world):
    from medical_sam2_amd.interactive import refine_volume
    m, vol, gt = world
    st = _prompted_state(m, vol)
    with pytest.raises(AssertionError, match="label values"):
        refine_volume(m, st, torch.from_numpy(gt).to(DEV), [2, 1])
    with pytest.raises(AssertionError, match="uint8"):
        refine_volume(m, st, torch.from_numpy(gt).to(DEV).float(), IDS)
