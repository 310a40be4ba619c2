"""Host half of the instance scores (medical_sam2_amd/instances.py: instance_scores_from_tables) and the restatement the GPU tests compare
csrc/instances.hip with (tests/instances_restate.py), both against what the reference's own stats_utils functions returned for the cases of
tests/golden/instances_cases.npz (tests/golden/make_instances_golden.py).  No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import instances_restate as R  # noqa: E402

CASES = ("a", "b", "c", "d", "e", "f", "g", "h")
THRESHOLDS = ((0.5, "pq05"), (0.3, "pq03"))


@pytest.fixture(scope="module")
def G():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "instances_cases.npz")))


@pytest.fixture(scope="module")
def scorer():
    from medical_sam2_amd.instances import instance_scores_from_tables
    return instance_scores_from_tables


def test_the_cases_are_what_the_issue_asks_for(G):
    t, p = R.tables(G["a_true"], G["a_pred"])[1:]
    assert G["a_true"].shape == (96, 128) and len(t) >= 20 and len(p) >= 15 and len(R.tables(G["a_true"], G["a_pred"])[0]) > len(p)
    assert sorted(np.unique(G["a_true"]))[1] == 2 and np.all((np.unique(G["a_true"])[1:] - 2) % 3 == 0)       # ids 3k + 2: not contiguous
    assert G["b_true"].shape == (4, 40, 48) and 0.0 < G["a_pq05"][2] < 1.0 and 0.0 < G["a_rest"][0] < 1.0 and 0.0 < G["b_pq05"][2] < 1.0
    assert len(R.tables(G["c_true"], G["c_pred"])[0]) == 0 and G["c_rest"][0] == 0.0 and G["c_pq05"][0] == 0.0 and G["c_pq05"][1] == 0.0
    assert G["d_true"].shape == (1, 8) and G["d_pq05"][0] == 0.0 and abs(G["d_rest"][0] - 0.4) < 1e-12 and abs(G["d_rest"][1] - 0.4) < 1e-12
    assert len(G["e_pq03_paired_true"]) == 2 and len(G["e_pq05_paired_true"]) == 0
    assert all(np.isnan(G[f"f_{k}"]).all() for k in ("pq05", "pq03", "rest"))


@pytest.mark.parametrize("name", CASES + ("cls1", "cls2", "clsall"))
def test_remap_restatement_is_the_reference_remap_label(G, name):
    for side in ("true", "pred"):
        m = G[f"{name}_{side}"]
        assert np.array_equal(R.remap(m)[0], G[f"{name}_remap_{side}"])
        out, orig, size, _, _ = R.remap(m, by_size=True)
        assert np.array_equal(out, G[f"{name}_bysize_{side}"])
        assert np.all(np.diff(size) <= 0) and all(np.all(np.diff(orig[size == s]) > 0) for s in set(size.tolist()))    # ties keep id order


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("thr,tag", THRESHOLDS)
def test_scores_from_restated_tables_equal_the_reference(G, scorer, name, thr, tag):
    rows, at, ap = R.tables(G[f"{name}_true"], G[f"{name}_pred"])
    assert R.golden_mismatches(R.scores(rows, at, ap, thr), G, name, tag) == []
    assert R.golden_mismatches(scorer(rows, at, ap, thr), G, name, tag) == []
    assert R.golden_mismatches(scorer(rows[::-1].astype(np.int32), at.astype(np.int32), ap, thr), G, name, tag) == []      # any row order, any int type


def _class_tables(G):
    t = R.remap(G["a_true"], labels=G["cls_labels_true"])
    p = R.remap(G["a_pred"], labels=G["cls_labels_pred"])
    rows, at, ap, _, _ = R.pairs(t[0], p[0], len(t[1]), len(p[1]))
    return rows, at, ap, t[3], p[3]


@pytest.mark.parametrize("thr,tag", THRESHOLDS)
def test_scores_per_class_equal_the_reference_on_the_maps_of_that_class(G, scorer, thr, tag):
    rows, at, ap, ct, cp = _class_tables(G)
    assert (ct[rows[:, 0] - 1] != cp[rows[:, 1] - 1]).any(), "the case has pairs across classes"
    got = scorer(rows, at, ap, thr, ct, cp)
    assert R.golden_mismatches(got, G, "clsall", tag) == []                     # every class on a plane of its own: cross pairs are gone
    assert R.golden_mismatches(R.scores(rows, at, ap, thr, ct, cp), G, "clsall", tag) == []
    assert sorted(got["per_class"]) == [1, 2]
    for c in (1, 2):
        # the reference numbered the instances of the class 1 .. n in ascending id: the same order, so the lists map through the class's ids
        ids_t, ids_p = np.flatnonzero(ct == c) + 1, np.flatnonzero(cp == c) + 1
        sub = dict(got["per_class"][c])
        for key, ids in (("paired_true", ids_t), ("unpaired_true", ids_t), ("paired_pred", ids_p), ("unpaired_pred", ids_p)):
            sub[key] = [int(np.searchsorted(ids, v)) + 1 for v in sub[key]]
        assert R.golden_mismatches(sub, G, f"cls{c}", tag) == []
    with pytest.raises(ValueError):
        scorer(rows, at, ap, thr, ct, None)


def _moved(G, defect):
    """the (case, threshold) pairs at which the defect changes a golden score or list"""
    hits = []
    if defect == "unstable_size":
        for name in CASES:
            for side in ("true", "pred"):
                if not np.array_equal(R.remap(G[f"{name}_{side}"], by_size=True, defect=defect)[0], G[f"{name}_bysize_{side}"]):
                    hits.append((name, side))
        return hits
    for thr, tag in THRESHOLDS:
        if defect == "cross_class":
            rows, at, ap, ct, cp = _class_tables(G)
            if R.golden_mismatches(R.scores(rows, at, ap, thr, ct, cp, defect=defect), G, "clsall", tag):
                hits.append(("clsall", tag))
            continue
        for name in CASES:
            rows, at, ap = R.tables(G[f"{name}_true"], G[f"{name}_pred"])
            if R.golden_mismatches(R.scores(rows, at, ap, thr, defect=defect), G, name, tag):
                hits.append((name, tag))
    return hits


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_defect_moves_a_golden(G, defect):
    hits = _moved(G, defect)
    assert hits, f"no case sees the defect {defect}"
    if defect == "ge":
        assert ("d", "pq05") in hits                    # IoU exactly 0.5 must not match
    if defect == "last_max":
        assert any(h[0] == "g" for h in hits)           # (d)'s tie gives the same sums either way; (g)'s leaves another pred unpaired
    if defect == "no_eps":
        assert any(h[0] == "h" for h in hits)           # 1 / 4 against 2 / 8


def test_the_restatement_of_pairs_and_paint_on_hand_made_maps():
    a = np.array([[1, 1, 2, 0], [1, 3, 2, 9]])
    b = np.array([[1, 2, 2, -4], [0, 1, 2, 1]])
    rows, aa, ab, oa, ob = R.pairs(a, b, 3, 2)
    assert rows.tolist() == [[1, 1, 1], [1, 2, 1], [2, 2, 2], [3, 1, 1]] and aa.tolist() == [3, 2, 1] and ab.tolist() == [3, 3] and (oa, ob) == (1, 1)
    masks = np.zeros((4, 2, 4), dtype=np.uint8)
    masks[0, 0, :3] = 1                 # painted as 1
    masks[1, 0, 1:3] = 1                # covered by 1: skipped
    masks[3, :, 2:] = 7                 # mask 2 is empty: skipped; mask 3 sees zeros: overwrites part of 1
    assert R.paint(masks).tolist() == [[1, 1, 4, 4], [0, 0, 4, 4]]
    assert R.paint(masks, skip_covered=False).tolist() == [[1, 2, 4, 4], [0, 0, 4, 4]]
    assert R.paint(masks, order=[3, 0, 9, 1]).tolist() == [[2, 2, 2, 1], [0, 0, 1, 1]]
    assert R.paint(masks, boxes=[[0, 0, 1, 0], [0, 0, 3, 1], [0, 0, 3, 1], [3, 0, 3, 1]]).tolist() == [[1, 2, 2, 4], [0, 0, 0, 4]]


def test_empty_sides_and_the_dense_cap(scorer):
    import medical_sam2_amd.instances as I
    s = scorer(np.zeros((0, 3)), [5, 6], [])
    assert all(np.isnan(s[k]) for k in I.SCORE_KEYS) and (s["tp"], s["fp"], s["fn"]) == (0, 0, 2) and s["unpaired_true"] == [1, 2]
    with pytest.raises(ValueError, match="DENSE_CAP"):
        scorer(np.zeros((0, 3)), np.ones(5000), np.ones(5000))
    with pytest.raises(ValueError):
        scorer([[3, 1, 1]], [4, 4], [4])
