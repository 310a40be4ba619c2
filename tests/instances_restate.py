"""Brute-force restatement of csrc/instances.hip's tables and of medical_sam2_amd.instances' scores, for the CPU and GPU tests.

Tables: np.unique on combined keys for the pairs, np.bincount for the areas, np.unique for the remap, the three-line loop for the paint.
Scores: dense [true, pred] matrices and the formulas as the reference's docstrings state them (sam2_train/modeling/stats_utils.py), written
out again here; tests/test_instances_cpu.py holds both this and the product's sparse form against what the reference itself returned
(tests/golden/instances_cases.npz).

`defect` turns one rule into a plausible mistake (DEFECTS names them); the CPU test shows that each moves at least one golden score or
list, i.e. that the cases can see it."""
import numpy as np
from scipy.optimize import linear_sum_assignment

DEFECTS = ("ge", "last_max", "no_eps", "drop_pair", "swap_areas", "cross_class", "unstable_size")


# ---- tables ---------------------------------------------------------------------------------------------------------------------------
def remap(m, id_bound=None, labels=None, by_size=False, defect=None):
    """-> (out int64, orig, size, cls, outside): ids in 1 .. id_bound - 1 renamed 1 .. n in ascending order; anything else becomes 0 and is
    counted.  by_size: larger first, ties in the order of the original ids."""
    m = np.asarray(m).astype(np.int64)
    bound = m.size + 1 if id_bound is None else int(id_bound)
    bad = (m < 0) | (m >= bound)
    m = np.where(bad, 0, m)
    orig = np.unique(m)
    orig = orig[orig > 0]
    size = np.array([(m == i).sum() for i in orig], dtype=np.int64)
    cls = np.array([labels[m == i].max() if labels is not None else 0 for i in orig], dtype=np.int64)
    if by_size:
        order = np.argsort(-size, kind="stable")
        if defect == "unstable_size":
            order = np.lexsort((-np.arange(len(size)), -size))      # ties in the reverse order
        orig, size, cls = orig[order], size[order], cls[order]
    out = np.zeros_like(m)
    for k, i in enumerate(orig):
        out[m == i] = k + 1
    return out, orig, size, cls, int(bad.sum())


def pairs(a, b, na, nb):
    """-> (rows int64 [P, 3] sorted by (i, j), area_a [na], area_b [nb], outside_a, outside_b)"""
    a, b = np.asarray(a).astype(np.int64).ravel(), np.asarray(b).astype(np.int64).ravel()
    bad_a, bad_b = (a < 0) | (a > na), (b < 0) | (b > nb)
    a, b = np.where(bad_a, 0, a), np.where(bad_b, 0, b)
    area_a, area_b = np.bincount(a, minlength=na + 1)[1:], np.bincount(b, minlength=nb + 1)[1:]
    both = (a > 0) & (b > 0)
    key, count = np.unique(a[both] * (nb + 1) + b[both], return_counts=True)
    rows = np.stack([key // (nb + 1), key % (nb + 1), count], 1).reshape(-1, 3)
    return rows, area_a, area_b, int(bad_a.sum()), int(bad_b.sum())


def paint(masks, order=None, boxes=None, skip_covered=True):
    masks = np.asarray(masks) != 0
    n, H, W = masks.shape
    out = np.zeros((H, W), dtype=np.int64)
    for k, m in enumerate(range(n) if order is None else order):
        if not 0 <= m < n:
            continue
        mask = masks[m]
        if boxes is not None:
            x0, y0, x1, y1 = (int(v) for v in boxes[m])
            inside = np.zeros_like(mask)
            inside[max(y0, 0): y1 + 1, max(x0, 0): x1 + 1] = True
            mask = mask & inside
        if skip_covered and out[mask].all():                     # nothing of it is still 0 (an empty mask: all of nothing)
            continue
        out[mask] = k + 1
    return out


def tables(true, pred):
    """remap of both maps and their pair tables -> (rows, area_t, area_p)"""
    t, p = remap(true), remap(pred)
    rows, at, ap, _, _ = pairs(t[0], p[0], len(t[1]), len(p[1]))
    return rows, at, ap


def host_alternative(true, pred):
    """what a host would do instead of csrc/instances.hip, without the per-instance loops of remap(): np.unique with the inverse for both
    remaps, np.unique on the combined keys and np.bincount -> (rows, area_t, area_p).  tools/instances_bench.py times it."""
    ids_t, inv_t = np.unique(true, return_inverse=True)
    ids_p, inv_p = np.unique(pred, return_inverse=True)
    assert ids_t[0] == 0 and ids_p[0] == 0, "maps with a background and no negative id"
    rows, at, ap, _, _ = pairs(inv_t.reshape(-1), inv_p.reshape(-1), len(ids_t) - 1, len(ids_p) - 1)
    return rows, at, ap


# ---- scores ---------------------------------------------------------------------------------------------------------------------------
def _assignment(score):
    r, c = linear_sum_assignment(-score)
    return r, c


def scores(rows, area_t, area_p, match_iou=0.5, cls_t=None, cls_p=None, defect=None):
    """dense restatement -> dict with dq, sq, pq, tp, fp, fn, the four id lists, aji, aji_plus, dice2, dice1"""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    at, ap = np.asarray(area_t, dtype=np.float64), np.asarray(area_p, dtype=np.float64)
    nt, npred = len(at), len(ap)
    nan = float("nan")
    if nt == 0 or npred == 0:
        return dict(dq=nan, sq=nan, pq=nan, aji=nan, aji_plus=nan, dice2=nan, dice1=nan, tp=0, fp=npred, fn=nt, paired_true=[], paired_pred=[],
                    unpaired_true=list(range(1, nt + 1)), unpaired_pred=list(range(1, npred + 1)))
    if defect == "drop_pair":
        rows = rows[:-1]
    if defect == "swap_areas":
        at, ap = np.resize(ap, nt), np.resize(at, npred)
    inter = np.zeros((nt, npred))
    for i, j, c in rows:
        if cls_t is None or defect == "cross_class" or cls_t[i - 1] == cls_p[j - 1]:
            inter[i - 1, j - 1] = c
    hit = inter > 0
    union = np.where(hit, at[:, None] + ap[None, :] - inter, 0.0)
    if defect == "swap_areas":
        union = np.maximum(union, inter)                         # (wrong areas may be smaller than the intersection: keep the ratios finite)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = np.where(hit, inter / union, 0.0)
    eps = 0.0 if defect == "no_eps" else 1.0e-6
    with np.errstate(divide="ignore", invalid="ignore"):
        iou_e = np.where(hit, inter / (union + eps), 0.0)
    above = (lambda x: x >= match_iou) if defect == "ge" else (lambda x: x > match_iou)
    if match_iou >= 0.5:
        pt, pp = np.nonzero(above(iou) & hit)
    else:
        r, c = _assignment(iou)
        keep = above(iou[r, c]) & hit[r, c]
        pt, pp = r[keep], c[keep]
    matched = iou[pt, pp]
    un_t = [i + 1 for i in range(nt) if i not in set(pt.tolist())]
    un_p = [j + 1 for j in range(npred) if j not in set(pp.tolist())]
    tp, fp, fn = len(pt), len(un_p), len(un_t)
    dq = tp / (tp + 0.5 * fp + 0.5 * fn)
    sq = matched.sum() / (tp + 1.0e-6)
    # AJI: every true instance with an overlap takes the pred of largest IoU, the first of equals
    best = np.argmax(iou_e, axis=1) if defect != "last_max" else npred - 1 - np.argmax(iou_e[:, ::-1], axis=1)
    has = iou_e.max(axis=1) > 0
    at_i, ap_j = np.nonzero(has)[0], best[has]
    i_sum, u_sum = inter[at_i, ap_j].sum(), union[at_i, ap_j].sum()
    u_sum += at[~has].sum() + ap[[j for j in range(npred) if j not in set(ap_j.tolist())]].sum()
    aji = i_sum / u_sum if u_sum > 0 else nan
    r, c = _assignment(iou_e)
    keep = iou_e[r, c] > 0
    r, c = r[keep], c[keep]
    u_plus = union[r, c].sum() + at[[i for i in range(nt) if i not in set(r.tolist())]].sum() + ap[[j for j in range(npred) if j not in set(c.tolist())]].sum()
    aji_plus = inter[r, c].sum() / u_plus if u_plus > 0 else nan
    total = (at[:, None] + ap[None, :])[hit].sum()
    dice2 = 2.0 * inter.sum() / total if total > 0 else nan
    dice1 = 2.0 * inter.sum() / (at.sum() + ap.sum()) if at.sum() + ap.sum() > 0 else nan
    return dict(dq=dq, sq=sq, pq=dq * sq, aji=aji, aji_plus=aji_plus, dice2=dice2, dice1=dice1, tp=tp, fp=fp, fn=fn,
                paired_true=(pt + 1).tolist(), paired_pred=(pp + 1).tolist(), unpaired_true=un_t, unpaired_pred=un_p)


# ---- comparison with the goldens ----------------------------------------------------------------------------------------------------------
def golden_mismatches(got, G, name, tag):
    """where the score dictionary `got` (at the threshold of tag: "pq05" / "pq03") differs from what the reference returned for case `name`:
    counts and id lists exactly, float scores to relative 1e-12 (sums of at most 4096 terms in [0, 1] differ by at most 4096 * 2^-53 =
    4.5e-13 across summation orders), NaN only against NaN."""
    bad = []

    def close(key, a, b):
        a, b = float(a), float(b)
        if np.isnan(a) or np.isnan(b):
            ok = np.isnan(a) and np.isnan(b)
        else:
            ok = abs(a - b) <= 1e-12 * max(abs(a), abs(b))
        if not ok:
            bad.append((key, a, b))

    for k, key in enumerate(("dq", "sq", "pq")):
        close(key, got[key], G[f"{name}_{tag}"][k])
    for k, key in enumerate(("aji", "aji_plus", "dice2", "dice1")):
        close(key, got[key], G[f"{name}_rest"][k])
    for key in ("paired_true", "paired_pred", "unpaired_true", "unpaired_pred"):
        want = [int(v) for v in G[f"{name}_{tag}_{key}"]]
        if [int(v) for v in got[key]] != want:
            bad.append((key, got[key], want))
    want = (len(G[f"{name}_{tag}_paired_true"]), len(G[f"{name}_{tag}_unpaired_pred"]), len(G[f"{name}_{tag}_unpaired_true"]))
    if (got["tp"], got["fp"], got["fn"]) != want:
        bad.append(("tp fp fn", (got["tp"], got["fp"], got["fn"]), want))
    return bad
