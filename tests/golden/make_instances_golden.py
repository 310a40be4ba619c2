#!/usr/bin/env python3
"""Records tests/golden/instances_cases.npz: small instance maps and what the reference's own functions return for them.

    python tests/golden/make_instances_golden.py <reference checkout>

Imports sam2_train/modeling/stats_utils.py from the reference checkout (1275468127/Medical-SAM2 @ 2024_10_08).  That module imports cv2 and
matplotlib.pyplot at its top and uses neither in these functions: an empty module is registered as cv2 first, MPLBACKEND=Agg keeps
matplotlib off any display.  Per case the file holds the two input maps and the outputs of remap_label (both orders), get_fast_pq at 0.5 and
0.3 (scores and the four lists), get_fast_aji, get_fast_aji_plus, get_fast_dice_2 and get_dice_1 on the remapped maps, the way
func_2d/function.py:636-642 calls them; where that caller reports NaN without calling them (function.py:627-634: a map with one unique
value) the scores are recorded as NaN.  get_fast_dice_2 divides 0 by 0 when no pair intersects: recorded as NaN.

Case "cls" adds per-class results for case "a": every instance has a class, the reference is run per class on the maps restricted to that
class, and once on the two maps with every class moved to a plane of its own (so pairs across classes do not intersect)."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def load_reference(root):
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    spec = importlib.util.spec_from_file_location("ref_stats_utils", os.path.join(root, "sam2_train", "modeling", "stats_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def discs(shape, centres, radii, ids):
    """int32 map: disc (ball in 3-D) k around centres[k] carries ids[k]; later discs overwrite earlier ones"""
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).astype(np.float64)
    m = np.zeros(shape, dtype=np.int32)
    for c, r, i in zip(centres, radii, ids):
        m[((grid - np.asarray(c, dtype=np.float64)) ** 2).sum(-1) <= r * r] = i
    return m


def shifted_prediction(true, merged_id):
    """the truth rolled by 2 columns, every id divisible by 5 removed, the left 20 columns merged into one id"""
    pred = np.roll(true, 2, axis=-1)
    pred[pred % 5 == 0] = 0
    left = pred[..., :20]
    left[left > 0] = merged_id
    return pred


def cases():
    out = {}
    # (a) 2-D, 5 x 5 discs of radius 6 .. 9 with ids 3k + 2; equal radii give equal sizes: the by_size order has ties to keep
    cen = [(10 + 19 * r, 11 + 25 * c) for r in range(5) for c in range(5)]
    rad = [6 + (k * 7) % 4 for k in range(25)]
    rad[24], cen[24] = 9, (80, 104)                          # the last disc swallows part of its neighbour
    true = discs((96, 128), cen, rad, [3 * k + 2 for k in range(25)])
    out["a"] = (true, shifted_prediction(true, 200))
    # (b) 3-D [4, 40, 48], built the same way
    cen = [(1 + (k % 3), 7 + 13 * (k // 4), 6 + 12 * (k % 4)) for k in range(12)]
    true = discs((4, 40, 48), cen, [4 + k % 3 for k in range(12)], [3 * k + 2 for k in range(12)])
    out["b"] = (true, shifted_prediction(true, 90))
    # (c) nothing intersects
    true = discs((32, 64), [(8, 8), (22, 20)], [5, 6], [4, 9])
    pred = discs((32, 64), [(8, 40), (22, 52), (10, 56)], [5, 4, 3], [7, 2, 11])
    out["c"] = (true, pred)
    # (d) threshold and tie: true 1 = 2 px with pred 1 = 1 px inside (IoU exactly 0.5); true 2 split between two 1-px preds
    out["d"] = (np.array([[1, 1, 0, 2, 2, 0, 0, 0]], dtype=np.int32), np.array([[1, 0, 0, 2, 3, 0, 0, 0]], dtype=np.int32))
    # (e) match_iou = 0.3: the assignment takes (1, 1) + (2, 2) with IoU 0.4 + 0.33 over the single best pair (1, 2) with 0.43
    true = np.zeros((1, 32), dtype=np.int32)
    pred = np.zeros((1, 32), dtype=np.int32)
    true[0, 0:10], true[0, 10:16] = 1, 2
    pred[0, 0:4], pred[0, 4:14] = 1, 2
    out["e"] = (true, pred)
    # (f) one side without instances
    out["f"] = (out["c"][0].copy(), np.zeros((32, 64), dtype=np.int32))
    # (g) an AJI tie that shows: true 2 is split evenly between preds 2 and 3 (as in (d), where either choice gives the same sums), and
    # pred 2 is also the best of true 3 -- the first maximum leaves pred 3 unpaired, the last one would not
    out["g"] = (np.array([[1, 1, 3, 2, 2, 0, 0, 0]], dtype=np.int32), np.array([[1, 0, 2, 2, 3, 3, 0, 0]], dtype=np.int32))
    # (h) the 1e-6 in AJI's IoU decides: true 1 (4 px) meets pred 1 with 1 / 4 and pred 2 with 2 / 8 -- equal without the epsilon (the first
    # would win), with it 2 / (8 + 1e-6) is the larger
    true = np.zeros((1, 16), dtype=np.int32)
    pred = np.zeros((1, 16), dtype=np.int32)
    true[0, 0:4] = 1
    pred[0, 0], pred[0, 2:8] = 1, 2
    out["h"] = (true, pred)
    return out


def record(ref, name, true, pred, store):
    store[f"{name}_true"], store[f"{name}_pred"] = true, pred
    for side, m in (("true", true), ("pred", pred)):
        store[f"{name}_remap_{side}"] = np.asarray(ref.remap_label(m.copy(), by_size=False), dtype=np.int32)
        store[f"{name}_bysize_{side}"] = np.asarray(ref.remap_label(m.copy(), by_size=True), dtype=np.int32)
    gt, pr = store[f"{name}_remap_true"], store[f"{name}_remap_pred"]
    empty = len(np.unique(gt)) == 1 or len(np.unique(pr)) == 1          # function.py:627: the caller reports NaN
    for thr, tag in ((0.5, "pq05"), (0.3, "pq03")):
        if empty:
            scores, lists = [np.nan] * 3, [[], [], [int(i) for i in np.unique(gt)[1:]], [int(i) for i in np.unique(pr)[1:]]]
        else:
            scores, lists = ref.get_fast_pq(gt, pr, match_iou=thr)
        store[f"{name}_{tag}"] = np.asarray(scores, dtype=np.float64)
        for which, ids in zip(("paired_true", "paired_pred", "unpaired_true", "unpaired_pred"), lists):
            store[f"{name}_{tag}_{which}"] = np.asarray(list(ids), dtype=np.int64)
    if empty:
        rest = [np.nan] * 4
    else:
        try:
            dice2 = float(ref.get_fast_dice_2(gt, pr))
        except ZeroDivisionError:
            dice2 = np.nan
        rest = [float(ref.get_fast_aji(gt, pr)), float(ref.get_fast_aji_plus(gt, pr)), dice2, float(ref.get_dice_1(gt, pr))]
    store[f"{name}_rest"] = np.asarray(rest, dtype=np.float64)          # aji, aji_plus, dice2, dice1


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = load_reference(sys.argv[1])
    store = {}
    all_cases = cases()
    for name, (true, pred) in all_cases.items():
        record(ref, name, true, pred, store)
    # classes for case (a): an instance's class is 1 + (original id % 2)
    true, pred = all_cases["a"]
    cls_true, cls_pred = np.where(true > 0, 1 + true % 2, 0).astype(np.uint8), np.where(pred > 0, 1 + pred % 2, 0).astype(np.uint8)
    store["cls_labels_true"], store["cls_labels_pred"] = cls_true, cls_pred
    for c in (1, 2):
        record(ref, f"cls{c}", np.where(cls_true == c, true, 0).astype(np.int32), np.where(cls_pred == c, pred, 0).astype(np.int32), store)
    record(ref, "clsall", np.stack([np.where(cls_true == c, true, 0) for c in (1, 2)]).astype(np.int32),
           np.stack([np.where(cls_pred == c, pred, 0) for c in (1, 2)]).astype(np.int32), store)
    path = os.path.join(HERE, "instances_cases.npz")
    np.savez_compressed(path, **store)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(store)} arrays")
    for n in ("a", "b", "c", "d", "e", "f", "g", "h", "cls1", "cls2", "clsall"):
        print(n, "true", int(store[f"{n}_remap_true"].max()), "pred", int(store[f"{n}_remap_pred"].max()), "pq05", store[f"{n}_pq05"], "pq03",
              store[f"{n}_pq03"], "aji aji+ dice2 dice1", store[f"{n}_rest"])


if __name__ == "__main__":
    main()
