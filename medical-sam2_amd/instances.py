"""Instance scores: panoptic quality (DQ / SQ / PQ), AJI, AJI+, the two Dice variants and lesion-wise detection counts.

The reference's 2-D validation (`func_2d/function.py:620-651`, the same loop in `sam2_train/modeling/function.py:640-656`) paints an
instance map from the predicted masks, calls `remap_label` on both maps and reports `get_fast_pq`, `get_fast_aji`, `get_fast_aji_plus`,
`get_fast_dice_2` and `get_dice_1` (`sam2_train/modeling/stats_utils.py`), all on the host: one boolean mask per instance and one masked
`np.unique` per ground-truth instance, three times over.  Every one of those scores is a function of three small integer tables -- the
non-empty entries of the pairwise-intersection matrix and the instance areas of both maps -- which csrc/instances.hip takes from one pass
over the two maps on the device.  The pattern of `label_stats` / `label_overlap` / `label_measure`: integer tables on the device, one small
host copy, scores on the host in float64.

  device   remap_instances, instances_from_labels, paint_instances, instance_tables
  host     instance_scores_from_tables (pure numpy: usable without the library), on whatever made the tables
  both     instance_scores

Maps are int32 [H, W] or [D, H, W], 0 = background."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

DENSE_CAP = 1 << 24               # true x pred entries of the dense matrix the Hungarian paths build (AJI+, match_iou < 0.5)
MAX_INSTANCES = 1 << 14           # default rows of the per-instance tables
SCORE_KEYS = ("dq", "sq", "pq", "aji", "aji_plus", "dice2", "dice1")


# ---- host half ------------------------------------------------------------------------------------------------------------------------
def _hungarian(ti, pj, value, nt, npred):
    """linear_sum_assignment on the dense negated matrix, as the reference calls it -> (rows, cols, index of the pair or -1)"""
    from scipy.optimize import linear_sum_assignment
    if nt * npred > DENSE_CAP:
        raise ValueError(f"instance scores: a dense {nt} x {npred} matrix for the Hungarian pairing exceeds DENSE_CAP = {DENSE_CAP} entries")
    dense = np.zeros((nt, npred), dtype=np.float64)
    which = np.full((nt, npred), -1, dtype=np.int64)
    dense[ti, pj] = value
    which[ti, pj] = np.arange(len(ti))
    rows, cols = linear_sum_assignment(-dense)
    return rows, cols, which[rows, cols]


def _core(ti, pj, inter, at, ap, match_iou):
    """the reference's formulas on 0-based pair indices ti / pj (sorted by (ti, pj)), intersections and the two area vectors"""
    nt, npred = len(at), len(ap)
    nan = float("nan")
    if nt == 0 or npred == 0:     # the reference's caller, function.py:627-634
        out = {k: nan for k in SCORE_KEYS}
        out.update(tp=0, fp=npred, fn=nt, paired_true=[], paired_pred=[], unpaired_true=list(range(nt)), unpaired_pred=list(range(npred)))
        return out
    inter = inter.astype(np.float64)
    union = at[ti].astype(np.float64) + ap[pj].astype(np.float64) - inter
    # PQ (get_fast_pq): IoU without the epsilon, a match is strictly above the threshold
    iou = inter / union
    if match_iou >= 0.5:
        sel = iou > match_iou
        paired_true, paired_pred, paired_iou = ti[sel], pj[sel], iou[sel]
    else:
        rows, cols, k = _hungarian(ti, pj, iou, nt, npred)
        got = np.where(k >= 0, iou[np.maximum(k, 0)], 0.0) if len(iou) else np.zeros(len(k))
        sel = got > match_iou
        paired_true, paired_pred, paired_iou = rows[sel], cols[sel], got[sel]
    pt, pp = set(paired_true.tolist()), set(paired_pred.tolist())
    unpaired_true = [i for i in range(nt) if i not in pt]
    unpaired_pred = [j for j in range(npred) if j not in pp]
    tp, fp, fn = len(paired_true), len(unpaired_pred), len(unpaired_true)
    dq = tp / (tp + 0.5 * fp + 0.5 * fn)
    sq = float(paired_iou.sum()) / (tp + 1.0e-6)
    # AJI (get_fast_aji): IoU with the epsilon, per true instance the FIRST maximum, a pred may serve several
    iou_e = inter / (union + 1.0e-6)
    order = np.lexsort((pj, -iou_e, ti))
    first = order[np.r_[True, ti[order][1:] != ti[order][:-1]]] if len(ti) else order
    first = first[iou_e[first] > 0.0]
    a_pred = set(pj[first].tolist())
    a_true = set(ti[first].tolist())
    rest = sum(float(at[i]) for i in range(nt) if i not in a_true) + sum(float(ap[j]) for j in range(npred) if j not in a_pred)
    den = float(union[first].sum()) + rest
    aji = float(inter[first].sum()) / den if den > 0 else nan
    # AJI+ (get_fast_aji_plus): Hungarian on the same IoU
    rows, cols, k = _hungarian(ti, pj, iou_e, nt, npred)
    k = k[k >= 0]
    k = k[iou_e[k] > 0.0]
    b_true, b_pred = set(ti[k].tolist()), set(pj[k].tolist())
    rest = sum(float(at[i]) for i in range(nt) if i not in b_true) + sum(float(ap[j]) for j in range(npred) if j not in b_pred)
    den = float(union[k].sum()) + rest
    aji_plus = float(inter[k].sum()) / den if den > 0 else nan
    # get_fast_dice_2: over the pairs; get_dice_1: foreground against foreground
    total = float((at[ti].astype(np.float64) + ap[pj].astype(np.float64)).sum())
    dice2 = 2.0 * float(inter.sum()) / total if total > 0 else nan
    fg = float(at.sum()) + float(ap.sum())
    dice1 = 2.0 * float(inter.sum()) / fg if fg > 0 else nan
    return dict(dq=dq, sq=sq, pq=dq * sq, aji=aji, aji_plus=aji_plus, dice2=dice2, dice1=dice1, tp=tp, fp=fp, fn=fn,
                paired_true=paired_true.tolist(), paired_pred=paired_pred.tolist(), unpaired_true=unpaired_true, unpaired_pred=unpaired_pred)


def _subset(ti, pj, inter, at, ap, keep_t, keep_p, match_iou):
    """_core on the true instances keep_t and the predicted instances keep_p (0-based, ascending), lists back as 1-based ids"""
    new_t = np.full(len(at), -1, dtype=np.int64)
    new_p = np.full(len(ap), -1, dtype=np.int64)
    new_t[keep_t] = np.arange(len(keep_t))
    new_p[keep_p] = np.arange(len(keep_p))
    sel = (new_t[ti] >= 0) & (new_p[pj] >= 0) if len(ti) else np.zeros(0, dtype=bool)
    out = _core(new_t[ti[sel]], new_p[pj[sel]], inter[sel], at[keep_t], ap[keep_p], match_iou)
    for name, ids in (("paired_true", keep_t), ("unpaired_true", keep_t), ("paired_pred", keep_p), ("unpaired_pred", keep_p)):
        out[name] = [int(ids[i]) + 1 for i in out[name]]
    return out


def instance_scores_from_tables(pairs, area_t, area_p, match_iou: float = 0.5, cls_t=None, cls_p=None) -> Dict:
    """The reference's instance scores from the three tables.  pairs [P, 3]: rows (i, j, |true == i and pred == j|) of the non-empty pairs,
    ids from 1; area_t [nt], area_p [np]: voxels per instance.  Returns dq, sq, pq, tp, fp, fn, the lists paired_true / paired_pred /
    unpaired_true / unpaired_pred (ids from 1, as get_fast_pq returns them), aji, aji_plus, dice2, dice1, all float64 arithmetic:
      * PQ: IoU = inter / union, a match is IoU > match_iou (strictly); below 0.5 the pairing is linear_sum_assignment on the dense negated
        IoU matrix; SQ = sum of the matched IoU / (tp + 1e-6), DQ = tp / (tp + fp / 2 + fn / 2);
      * AJI: IoU = inter / (union + 1e-6), every true instance takes its first maximum (the smallest pred id among equals); AJI+: the same
        IoU through linear_sum_assignment; unpaired instances of both sides join the union;
      * dice2 = 2 sum(inter) / sum(area_t[i] + area_p[j]) over the pairs, dice1 = 2 sum(inter) / (sum(area_t) + sum(area_p));
      * every score is NaN when either side has no instance (function.py:627-634); dice2 also when no pair exists (the reference divides
        0 by 0 there).
    The dense matrices of the Hungarian paths hold at most DENSE_CAP entries: more raises ValueError.
    cls_t [nt] / cls_p [np] (both or none): the class of every instance.  Pairs across classes are dropped before anything is computed, and
    the result carries per_class = {class: the same dictionary over the instances of that class} -- per-organ PQ."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 3)
    at, ap = np.asarray(area_t, dtype=np.int64).reshape(-1), np.asarray(area_p, dtype=np.int64).reshape(-1)
    ti, pj, inter = pairs[:, 0] - 1, pairs[:, 1] - 1, pairs[:, 2]
    if len(ti) and (ti.min() < 0 or ti.max() >= len(at) or pj.min() < 0 or pj.max() >= len(ap) or inter.min() < 1):
        raise ValueError("instance scores: a pair row names an instance outside the area tables or an empty intersection")
    order = np.lexsort((pj, ti))
    ti, pj, inter = ti[order], pj[order], inter[order]
    if (cls_t is None) != (cls_p is None):
        raise ValueError("instance scores: cls_t and cls_p go together")
    all_t, all_p = np.arange(len(at)), np.arange(len(ap))
    if cls_t is None:
        return _subset(ti, pj, inter, at, ap, all_t, all_p, match_iou)
    ct, cp = np.asarray(cls_t, dtype=np.int64).reshape(-1), np.asarray(cls_p, dtype=np.int64).reshape(-1)
    if len(ct) != len(at) or len(cp) != len(ap):
        raise ValueError("instance scores: cls_t / cls_p must name a class per instance")
    same = ct[ti] == cp[pj]
    ti, pj, inter = ti[same], pj[same], inter[same]
    out = _subset(ti, pj, inter, at, ap, all_t, all_p, match_iou)
    out["per_class"] = {int(c): _subset(ti, pj, inter, at, ap, all_t[ct == c], all_p[cp == c], match_iou)
                        for c in sorted(set(ct.tolist()) | set(cp.tolist()))}
    return out


# ---- device half ----------------------------------------------------------------------------------------------------------------------
def remap_instances(map, labels=None, id_bound: Optional[int] = None, by_size: bool = False, max_instances: int = MAX_INSTANCES):
    """remap_label (stats_utils.py:362-391) on the device -> (out, orig, size, cls, info): the map with contiguous ids 1 .. n and the
    tables of `ops.instance_remap` (original id, voxel count, largest value of the uint8 volume `labels` over the instance; max_instances rows).
    by_size=False: ascending original id (np.unique's order).  by_size=True: larger instances get smaller ids, ties keep the order of the
    original ids (the reference's stable `sorted`): a stable descending torch.sort of the size table, applied with `ops.instance_apply`; the
    tables are permuted alike.  id_bound: ids are in 0 .. id_bound - 1; None = voxels + 1 (enough for `ops.label_components`' comp and for
    painted maps).  Nothing is copied to the host: the caller reads info = (instances found, voxels with an id outside the bound -- they
    became background --, 1 if found > max_instances, 0)."""
    import torch
    from . import ops
    bound = map.numel() + 1 if id_bound is None else int(id_bound)
    out, orig, size, cls, info = ops.instance_remap(map, bound, max_instances, labels)
    if by_size:
        order = torch.sort(size, descending=True, stable=True).indices      # empty rows (size 0) stay behind every instance
        table = torch.zeros(max_instances + 1, dtype=torch.int32, device=map.device)
        table[order + 1] = torch.arange(1, max_instances + 1, dtype=torch.int32, device=map.device)
        ops.instance_apply(out, table, out=out)
        orig, size, cls = orig[order].contiguous(), size[order].contiguous(), cls[order].contiguous()
    return out, orig, size, cls, info


def instances_from_labels(labels, connectivity: int = 26, obj_ids: Optional[Sequence[int]] = None, min_voxels: int = 0,
                          max_instances: int = MAX_INSTANCES):
    """uint8 label volume [D, H, W] -> (map, orig, size, cls, info) as remap_instances gives them: one instance per connected component
    (`ops.label_components`), cls = the component's label value, orig = its canonical name (1 + smallest linear index).  Components of a value
    not in obj_ids (None = every value) or with fewer than min_voxels voxels are dropped and the ids closed up again with a keep table through
    `ops.instance_apply`; info[0] = instances kept.  Nothing is copied to the host."""
    import torch
    from . import ops
    comp, _ = ops.label_components(labels, connectivity)
    out, orig, size, cls, info = ops.instance_remap(comp, labels.numel() + 1, max_instances, labels, out=None)
    if obj_ids is None and int(min_voxels) <= 1:
        return out, orig, size, cls, info
    dev = labels.device
    keep = size >= max(1, int(min_voxels))
    if obj_ids is not None:
        wanted = torch.zeros(256, dtype=torch.bool)
        wanted[[int(v) for v in obj_ids]] = True
        keep &= wanted.to(dev)[cls.long()]
    new_id = torch.cumsum(keep.to(torch.int32), 0, dtype=torch.int32)
    table = torch.zeros(max_instances + 1, dtype=torch.int32, device=dev)
    table[1:] = torch.where(keep, new_id, torch.zeros_like(new_id))
    ops.instance_apply(out, table, out=out)
    slot = torch.where(keep, new_id.long() - 1, torch.full_like(new_id, max_instances).long())    # dropped rows go to a spare row
    packed = []
    for t in (orig, size, cls):
        p = torch.zeros(max_instances + 1, dtype=torch.int32, device=dev)
        p[slot] = t
        packed.append(p[:max_instances].contiguous())
    info = info.clone()
    info[0] = torch.where(info[2] > 0, info[0], new_id[-1])     # (an overflowing table stays flagged: info[2])
    return out, packed[0], packed[1], packed[2], info


def paint_instances(masks, order=None, boxes=None, skip_covered: bool = True):
    """The instance map the reference paints from its predicted masks (func_2d/function.py:620-624): masks [N, H, W] (bool or uint8, non-zero =
    inside) painted in `order` (mask indices; None = as stacked), a mask that finds no 0 left under it is skipped, the others overwrite.
    boxes [N, 4] = (x0, y0, x1, y1) inclusive per mask restrict the work.  -> int32 [H, W] on the device."""
    import torch
    from . import ops
    m = masks if masks.dtype == torch.uint8 else (masks != 0).to(torch.uint8)
    dev = m.device
    o = None if order is None else torch.as_tensor(order).to(device=dev, dtype=torch.int32).contiguous()
    b = None if boxes is None else torch.as_tensor(boxes).to(device=dev, dtype=torch.int32).contiguous()
    return ops.instance_paint(m.contiguous(), o, b, skip_covered)


def instance_tables(true, pred, max_pairs: Optional[int] = None, max_instances: int = MAX_INSTANCES, labels_true=None, labels_pred=None,
                    remapped: bool = False, cls=None, infos=None):
    """Two instance maps of one shape -> the host tables (pairs int64 [P, 3], area_t [nt], area_p [np], cls_t [nt], cls_p [np]) with ONE
    device-to-host copy.  The maps are remapped first (`ops.instance_remap`, ids below voxels + 1; labels_true / labels_pred: uint8 volumes
    that give every instance its class) unless remapped=True says their ids are contiguous already (cls: the two device class tables of
    max_instances rows, or None; infos: the two info tables of the calls that made the maps, or None).  max_pairs: rows of the pair table, None = 4 x max_instances.  Raises when a table overflows or an id is
    outside its range."""
    import torch
    from . import ops
    cap = 4 * max_instances if max_pairs is None else int(max_pairs)
    dev = true.device
    zero4 = torch.zeros(4, dtype=torch.int32, device=dev)
    if remapped:
        a, b = true, pred
        info_t, info_p = infos if infos is not None else (zero4, zero4)
        cls_t, cls_p = cls if cls is not None else (torch.zeros(max_instances, dtype=torch.int32, device=dev),) * 2
    else:
        a, _, _, cls_t, info_t = ops.instance_remap(true, true.numel() + 1, max_instances, labels_true)
        b, _, _, cls_p, info_p = ops.instance_remap(pred, pred.numel() + 1, max_instances, labels_pred)
    pairs, area_t, area_p, info = ops.instance_pairs(a, b, max_instances, max_instances, cap)
    host = torch.cat([info_t, info_p, info, cls_t, cls_p, area_t, area_p, pairs.reshape(-1)]).cpu().numpy().astype(np.int64)
    it, ip, ipr = host[0:4], host[4:8], host[8:12]
    M = max_instances
    cls_t, cls_p, area_t, area_p = (host[12 + k * M: 12 + (k + 1) * M] for k in range(4))
    rows = host[12 + 4 * M:].reshape(-1, 3)
    if it[2] or ip[2]:
        raise ValueError(f"instance_tables: {it[0]} true and {ip[0]} predicted instances, the tables hold max_instances = {M}")
    if it[1] or ip[1] or ipr[2] or ipr[3]:
        raise ValueError(f"instance_tables: ids outside the range ({it[1]} + {ipr[2]} voxels of true, {ip[1]} + {ipr[3]} of pred): pass maps with "
                         f"non-negative ids below voxels + 1, remapped ones with ids up to max_instances = {M}")
    if ipr[1]:
        raise ValueError(f"instance_tables: more than max_pairs = {cap} pairs of instances intersect")
    if remapped:
        nt = int(np.flatnonzero(area_t).max() + 1) if area_t.any() else 0
        npred = int(np.flatnonzero(area_p).max() + 1) if area_p.any() else 0
    else:
        nt, npred = int(it[0]), int(ip[0])
    return rows[: int(ipr[0])], area_t[:nt], area_p[:npred], cls_t[:nt], cls_p[:npred]


def instance_scores(true, pred, match_iou: float = 0.5, labels_true=None, labels_pred=None, max_pairs: Optional[int] = None,
                    max_instances: int = MAX_INSTANCES) -> Dict:
    """remap_label on both maps + get_fast_pq / get_fast_aji / get_fast_aji_plus / get_fast_dice_2 / get_dice_1 (function.py:636-642): the tables
    on the device, one host copy, `instance_scores_from_tables`.  With labels_true and labels_pred (uint8 volumes of the maps' shape) every
    instance has a class and the scores come per class as well."""
    pairs, at, ap, ct, cp = instance_tables(true, pred, max_pairs, max_instances, labels_true, labels_pred)
    with_cls = labels_true is not None and labels_pred is not None
    return instance_scores_from_tables(pairs, at, ap, match_iou, ct if with_cls else None, cp if with_cls else None)
