"""End of the 3-D path: from the low-res logits that `volume.segment_volume` returns to a label volume (one uint8 per voxel: organ id or 0)
and per-organ scores against a ground-truth label volume, without ever writing the up-sampled logits.

The reference's validation (`func_3d/function.py:215-330`) up-samples every slice's logits to video resolution and scores every
(slice, object) pair with an `eval_seg` call of its own (one device-to-host copy each).  Here `ops.label_slices` (csrc/volume_labels.hip)
re-evaluates the bilinear resize per voxel, `label_volume` feeds it the slices chunk by chunk, and the counts of the whole volume
[K, T, n, 3] cross to the host once, in `volume_scores`.

Label rule (per voxel): the highest-scoring object above `label_thr` (0: the mask threshold of the video predictor), ties to the lower
object index, 0 = background -- the per-pixel rule of the reference's non-overlapping constraint (`sam2_base.py:812-830`) applied at
video resolution.  Counts are taken per object on its own (`exclusive=False`: what the reference's validation scores) or on the label
volume (`exclusive=True`).

Between the label volume and its scores sits the usual post-processing, on the device as well: `clean_labels` keeps the largest component of
every organ and drops islands (csrc/components.hip), `fill_holes` fills the cavities enclosed by an organ, 3-D or slice by slice
(csrc/holes.hip: scipy.ndimage.binary_fill_holes per organ), and `postprocess_labels` runs the two in that order; `morph_labels` erodes,
dilates, opens or closes every organ with a ball of a radius in millimetres (csrc/morph.hip).

Where no ground truth exists the organs are measured: `organ_measurements` (csrc/measure.hip: one pass over the label volume and the
image, five small integer tables) gives volume, extent, centroid, covariance and principal axes, the voxel-face surface area and the
intensity statistics inside every organ (mean, spread, range, percentiles, histogram); `measurements_from_tables` is its host half,
`measurement_errors` compares two such reports (relative volume difference, centroid distance).  `organ_meshes` (csrc/mesh.hip) gives the
surface of every organ as a closed quad mesh on the device -- surface nets or the voxel faces -- for a viewer, a printer or a planning
tool (`meshes.OrganMesh`: area, enclosed volume, STL / OBJ / PLY); `mesh_measurements` reports its area and volume.

How far to trust them, still without a ground truth: `volume_confidence` (`ops.label_confidence`, csrc/volume_labels.hip) repeats
`label_volume`'s pass and keeps what the arg-max drops -- per voxel the margin by which the decision held, against bands given in logit units
(`margins_from_probabilities`) -- as a confidence map, a confident core volume, a generous envelope volume and integer tables per (slice, organ);
`slice_consistency` counts the overlap of adjacent slices; `confidence_report` is the host half: volume intervals in mL, uncertain fractions,
adjacent-slice Dice.  Core and envelope are label volumes, so every entry above (measurements, surface distances, clicks) applies to them."""
from __future__ import annotations

import math
from fractions import Fraction

from typing import Dict, Optional, Sequence, Union

import numpy as np
import torch

from . import ops
from .metrics import scores_from_counts

F32 = torch.float32
REFERENCE_THRESHOLDS = (0.1, 0.3, 0.5, 0.7, 0.9)


def _masks_layout(masks):
    """the two forms of `masks` -> (slice keys in ascending order | None for a tensor, T, n, device)"""
    if isinstance(masks, torch.Tensor):
        assert masks.dim() == 4, "masks: [T, n, h, w]"
        return None, masks.shape[0], masks.shape[1], masks.device
    order = sorted(masks)
    first = masks[order[0]]
    assert first.dim() == 4 and first.shape[1] == 1, "masks: {slice: [n, 1, h, w]}"
    return order, len(order), first.shape[0], first.device


def _chunk(masks, order, i: int, j: int) -> torch.Tensor:
    """slices order[i:j] as one contiguous fp32 [j - i, n, h, w] tensor (the only copy of logits this module makes)"""
    if isinstance(masks, torch.Tensor):
        return masks[i:j].to(F32).contiguous()
    return torch.stack([masks[t][:, 0] for t in order[i:j]]).to(F32).contiguous()


@torch.no_grad()
def label_volume(masks: Union[Dict[int, torch.Tensor], torch.Tensor], H: int, W: int, obj_ids: Optional[Sequence[int]] = None,
                 gt: Optional[torch.Tensor] = None, thresholds=REFERENCE_THRESHOLDS, exclusive: bool = False, slices_per_call: int = 8,
                 label_thr: float = 0.0):
    """masks: {slice: [n, 1, h, w]} as `segment_volume` returns it (slices in ascending key order) or a [T, n, h, w] tensor, on the GPU.
    obj_ids: the label value of each object (default 1 .. n; distinct, 1 .. 255).  Returns labels uint8 [T, H, W] on the device; with
    gt (uint8 [T, H, W] label volume, e.g. `labels_from_pack`) returns (labels, counts): counts int32 [K, T, n, 3] on the device =
    (|P & G|, |P|, |G|) per threshold, slice and object (see `ops.label_slices`), for `volume_scores`.  The slices go through
    `slices_per_call` at a time, so no copy of the logits is larger than one chunk; nothing is copied to the host."""
    order, T, n, dev = _masks_layout(masks)
    H, W = int(H), int(W)
    ids = ops.label_ids(list(range(1, n + 1)) if obj_ids is None else obj_ids, dev)
    assert ids.numel() == n, f"{n} objects need {n} ids"
    labels = torch.empty(T, H, W, dtype=torch.uint8, device=dev)
    counts, thr = None, []
    if gt is not None:
        assert gt.dtype == torch.uint8 and tuple(gt.shape) == (T, H, W), f"gt: uint8 [{T}, {H}, {W}]"
        gt = gt.to(dev).contiguous()
        thr = [float(t) for t in thresholds]
        assert thr, "scores need at least one threshold"
        counts = torch.empty(len(thr), T, n, 3, dtype=torch.int32, device=dev)
    step = max(1, int(slices_per_call))
    for i in range(0, T, step):
        j = min(T, i + step)
        x = _chunk(masks, order, i, j)
        if counts is None:
            ops.label_slices(x, ids, H, W, label_thr, labels=labels[i:j])
            continue
        for k in range(0, len(thr), ops.LABEL_MAX_THRESHOLDS):            # at most 8 thresholds per launch; the labels with the first
            part = thr[k: k + ops.LABEL_MAX_THRESHOLDS]
            _, c = ops.label_slices(x, ids, H, W, label_thr, gt=gt[i:j], thresholds=part, exclusive=exclusive,
                                    labels=labels[i:j] if k == 0 else False)
            counts[k: k + len(part), i:j] = c
    return labels if counts is None else (labels, counts)


def volume_scores(counts) -> dict:
    """Scores from `label_volume`'s counts [K, T, n, 3] (device tensor: the one device-to-host copy of the path; or a numpy array).

    * "iou", "dice": the reference's validation figures (`func_3d/function.py:300-330`): the mean over (slice, object) of eval_seg's
      threshold-averaged IoU / Dice -- the arithmetic, smoothing constants and float types of `metrics.eval_seg` (shared code);
      "iou_per_pair" / "dice_per_pair" [T, n] hold what eval_seg returns for each pair.
    * "volume_dice", "volume_iou" float64 [K, n]: per organ and threshold from the counts summed over the slices in int64,
      2 I / (P + G) and I / (P + G - I); NaN where an organ is neither predicted nor present."""
    k = counts.cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
    k = k.astype(np.int64)
    K, T, n, _ = k.shape
    ious, dices = scores_from_counts(k.reshape(K, 1, T * n, 3))           # every (slice, object) as eval_seg sees it: b = c = 1
    iou = dice = 0.0
    for a, b in zip(ious, dices):                                         # the running sums of validate_volume, in its order
        iou, dice = iou + a, dice + b
    vol = k.sum(axis=1)                                                   # [K, n, 3] int64
    inter, ps, gs = (vol[..., i].astype(np.float64) for i in range(3))
    with np.errstate(divide="ignore", invalid="ignore"):
        v_dice = 2.0 * inter / (ps + gs)
        v_iou = inter / (ps + gs - inter)
    return {"iou": iou / (T * n), "dice": dice / (T * n),
            "iou_per_pair": np.array(ious, dtype=np.float64).reshape(T, n), "dice_per_pair": np.array(dices, dtype=np.float64).reshape(T, n),
            "volume_dice": v_dice, "volume_iou": v_iou}


def labels_from_pack(label: Dict[int, Dict[int, torch.Tensor]], obj_list: Sequence[int], device=None) -> torch.Tensor:
    """The data contract's ground truth (`data.BTCVVolumes[i]["label"]`: {frame: {obj: [1, S, S] int mask}}, frames 0 .. T-1) as one uint8
    [T, S, S] label volume: voxel = obj where that object's mask is set, 0 elsewhere (where masks overlap, the object later in obj_list).
    Built on the host, moved to `device` in one copy."""
    frames = sorted(label)
    assert frames == list(range(len(frames))), "frames must be 0 .. T-1"
    assert all(1 <= int(o) <= 255 for o in obj_list), "object ids must be 1 .. 255"
    shape = next((tuple(m.shape[-2:]) for f in frames for m in label[f].values()), None)
    assert shape is not None, "no mask in the pack"
    vol = torch.zeros(len(frames), *shape, dtype=torch.uint8)
    for f in frames:
        for o in obj_list:
            m = label[f].get(o)
            if m is not None:
                vol[f][torch.as_tensor(m).reshape(shape) > 0] = int(o)
    return vol if device is None else vol.to(device)


def _resolve_ids(what: str, labels: torch.Tensor, obj_ids, n):
    """obj_ids / n as `clean_labels` documents them -> the ids on labels' device"""
    if obj_ids is None:
        assert n is not None and int(n) >= 1, f"{what}: without obj_ids the number of objects n is needed (the volume is not scanned)"
        obj_ids = list(range(1, int(n) + 1))
    dev = labels.device
    on_dev = isinstance(obj_ids, torch.Tensor) and obj_ids.device == dev and dev.type != "cpu"
    ids = obj_ids if on_dev else ops.label_ids(obj_ids, dev)
    assert n is None or ids.numel() == int(n), f"{what}: {ids.numel()} ids for n = {n}"
    return ids


@torch.no_grad()
def clean_labels(labels: torch.Tensor, obj_ids: Optional[Sequence[int]] = None, connectivity: int = 26, keep_largest=True, min_voxels=0,
                 in_place: bool = False, n: Optional[int] = None):
    """Island removal between `label_volume` and the scores: the components of every listed value of the uint8 [T, H, W] label volume
    (`ops.label_components`: 6 / 18 / 26 in 3-D, 4 / 8 slice by slice), of which only the largest per value (`keep_largest`) with at least
    `min_voxels` voxels survive (`ops.label_clean`); voxels of other values stay.  keep_largest / min_voxels: one value, or one per object.
    obj_ids: the label values (distinct, 1 .. 255; a device tensor of `ops.label_ids` is taken as is); None = 1 .. n with `n` given by the
    caller -- the volume is never scanned on the host.  Returns (cleaned uint8 [T, H, W], info int32 [n, 6]) on the device, info =
    (components found, voxels found, largest size, its canonical name or 0, components kept, voxels kept); in_place=True overwrites labels."""
    ids = _resolve_ids("clean_labels", labels, obj_ids, n)
    comp, size = ops.label_components(labels, connectivity)
    mv = None if isinstance(min_voxels, int) and min_voxels == 0 else min_voxels
    return ops.label_clean(labels, comp, size, ids, min_voxels=mv, keep_largest=keep_largest, out=labels if in_place else None)


@torch.no_grad()
def fill_holes(labels: torch.Tensor, obj_ids: Optional[Sequence[int]] = None, connectivity: int = 6, max_voxels=0, claim: str = "background",
               in_place: bool = False, n: Optional[int] = None):
    """Hole filling after `clean_labels`: scipy.ndimage.binary_fill_holes per organ of the uint8 [T, H, W] label volume on the device
    (`ops.label_fill_holes`).  `connectivity` is that of the background flood: 6 (scipy's default) / 18 / 26 in 3-D, 4 / 8 slice by slice.
    A hole of an organ is a component of the voxels that are not the organ's which does not reach the frame; holes of more than
    `max_voxels` voxels stay (0: no limit; one value, or one per object); claim="background" fills only the background voxels of a hole,
    "any" also an enclosed lesion of another label.  A voxel in the holes of several organs goes to the one first in obj_ids.
    obj_ids / n: as `clean_labels` takes them.  Returns (filled uint8 [T, H, W], info int32 [n, 4]) on the device, info = (holes found, voxels
    in them, holes that qualify, voxels the organ gained); in_place=True overwrites labels."""
    ids = _resolve_ids("fill_holes", labels, obj_ids, n)
    mv = None if isinstance(max_voxels, int) and max_voxels == 0 else max_voxels
    return ops.label_fill_holes(labels, ids, connectivity, max_voxels=mv, claim=claim, out=labels if in_place else None)


@torch.no_grad()
def morph_labels(labels: torch.Tensor, obj_ids: Optional[Sequence[int]] = None, op: str = "close", radius=1.0, spacing=(1.0, 1.0, 1.0),
                 claim: str = "background", in_place: bool = False, n: Optional[int] = None, radius2=None):
    """Morphology with a ball of a physical radius on the uint8 [T, H, W] label volume, per organ, on the device (`ops.label_morph`): op =
    "erode" / "dilate" / "open" / "close", `radius` in the unit of `spacing` = (sz, sy, sx), one value or one per object.  An opening drops the
    thin bridge that joins a leak to an organ (which `clean_labels` cannot: the bridge makes them one component); a closing fills the notches
    and gaps open to the background that `fill_holes` leaves; a dilation is a margin that stops at the neighbours, an erosion a safe core.
    The ball is d2 <= r2 with r2 = float(radius) * float(radius); `radius2` (then radius is ignored) gives r2 directly -- (3 ** 0.5) ** 2 ==
    2.9999999999999996, so radius=sqrt(3) does not reach a voxel at d2 = 3 and radius2=3.0 does.  An organ cut by the field of view does not
    erode from the frame.  dilate / close change only eligible voxels (claim="background": input value 0; "any": any value not in obj_ids), a
    voxel several organs reach goes to the one whose original mask is nearest, ties to the one earlier in obj_ids.
    obj_ids / n: as `clean_labels` takes them.  Returns (labels uint8 [T, H, W], info int32 [n, 4]) on the device, info = (voxels before, voxels
    in the organ's own result set, voxels after, voxels taken from non-zero values); in_place=True overwrites labels."""
    ids = _resolve_ids("morph_labels", labels, obj_ids, n)
    r = dict(radius2=radius2) if radius2 is not None else dict(radius=radius)
    return ops.label_morph(labels, ids, op, spacing=spacing, claim=claim, out=labels if in_place else None, **r)


@torch.no_grad()
def postprocess_labels(labels: torch.Tensor, obj_ids: Optional[Sequence[int]] = None, connectivity: int = 26, keep_largest=True, min_voxels=0,
                       hole_connectivity: int = 6, max_voxels=0, claim: str = "background", in_place: bool = False, n: Optional[int] = None):
    """The usual abdominal post-processing between `label_volume` and the scores: `clean_labels` (connectivity, keep_largest, min_voxels),
    then `fill_holes` (hole_connectivity, max_voxels, claim) on its result.  Returns (labels, clean_info int32 [n, 6], hole_info int32 [n, 4])
    on the device; in_place=True overwrites labels."""
    ids = _resolve_ids("postprocess_labels", labels, obj_ids, n)
    cleaned, clean_info = clean_labels(labels, ids, connectivity, keep_largest, min_voxels, in_place=in_place)
    filled, hole_info = fill_holes(cleaned, ids, hole_connectivity, max_voxels, claim, in_place=True)
    return filled, clean_info, hole_info


@torch.no_grad()
def label_scores(pred: torch.Tensor, gt: torch.Tensor, obj_ids) -> dict:
    """Scores of a label volume (e.g. `clean_labels`' output) against the ground-truth label volume, both uint8 [T, H, W] on the device:
    `ops.label_overlap`'s counts [T, n, 3] as `volume_scores`' [1, T, n, 3] -- its keys and arithmetic at K = 1 (a label volume has no
    threshold left), with the path's one device-to-host copy inside it."""
    counts = ops.label_overlap(pred, gt, obj_ids)
    return volume_scores(counts[None])


@torch.no_grad()
def lesion_scores(pred: torch.Tensor, gt: torch.Tensor, obj_ids, connectivity: int = 26, match_iou: float = 0.5, min_voxels: int = 0,
                  spacing=None, max_instances: Optional[int] = None) -> dict:
    """Lesion-wise detection scores of a label volume against the ground truth, both uint8 [D, H, W] on the device: "7 of 9 lesions found, 2
    false positives", the number tumour and lesion work reports beside Dice; per organ it is panoptic quality proper.  Every connected
    component (`connectivity`, at least `min_voxels` voxels) of a value in obj_ids is an instance of that organ (`instances.instances_from_labels`
    on both volumes); a predicted lesion is found iff its IoU with a true lesion of the same organ is > match_iou (csrc/instances.hip's pair
    table, one device-to-host copy, `instances.instance_scores_from_tables` with the organ as the class).  Per organ, in the order of
    obj_ids, lists under: "tp", "fp", "fn", "f1" (= DQ), "sq", "pq", "aji", "missed" / "spurious" (the sizes of the unmatched true / predicted
    lesions, ascending lesion id: voxels, or mm^3 with spacing = (sz, sy, sx)), "true_lesions", "pred_lesions"; "overall": the whole score
    dictionary over all organs, pairs across organs dropped."""
    from . import instances as inst
    ids = [int(v) for v in obj_ids]
    M = inst.MAX_INSTANCES if max_instances is None else int(max_instances)
    g_map, _, _, g_cls, g_info = inst.instances_from_labels(gt, connectivity, ids, min_voxels, M)
    p_map, _, _, p_cls, p_info = inst.instances_from_labels(pred, connectivity, ids, min_voxels, M)
    pairs, at, ap, ct, cp = inst.instance_tables(g_map, p_map, None, M, remapped=True, cls=(g_cls, p_cls), infos=(g_info, p_info))
    s = inst.instance_scores_from_tables(pairs, at, ap, match_iou, ct, cp)
    unit = 1.0 if spacing is None else float(spacing[0]) * float(spacing[1]) * float(spacing[2])
    size = (lambda a, which: [int(a[i - 1]) if spacing is None else float(a[i - 1]) * unit for i in which])
    out = {k: [] for k in ("tp", "fp", "fn", "f1", "sq", "pq", "aji", "missed", "spurious", "true_lesions", "pred_lesions")}
    empty = inst.instance_scores_from_tables(np.zeros((0, 3)), np.zeros(0), np.zeros(0), match_iou)
    for v in ids:
        c = s["per_class"].get(v, empty)
        for k, name in (("tp", "tp"), ("fp", "fp"), ("fn", "fn"), ("f1", "dq"), ("sq", "sq"), ("pq", "pq"), ("aji", "aji")):
            out[k].append(c[name])
        out["missed"].append(size(at, c["unpaired_true"]))
        out["spurious"].append(size(ap, c["unpaired_pred"]))
        out["true_lesions"].append(c["tp"] + c["fn"])
        out["pred_lesions"].append(c["tp"] + c["fp"])
    out["overall"] = s
    return out


# ---- surface distances: HD95, ASSD, NSD (MONAI's conventions) ----------------------------------------------------------------
def _sqrt_threshold(tau: float) -> float:
    """the largest float64 t with sqrt(t) <= tau (correctly rounded sqrt, monotone): #{sqrt(d2) <= tau} = #{d2 <= t} without a device sqrt"""
    tau = float(tau)
    if not tau >= 0.0:
        return -1.0                                                       # nothing is <= a negative (or NaN) tolerance
    if np.isinf(tau):
        return tau
    t = np.float64(tau) * np.float64(tau)
    while np.sqrt(t) > tau:
        t = np.nextafter(t, -np.inf)
    while np.sqrt(np.nextafter(t, np.inf)) <= tau:
        t = np.nextafter(t, np.inf)
    return float(t)


def _direction_row(seg: torch.Tensor, m: torch.Tensor, q: float, thr2: torch.Tensor) -> torch.Tensor:
    """seg: float64 [cap], ascending, its first m elements (m: 0-dim int64 tensor on seg's device) the squared distances of one direction
    -> float64 [5 + K] = (largest d2, sum of the distances, the two neighbours of the percentile position, #{d2 <= thr2[k]}, m), torch ops
    on seg's device only; an empty segment gives zeros and m"""
    count = m.reshape(1).to(torch.float64)                               # exact: far below 2^53
    if seg.numel() == 0:
        return torch.cat([torch.zeros(4 + thr2.numel(), dtype=torch.float64, device=m.device), count])
    d = torch.sqrt(seg)
    valid = torch.arange(seg.numel(), device=seg.device) < m
    last = torch.clamp(m - 1, min=0)
    lo = torch.floor(last.to(torch.float64) * q).to(torch.int64)          # numpy's virtual index (m - 1) * (percentile / 100)
    hi = torch.minimum(lo + 1, last)
    total = torch.where(valid, d, torch.zeros_like(d)).sum()
    below = (valid[:, None] & (seg[:, None] <= thr2[None, :])).sum(0).to(torch.float64)
    return torch.cat([torch.stack([seg[last], total, d[lo], d[hi]]), below, count])


def _scores(segments, percentile: float, tolerances) -> dict:
    """segments: per organ ((seg, m), (seg, m)) as `_direction_row` takes them, all on one device -> the dict of `surface_scores`.  One
    table [n, 2, 5 + K] crosses to the host: the only copy."""
    q = float(percentile) / 100.0
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"surface scores: percentile {percentile} (0 .. 100)")
    tol = [float(t) for t in tolerances]
    K, n = len(tol), len(segments)
    hd, hd95, assd, nsd = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan), np.full((n, K), np.nan)
    counts = np.zeros((n, 2), dtype=np.int64)
    if n:
        dev = segments[0][0][1].device
        thr2 = torch.tensor([_sqrt_threshold(t) for t in tol], dtype=torch.float64).to(dev)       # once per call
        table = torch.stack([_direction_row(seg, m, q, thr2) for pair in segments for seg, m in pair])
        rows = table.cpu().numpy().reshape(n, 2, 5 + K)
        counts = rows[:, :, 4 + K].astype(np.int64)
    for j in range(n):
        mp, mg = int(counts[j, 0]), int(counts[j, 1])
        if mp == 0 or mg == 0:
            continue                                                      # absent from either volume: NaN
        p95 = []
        for d, m in ((0, mp), (1, mg)):
            pos = (m - 1) * q
            t = pos - np.floor(pos)
            a, b = rows[j, d, 2], rows[j, d, 3]
            p95.append(a + (b - a) * t if t < 0.5 else b - (b - a) * (1.0 - t))   # numpy's linear interpolation, both of its branches
        hd[j] = np.sqrt(max(rows[j, 0, 0], rows[j, 1, 0]))
        hd95[j] = max(p95)
        assd[j] = (rows[j, 0, 1] + rows[j, 1, 1]) / (mp + mg)
        nsd[j] = (rows[j, 0, 4: 4 + K] + rows[j, 1, 4: 4 + K]) / (mp + mg)
    return {"hd": hd, "hd95": hd95, "assd": assd, "nsd": nsd, "surface_voxels": counts}


def surface_scores_from_distances(lists, percentile: float = 95.0, tolerances=(1.0,)) -> dict:
    """The scores from sorted squared-distance lists: lists[j] = (d2 of pred's surface voxels to gt's surface, d2 of gt's to pred's), each a
    1-D ascending float64 sequence (tensor, array or list; empty where the organ is absent).  Per organ, with d = sqrt(d2):
    hd = the largest d of both lists; hd95 = the larger of the two lists' `percentile` (numpy's default linear percentile);
    assd = (sum d_pg + sum d_gp) / (|S_p| + |S_g|); nsd [n, K] = (#{d_pg <= tau} + #{d_gp <= tau}) / (|S_p| + |S_g|) per tolerance;
    surface_voxels int64 [n, 2] = (|S_p|, |S_g|).  All four are NaN when either list is empty.  float64 numpy arrays."""
    segments = []
    for pair in lists:
        if len(pair) != 2:
            raise ValueError("surface scores: one (pred -> gt, gt -> pred) pair of lists per organ")
        ts = [(x.to(torch.float64) if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x, dtype=np.float64))).reshape(-1) for x in pair]
        segments.append([(t, torch.tensor(t.numel(), device=t.device)) for t in ts])
    return _scores(segments, percentile, tolerances)


@torch.no_grad()
def surface_scores(pred: torch.Tensor, gt: torch.Tensor, obj_ids, spacing=(1.0, 1.0, 1.0), percentile: float = 95.0, tolerances=(1.0,),
                   workspace_bytes: int = ops.SURFACE_WORKSPACE_BYTES) -> dict:
    """HD, HD95, ASSD and NSD per organ of a label volume against the ground truth, both uint8 [T, H, W] on the device, spacing (sz, sy, sx)
    in millimetres: `ops.surface_segments` (exact squared distances of every surface voxel to the other surface), then sorting, sqrt,
    sums, the percentile gather and the tolerance counts as torch ops on the device; one small table [n, 2, 5 + K], the surface counts in
    it, crosses to the host at the end.  Keys and conventions: `surface_scores_from_distances`."""
    dist, offs, caps, counts = ops.surface_segments(pred, gt, obj_ids, spacing, workspace_bytes)
    counts64 = counts.to(torch.int64)
    segments = [[(torch.sort(dist[offs[j][d]: offs[j][d] + caps[j][d]]).values, counts64[j, d]) for d in range(2)]   # +inf beyond the count sorts last
                for j in range(len(offs))]
    return _scores(segments, percentile, tolerances)


# ---- measurements: volume, shape, surface, intensity per organ ---------------------------------------------------------------
DEFAULT_HIST_RANGE = {torch.int16: (-1024, 3072), torch.uint8: (0, 256)}     # [lo, hi): Hounsfield units / the grey of the intake


def _order_statistic(cum: np.ndarray, below: int, hist_lo: int, k: int) -> float:
    """the k-th smallest value (k from 0) of an organ from its cumulative histogram (cum[b] = voxels with v <= hist_lo + b inside the range);
    NaN when it lies in a clipped tail"""
    k -= below
    if k < 0 or len(cum) == 0 or k >= int(cum[-1]):
        return float("nan")
    return float(hist_lo + int(np.searchsorted(cum, k, side="right")))


def measurements_from_tables(moments, extent, vrange=None, faces=None, hist=None, hist_lo: int = 0, spacing=(1.0, 1.0, 1.0),
                             percentiles=(5, 25, 50, 75, 95)) -> dict:
    """The report from `ops.label_measure`'s tables as numpy arrays (vrange None: no image; faces / hist None: skipped), all indexed by organ.

    Geometry: "voxels" int64; "volume_mm3", "volume_ml"; "bbox" int64 [n, 6] = inclusive (z0, z1, y0, y1, x0, x1), -1 when absent; "extent_mm"
    [n, 3]; "centroid_vox", "centroid_mm" [n, 3]: the mean of the voxel centres in (z, y, x), in indices and times the spacing;
    "covariance_mm2" [n, 3, 3] (population covariance of the voxel centres); "principal_lengths_mm" [n, 3] = 4 sqrt(eigenvalue), descending,
    and "principal_axes" [n, 3, 3]: row k = the unit vector (z, y, x) of the k-th longest axis, its largest component positive
    (np.linalg.eigh of the covariance).  With faces: "surface_mm2" = interior faces times the face area per axis -- the VOXEL-FACE area: it
    over-estimates a smooth surface (by up to sqrt(3); 1.5 on a large sphere) and depends neither on scheduling nor on a mesher;
    "frame_faces" int64 [n, 3] = the organ's faces on the volume's frame per axis z, y, x, "touches_frame" = any of them: the field of view
    cuts the organ, its volume is a lower bound.
    Intensity (vrange given): "mean", "std" (population), "min", "max", "clipped" int64 [n, 2] = voxels (below, at or above) the histogram
    range; with hist: "percentiles" [n, len(percentiles)], "percentile_bounds" [n, len(percentiles), 2] (the two order statistics each one
    interpolates), "hist", "hist_lo".
    Means, variances and covariances come from the integer sums in exact rational arithmetic and are rounded to float64 once (the variance
    is (count Svv - Sv^2) / count^2; Svv / count - mean^2 cancels and is not used).  A percentile follows numpy's "linear" definition:
    virtual index q / 100 (count - 1), the two order statistics read exactly from the cumulative histogram, interpolated in float64; it
    is NaN if either order statistic lies in a clipped tail -- nothing is clamped.  Absent organs: NaN for float figures, 0 for counts,
    -1 for boxes."""
    M = np.asarray(moments).astype(np.int64).reshape(-1, 14)
    E = np.asarray(extent).astype(np.int64).reshape(-1, 6)
    n = M.shape[0]
    sp = tuple(float(s) for s in spacing)
    assert len(sp) == 3 and all(s > 0.0 for s in sp), "spacing: three positive values (sz, sy, sx)"
    nan = float("nan")
    count = M[:, 0].copy()
    out = {"voxels": count, "volume_mm3": count.astype(np.float64) * (sp[0] * sp[1] * sp[2]), "bbox": E.copy()}
    out["volume_ml"] = out["volume_mm3"] / 1000.0
    ext_mm, cen, cov = np.full((n, 3), nan), np.full((n, 3), nan), np.full((n, 3, 3), nan)
    plen, pax = np.full((n, 3), nan), np.full((n, 3, 3), nan)
    second = {(0, 0): 4, (1, 1): 5, (2, 2): 6, (0, 1): 7, (0, 2): 8, (1, 2): 9}
    for j in range(n):
        c = int(count[j])
        if c == 0:
            continue
        s1 = [int(M[j, 1 + a]) for a in range(3)]
        for a in range(3):
            ext_mm[j, a] = float(int(E[j, 2 * a + 1]) - int(E[j, 2 * a]) + 1) * sp[a]
            cen[j, a] = s1[a] / c                                         # int / int: correctly rounded
            for b in range(a, 3):
                cov[j, a, b] = cov[j, b, a] = float(Fraction(c * int(M[j, second[(a, b)]]) - s1[a] * s1[b], c * c)) * sp[a] * sp[b]
        w, v = np.linalg.eigh(cov[j])
        order = np.argsort(-w, kind="stable")
        plen[j] = 4.0 * np.sqrt(np.maximum(w[order], 0.0))
        axes = v[:, order].T
        for k in range(3):
            if axes[k, int(np.argmax(np.abs(axes[k])))] < 0.0:
                axes[k] = -axes[k]
        pax[j] = axes
    out.update(extent_mm=ext_mm, centroid_vox=cen, centroid_mm=cen * np.array(sp), covariance_mm2=cov, principal_lengths_mm=plen,
               principal_axes=pax)
    if faces is not None:
        Fc = np.asarray(faces).astype(np.int64).reshape(n, 6)
        out["surface_mm2"] = (Fc[:, 0].astype(np.float64) * (sp[1] * sp[2]) + Fc[:, 1].astype(np.float64) * (sp[0] * sp[2])
                              + Fc[:, 2].astype(np.float64) * (sp[0] * sp[1]))
        out["surface_mm2"][count == 0] = nan
        out["frame_faces"] = Fc[:, 3:6].copy()
        out["touches_frame"] = (Fc[:, 3:6] > 0).any(axis=1)
    if vrange is None:
        return out
    V = np.asarray(vrange).astype(np.int64).reshape(n, 2)
    mean, std, vmin, vmax = (np.full(n, nan) for _ in range(4))
    for j in range(n):
        c = int(count[j])
        if c == 0:
            continue
        sv, svv = int(M[j, 10]), int(M[j, 11])
        mean[j] = sv / c
        std[j] = math.sqrt(float(Fraction(c * svv - sv * sv, c * c)))
        vmin[j], vmax[j] = float(V[j, 0]), float(V[j, 1])
    out.update(mean=mean, std=std, min=vmin, max=vmax, clipped=M[:, 12:14].copy())
    if hist is None:
        return out
    Hh = np.asarray(hist).astype(np.int64).reshape(n, -1)
    qs = [float(q) for q in percentiles]
    assert all(0.0 <= q <= 100.0 for q in qs), "percentiles: 0 .. 100"
    pct, bounds = np.full((n, len(qs)), nan), np.full((n, len(qs), 2), nan)
    for j in range(n):
        c = int(count[j])
        if c == 0:
            continue
        cum = np.cumsum(Hh[j])
        for i, q in enumerate(qs):
            pos = (c - 1) * (q / 100.0)                                   # numpy's virtual index
            lo = int(math.floor(pos))
            hi = min(lo + 1, c - 1)
            t = pos - lo
            a, b = (_order_statistic(cum, int(M[j, 12]), int(hist_lo), k) for k in (lo, hi))
            bounds[j, i] = (a, b)
            pct[j, i] = a + (b - a) * t if t < 0.5 else b - (b - a) * (1.0 - t)   # numpy's linear interpolation, both of its branches
    out.update(percentiles=pct, percentile_bounds=bounds, hist=Hh, hist_lo=int(hist_lo))
    return out


@torch.no_grad()
def organ_measurements(labels: torch.Tensor, image: Optional[torch.Tensor] = None, obj_ids: Optional[Sequence[int]] = None,
                       spacing=(1.0, 1.0, 1.0), percentiles=(5, 25, 50, 75, 95), hist_range=None, n: Optional[int] = None) -> dict:
    """Per-organ measurements of the uint8 [T, H, W] label volume on the device and, with `image` (int16 Hounsfield units or uint8 grey, same
    shape and device), the intensity statistics inside every organ: one `ops.label_measure` call, one device-to-host copy of its small
    tables, then `measurements_from_tables` (keys and arithmetic: see there).  spacing = (sz, sy, sx) in millimetres.  hist_range = (lo, hi):
    the histogram behind the percentiles has one bin per integer in [lo, hi) (at most 65536); default (-1024, 3072) for int16, (0, 256) for
    uint8; values outside are counted in "clipped", and a percentile that falls among them is NaN.  obj_ids / n: as `clean_labels` takes
    them."""
    ids = _resolve_ids("organ_measurements", labels, obj_ids, n)
    lo = bins = 0
    if image is not None:
        assert image.dtype in DEFAULT_HIST_RANGE, "organ_measurements: the image must be int16 or uint8"
        lo, hi = (int(x) for x in (DEFAULT_HIST_RANGE[image.dtype] if hist_range is None else hist_range))
        assert 1 <= hi - lo <= ops.MEASURE_MAX_BINS, f"organ_measurements: hist_range [{lo}, {hi}) must hold 1 .. {ops.MEASURE_MAX_BINS} values"
        bins = hi - lo
    tables = ops.label_measure(labels, ids, image, lo, bins, faces=True)
    k = ids.numel()
    flat = torch.cat([t.reshape(-1).to(torch.int64) for t in tables if t is not None]).cpu().numpy()      # the one device-to-host copy
    sizes = [k * 14, k * 6, k * 2, k * 6, k * bins]
    m, e, v, f, h = (flat[sum(sizes[:i]): sum(sizes[:i + 1])] for i in range(5))
    if image is None:
        return measurements_from_tables(m, e, None, f, None, 0, spacing, percentiles)
    return measurements_from_tables(m, e, v, f, h.reshape(k, bins), lo, spacing, percentiles)


@torch.no_grad()
def organ_meshes(labels: torch.Tensor, obj_ids: Optional[Sequence[int]] = None, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0),
                 placement: str = "nets", relax: int = 0, n: Optional[int] = None, workspace_bytes: int = ops.MESH_WORKSPACE_BYTES) -> dict:
    """The surface of every organ of the uint8 [T, H, W] label volume as a closed quad mesh on the device (`ops.label_mesh`,
    csrc/mesh.hip) -> {obj_id: `meshes.OrganMesh`}: views of one vertex and one quad table, nothing copied to the host beyond the boxes and
    sizes on the way in.  spacing = (sz, sy, sx) and origin = (oz, oy, ox) in millimetres: voxel centre (z, y, x) sits at origin + (z sz,
    y sy, x sx).  placement="nets": surface nets, whose area is close to that of the smooth surface; "corner": the voxel faces themselves
    (the area `organ_measurements` reports, and exactly the organ's voxel volume).  relax: Jacobi sweeps that smooth the net while every
    vertex stays inside its cell (0 .. 64).  An organ without a voxel gives an empty mesh.  obj_ids / n: as `clean_labels` takes them."""
    from .meshes import OrganMesh
    ids = _resolve_ids("organ_meshes", labels, obj_ids, n)
    vertices, quads, v_offs, q_offs, _, values = ops.label_mesh_with_values(labels, ids, spacing, origin, placement, relax, workspace_bytes)
    return {v: OrganMesh(vertices[v_offs[j]: v_offs[j + 1]], quads[q_offs[j]: q_offs[j + 1]]) for j, v in enumerate(values)}


def mesh_measurements(meshes: dict) -> dict:
    """{obj_id: OrganMesh} of `organ_meshes` (spacing in millimetres) -> "ids", "area_mm2", "volume_mm3", "volume_ml" (float64 arrays in the
    dict's order), "vertices" and "quads" (counts): the surface area and the enclosed volume of the mesh, beside `organ_measurements`'
    voxel-face area and voxel volume (which stay as they are).  One scalar per figure and organ crosses to the host."""
    ids = list(meshes)
    area = np.array([meshes[v].area() for v in ids], dtype=np.float64)
    vol = np.array([meshes[v].volume() for v in ids], dtype=np.float64)
    return {"ids": ids, "area_mm2": area, "volume_mm3": vol, "volume_ml": vol / 1000.0,
            "vertices": np.array([meshes[v].vertices.shape[0] for v in ids], dtype=np.int64),
            "quads": np.array([meshes[v].quads.shape[0] for v in ids], dtype=np.int64)}


def measurement_errors(pred_m: dict, gt_m: dict) -> dict:
    """Two reports of `organ_measurements` / `measurements_from_tables` on the same organs -> "volume_rel_diff" = (Vp - Vg) / Vg per organ
    (signed; NaN where the organ is absent from the ground truth) and "centroid_distance_mm" (NaN where it is absent from either): the
    figures usually reported beside Dice, with no further device work."""
    vp, vg = (np.asarray(m["volume_mm3"], dtype=np.float64) for m in (pred_m, gt_m))
    assert vp.shape == vg.shape, "measurement_errors: the two reports must list the same organs"
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(vg > 0.0, (vp - vg) / vg, np.nan)
    d = np.asarray(pred_m["centroid_mm"], dtype=np.float64) - np.asarray(gt_m["centroid_mm"], dtype=np.float64)
    return {"volume_rel_diff": rel, "centroid_distance_mm": np.sqrt((d * d).sum(axis=1))}


# ---- confidence without a ground truth: margins, core / envelope volumes, per-slice tables -----------------------------------
DEFAULT_PROBABILITIES = (0.6, 0.75, 0.9)
CONFIDENCE_MAPS = ops.CONFIDENCE_OUTPUTS


def margins_from_probabilities(ps) -> tuple:
    """Winning probabilities in (0.5, 1) -> margins in logit units, log(p / (1 - p)) rounded to fp32 (as the device compares with them): at
    label_thr = 0 the band "margin < logit(p)" holds the voxels whose decision had a sigmoid probability below p."""
    out = []
    for p in ps:
        p = float(p)
        if not 0.5 < p < 1.0:
            raise ValueError(f"margins_from_probabilities: p = {p} (a winning probability: 0.5 < p < 1)")
        out.append(float(np.float32(math.log(p / (1.0 - p)))))
    return tuple(out)


@torch.no_grad()
def volume_confidence(masks: Union[Dict[int, torch.Tensor], torch.Tensor], H: int, W: int, obj_ids: Optional[Sequence[int]] = None,
                      probabilities=DEFAULT_PROBABILITIES, margins=None, select: int = 1, label_thr: float = 0.0, slices_per_call: int = 8,
                      maps=CONFIDENCE_MAPS) -> dict:
    """`label_volume` without a ground truth: masks and obj_ids as it takes them.  margins: K <= 8 ascending positive logit distances (default:
    `margins_from_probabilities(probabilities)`); select: the band of the core / envelope volumes.  Returns {"labels", "core", "envelope",
    "conf": uint8 [T, H, W] for each name in `maps`; "counts": int32 [T, n, 2 + 2K]; "margins": the K floats} with every tensor on the device
    (`ops.label_confidence` documents volumes and columns).  The slices go through `slices_per_call` at a time; nothing is copied to the host."""
    order, T, n, dev = _masks_layout(masks)
    H, W = int(H), int(W)
    ids = ops.label_ids(list(range(1, n + 1)) if obj_ids is None else obj_ids, dev)
    assert ids.numel() == n, f"{n} objects need {n} ids"
    m = margins_from_probabilities(probabilities) if margins is None else tuple(float(np.float32(v)) for v in margins)
    maps = tuple(maps)
    assert all(name in CONFIDENCE_MAPS for name in maps), f"maps: any of {CONFIDENCE_MAPS}"
    out = {name: torch.empty(T, H, W, dtype=torch.uint8, device=dev) for name in CONFIDENCE_MAPS if name in maps}
    out["counts"] = torch.empty(T, n, 2 + 2 * len(m), dtype=torch.int32, device=dev)
    step = max(1, int(slices_per_call))
    for i in range(0, T, step):
        j = min(T, i + step)
        ops.label_confidence(_chunk(masks, order, i, j), ids, H, W, m, select, label_thr, counts=out["counts"][i:j],
                             **{name: out[name][i:j] if name in out else False for name in CONFIDENCE_MAPS})
    out["margins"] = m
    return out


@torch.no_grad()
def slice_consistency(labels: torch.Tensor, obj_ids) -> torch.Tensor:
    """int32 [D - 1, n, 3] on the device = (|A & B|, |A|, |B|) per object between every slice A of the uint8 [D, H, W] label volume and the next
    slice B: `ops.label_overlap` on the volume without its last and without its first slice (both contiguous views; D >= 2)."""
    assert labels.dim() == 3 and labels.shape[0] >= 2, "slice_consistency: a label volume of at least two slices"
    return ops.label_overlap(labels[:-1], labels[1:], obj_ids)


def _host_int64(*tables):
    """tensors (one concatenated device-to-host copy) or arrays -> int64 numpy arrays of the same shapes"""
    if any(isinstance(t, torch.Tensor) for t in tables):
        assert all(isinstance(t, torch.Tensor) for t in tables), "tensors or arrays, not both"
        flat = torch.cat([t.reshape(-1).to(torch.int64) for t in tables]).cpu().numpy()
        out, at = [], 0
        for t in tables:
            out.append(flat[at: at + t.numel()].reshape(tuple(t.shape)))
            at += t.numel()
        return out
    return [np.asarray(t).astype(np.int64) for t in tables]


def _confidence_figures(k: np.ndarray, K: int, ml_per_voxel: float) -> dict:
    """k int64 [..., n, 2 + 2K] -> the figures of `confidence_report` with the same leading axes"""
    label, inside, outside = k[..., 0], k[..., 2: 2 + K], k[..., 2 + K: 2 + 2 * K]
    core, env = label[..., None] - inside, label[..., None] + outside
    uncertain = inside + outside
    with np.errstate(divide="ignore", invalid="ignore"):
        fraction = np.where(env > 0, uncertain.astype(np.float64) / env.astype(np.float64), np.nan)
    return {"voxels": label, "volume_ml": label * ml_per_voxel, "core_voxels": core, "core_ml": core * ml_per_voxel, "envelope_voxels": env,
            "envelope_ml": env * ml_per_voxel, "uncertain_voxels": uncertain, "uncertain_fraction": fraction, "overlap_voxels": k[..., 1]}


def confidence_report(counts, consistency=None, spacing=(1.0, 1.0, 1.0)) -> dict:
    """The host half of `volume_confidence`: counts [T, n, 2 + 2K] and, optionally, `slice_consistency`'s table [T - 1, n, 3] (device tensors:
    the call's one device-to-host copy; or numpy arrays), spacing (sz, sy, sx) in millimetres.  Per organ o and band k, from int64 sums over the
    slices: "voxels", "volume_ml" [n] of the label; "core_voxels", "core_ml" [n, K] (label minus the labelled voxels with a margin below
    margins[k]); "envelope_voxels", "envelope_ml" [n, K] (label plus the background voxels that near to o) -- the volume interval of band k;
    "uncertain_voxels" [n, K] and "uncertain_fraction" = uncertain / envelope (NaN where the envelope is empty); "overlap_voxels" [n]: above the
    label threshold but labelled another organ.  "per_slice": the same keys with a leading slice axis.  With consistency: "slice_dice"
    float64 [T - 1, n] = 2 |A & B| / (|A| + |B|) of adjacent slices, NaN where both are empty.  Integers up to the final division."""
    tables = _host_int64(counts) if consistency is None else _host_int64(counts, consistency)
    k = tables[0]
    assert k.ndim == 3 and k.shape[-1] >= 4 and k.shape[-1] % 2 == 0, "counts: [T, n, 2 + 2K]"
    K = (k.shape[-1] - 2) // 2
    sp = tuple(float(s) for s in spacing)
    assert len(sp) == 3 and all(s > 0.0 for s in sp), "spacing: three positive values (sz, sy, sx)"
    ml = sp[0] * sp[1] * sp[2] / 1000.0
    out = _confidence_figures(k.sum(axis=0), K, ml)
    out["per_slice"] = _confidence_figures(k, K, ml)
    if consistency is not None:
        c = tables[1]
        assert c.ndim == 3 and c.shape[-1] == 3 and c.shape[1] == k.shape[1], "consistency: [T - 1, n, 3]"
        den = c[..., 1] + c[..., 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            out["slice_dice"] = np.where(den > 0, 2.0 * c[..., 0].astype(np.float64) / den.astype(np.float64), np.nan)
    return out
