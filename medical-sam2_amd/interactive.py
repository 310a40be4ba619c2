"""The interactive loop on a volume: "Dice after k clicks".  Every round propagates, scores the label volume against the ground truth, puts
one corrective click per object at the centre of its largest error and propagates again -- SAM-style interactive evaluation, with the clicks
SAM 2's training samples from error regions (`sample_one_point_from_error_center`, `sample_random_points_from_errors`).

The predictor implements its half already: `add_new_points(..., clear_old_points=False)` on a tracked slice feeds the previous logits back
together with the new click, and the next `propagate_in_video` re-tracks the unprompted slices.  This module supplies the other half on the
device: `volume_labels.label_volume` turns the stored low-res logits into a label volume, `ops.label_overlap` counts, `prompts.corrective_clicks`
(csrc/clicks.hip) finds the click of every (slice, object) and `prompts.worst_slices` the slices to correct.  Per round one small table
crosses to the host: the overlap counts and the chosen click rows, in one copy.

Without a ground truth `review_queue` takes the place of `refine_volume`'s scoring half: `volume_labels.volume_confidence` turns the same stored
logits into the label volume, a confident core and a generous envelope, `prompts.review_slices` names each object's most uncertain slices and
`corrective_clicks(core, envelope)` the centre of the largest uncertain part of each -- where a reader should look first; one copy to the host.

Not built: clicks merged into `segment_volume`'s or `train_step_3d`'s prompt dictionaries, and the image predictor's loop."""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from . import ops
from .prompts import corrective_clicks, review_slices, worst_slices
from .volume_labels import (DEFAULT_PROBABILITIES, confidence_report, label_volume, margins_from_probabilities, slice_consistency,
                            volume_confidence, volume_scores)


def _propagate(predictor, state) -> None:
    """forward from the first conditioning slice; when that is not slice 0, also in reverse from it"""
    for _ in predictor.propagate_in_video(state):
        pass
    first = min(state["output_dict"]["cond_frame_outputs"])
    if first > 0:
        for _ in predictor.propagate_in_video(state, start_frame_idx=first, reverse=True):
            pass


def _stored_logits(state) -> dict:
    """{slice: low-res logits [n, 1, h, w]} of every slice of a propagated state, on the state's compute device"""
    od = state["output_dict"]
    out = {}
    for t in range(state["num_frames"]):
        cur = od["cond_frame_outputs"].get(t) or od["non_cond_frame_outputs"].get(t)
        assert cur is not None, f"slice {t} has not been tracked"
        out[t] = cur["pred_masks"].to(state["device"])
    return out


@torch.no_grad()
def refine_volume(predictor, state, gt: torch.Tensor, obj_ids: Sequence[int], rounds: int = 3, clicks_per_round: int = 1, mode: str = "center",
                  generator: Optional[torch.Generator] = None, label_thr: float = 0.0, keep_labels: bool = False) -> List[dict]:
    """predictor: a `SAM2VideoPredictor`; state: its inference state with the caller's first prompts for every object, the object ids being
    the label values `obj_ids` (in the state's order); gt: uint8 [T, video_height, video_width] label volume on the device.
    Round: propagate; label volume of the stored low-res logits at video resolution (`label_thr`: see `label_volume`); counts against gt;
    per object the click (`corrective_clicks`, `mode`, `generator` for mode="uniform") on each of its `clicks_per_round` worst slices
    (`worst_slices`), added with `add_new_points(state, slice, obj_id, [[x, y]], [label], clear_old_points=False)`.  After `rounds`
    correction rounds one more propagation is scored; the loop ends earlier once no object has an error voxel.
    Returns one record per propagation: {"counts": int32 [T, n, 3] = (|P & G|, |P|, |G|) on the device, "volume_dice": float64 [n]
    (`volume_scores`' arithmetic), "clicks": [(obj_id, slice, x, y, label)] added after it, "labels": the label volume if keep_labels}."""
    obj_ids = [int(o) for o in obj_ids]
    assert [int(o) for o in state["obj_ids"]] == obj_ids, f"the state's objects {state['obj_ids']} must be the label values {obj_ids}, in this order"
    T, H, W = state["num_frames"], state["video_height"], state["video_width"]
    assert gt.dtype == torch.uint8 and tuple(gt.shape) == (T, H, W) and gt.is_cuda, f"gt: uint8 [{T}, {H}, {W}] label volume on the GPU"
    gt = gt.contiguous()
    ids = ops.label_ids(obj_ids, gt.device)
    n, per = len(obj_ids), int(clicks_per_round)
    obj = torch.arange(n, device=gt.device)[:, None]
    records = []
    for r in range(int(rounds) + 1):
        _propagate(predictor, state)
        labels = label_volume(_stored_logits(state), H, W, obj_ids, label_thr=label_thr)
        counts = ops.label_overlap(labels, gt, ids)
        parts = [counts.reshape(-1).to(torch.int64)]
        if r < rounds:
            points, point_labels, errors = corrective_clicks(labels, gt, obj_ids, mode, generator=generator)
            where = worst_slices(errors, per)                                           # [n, per], -1 = no such slice
            at = where.clamp(min=0)
            xy = points[at, obj, 0].to(torch.int64)                                     # [n, per, 2]
            chosen = torch.cat([where[..., None], xy, point_labels[at, obj].to(torch.int64)], dim=-1)
            parts.append(chosen.reshape(-1))
        host = torch.cat(parts).cpu().numpy()                                           # the round's one device-to-host copy
        k = host[: T * n * 3].reshape(1, T, n, 3)
        record = {"counts": counts, "volume_dice": volume_scores(k)["volume_dice"][0], "clicks": []}
        if keep_labels:
            record["labels"] = labels
        records.append(record)
        if r == rounds:
            break
        for j, rows in enumerate(host[T * n * 3:].reshape(n, per, 4).tolist()):
            for t, x, y, label in rows:
                if t >= 0:                                                              # (a named slice has an error voxel: its label is 0 or 1)
                    record["clicks"].append((obj_ids[j], t, x, y, label))
        if not record["clicks"]:
            break
        for o, t, x, y, label in record["clicks"]:
            predictor.add_new_points(state, t, o, [[float(x), float(y)]], [label], clear_old_points=False)
    return records


@torch.no_grad()
def review_queue(state, obj_ids: Sequence[int], probabilities=DEFAULT_PROBABILITIES, select: int = 1, per_object: int = 1,
                 label_thr: float = 0.0):
    """state: a propagated inference state (only its stored low-res logits are read: no predictor, no ground truth); obj_ids: the label values
    of its objects, in the state's order.  `volume_confidence` at video resolution with the margins of `probabilities` gives labels, core and
    envelope of band `select`; per object its `per_object` slices with the most uncertain voxels of that band (`review_slices`) and on each the
    point `corrective_clicks(core, envelope, mode="center")` gives: the voxels of the envelope that the core misses ARE the uncertain band, so
    it is the voxel deepest inside its largest part.  Returns (report, queue): report = `confidence_report` (with "slice_dice" when the volume has
    two slices or more, plus "margins"), queue = [(obj_id, slice, x, y, uncertain_voxels)], objects in order, most uncertain slice first; an object
    with fewer uncertain slices has fewer rows.  One device-to-host copy."""
    obj_ids = [int(o) for o in obj_ids]
    T, H, W = state["num_frames"], state["video_height"], state["video_width"]
    n, per = len(obj_ids), int(per_object)
    margins = margins_from_probabilities(probabilities)
    conf = volume_confidence(_stored_logits(state), H, W, obj_ids, margins=margins, select=select, label_thr=label_thr,
                             maps=("labels", "core", "envelope"))
    counts = conf["counts"]
    dev, K = counts.device, len(margins)
    parts = [counts]
    if T > 1:
        parts.append(slice_consistency(conf["labels"], obj_ids))
    points, _, _ = corrective_clicks(conf["core"], conf["envelope"], obj_ids, "center")
    where = review_slices(counts, select, per)                                          # [n, per], -1 = no such slice
    at = where.clamp(min=0)
    obj = torch.arange(n, device=dev)[:, None]
    xy = points[at, obj, 0].to(torch.int64)                                             # [n, per, 2]
    uncertain = (counts[..., 2 + select] + counts[..., 2 + K + select]).to(torch.int64)[at, obj]
    parts.append(torch.cat([where[..., None], xy, uncertain[..., None]], dim=-1))
    host = torch.cat([p.reshape(-1).to(torch.int64) for p in parts]).cpu().numpy()      # the call's one device-to-host copy
    sizes = [p.numel() for p in parts]
    k = host[: sizes[0]].reshape(tuple(counts.shape))
    c = host[sizes[0]: sizes[0] + sizes[1]].reshape(T - 1, n, 3) if T > 1 else None
    report = confidence_report(k, c)
    report["margins"] = margins
    queue = []
    for j, rows in enumerate(host[len(host) - sizes[-1]:].reshape(n, per, 4).tolist()):
        queue.extend((obj_ids[j], t, x, y, u) for t, x, y, u in rows if t >= 0)
    return report, queue
