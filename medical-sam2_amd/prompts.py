"""Start of the 3-D path: the box and click prompts that `volume.segment_volume`, `data.validate_volume` and
`training_3d.train_step_3d` consume, taken from a uint8 label volume on the device.

The reference's dataset (`func_3d/dataset/btcv.py:88-104`, here `data.BTCVVolumes.__getitem__`) builds them per (slice, object) pair on
the host: `generate_bbox` / `random_click` (`func_3d/utils.py:89-137`) run `np.argwhere(mask == max)` over a full-resolution mask for every
pair.  Here `ops.label_stats` (csrc/prompts.hip) reads the label volume of `volume_labels.labels_from_pack` once and returns, per pair,
the voxel count and the inclusive row / column extent -- the box --, and `ops.label_pick` the k-th voxel of the object in raster order,
which is `np.argwhere`'s order -- the click.  All results are integers; one small table per volume crosses to the host, and only where a
caller wants host dictionaries.

* `label_prompts`: device tensors for all slices and objects, no host sync.
* `prompts_pack`: the dictionaries `BTCVVolumes.__getitem__` puts under "bbox", or under "pt" / "p_label".
* `segment_prompts`: the `{slice: {...}}` prompts of `segment_volume` / `train_step_3d`; `targets_from_labels`: the latter's targets.
* `corrective_clicks`: the next click per (slice, object) from the error regions of a prediction against the ground truth
  (`ops.label_error_clicks`, csrc/clicks.hip); `worst_slices`: where an object's error is largest.  `interactive.refine_volume` drives them.
* `review_slices`: `worst_slices` on the uncertain-voxel columns of `volume_labels.volume_confidence` -- no ground truth
  (`interactive.review_queue`).

Not reproduced: what `random_click` does with an empty mask (label 0 at a random background pixel: the dataset never calls it for an
absent object, and `present` tells the caller), and overlapping object masks (a label volume has one value per voxel;
`labels_from_pack` documents which mask wins).

The same entries serve the 2-D path: a `[B, H, W]` uint8 batch of binary masks with `obj_ids=[1]` gives one box or one click per image."""
from __future__ import annotations

import random
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import ops

F32 = torch.float32


@torch.no_grad()
def _tables(labels: torch.Tensor, ids: torch.Tensor, slices_per_call: int, k: Optional[torch.Tensor] = None, u: Optional[torch.Tensor] = None):
    """(stats int32 [D, n, 5], xy int32 [D, n, 2] | None) of the whole volume, `slices_per_call` slices at a time: the per-row workspace
    is [slices_per_call, n, H] however many slices there are."""
    D, H, _ = labels.shape
    n, dev = ids.numel(), labels.device
    step = max(1, min(int(slices_per_call), D))
    rows = torch.empty(step, n, H, dtype=torch.int32, device=dev)
    stats = torch.empty(D, n, 5, dtype=torch.int32, device=dev)
    pick = k is not None or u is not None
    xy = torch.empty(D, n, 2, dtype=torch.int32, device=dev) if pick else None
    for i in range(0, D, step):
        j = min(D, i + step)
        s, r = ops.label_stats(labels[i:j], ids, rows=rows[: j - i])
        stats[i:j] = s
        if pick:
            xy[i:j] = ops.label_pick(labels[i:j], ids, s, r, k=None if k is None else k[i:j], u=None if u is None else u[i:j])
    return stats, xy


def _volume(labels: torch.Tensor) -> torch.Tensor:
    assert isinstance(labels, torch.Tensor) and labels.dtype == torch.uint8 and labels.dim() == 3, "labels: uint8 [D, H, W] label volume"
    return labels.contiguous()


@torch.no_grad()
def label_prompts(labels: torch.Tensor, obj_ids: Sequence[int], prompt: str = "bbox", u: Optional[torch.Tensor] = None,
                  k: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None, slices_per_call: int = 8):
    """labels: uint8 [D, H, W] on the GPU; obj_ids: the label value of each of the n objects (distinct, 1 .. 255).
    prompt="bbox": returns (boxes, present): boxes float32 [D, n, 4] = (x0, y0, x1, y1) = (c0, r0, c1, r1), inclusive, the order
    `data.generate_bbox` returns and `volume.box_point_inputs` takes; -1 where the object is absent.
    prompt="click": returns (points, point_labels, present): points float32 [D, n, 1, 2] = (x, y) of the k-th voxel of the object in
    raster order, point_labels int32 [D, n, 1] = 1 (-1, with the point at (-1, -1), where the object is absent).  k int32 [D, n]
    selects the voxels; or u uint32 [D, n] uniform random words (k = (u * count) >> 32); without either the words are drawn on the
    device with `generator`.
    present: bool [D, n].  Everything stays on the device, and nothing waits for it."""
    if prompt not in ("bbox", "click"):
        raise ValueError("Prompt not recognized")
    labels = _volume(labels)
    dev = labels.device
    ids = ops.label_ids(obj_ids, dev)
    D, n = labels.shape[0], ids.numel()
    if prompt == "bbox":
        stats, _ = _tables(labels, ids, slices_per_call)
        return stats[..., [3, 1, 4, 2]].to(F32), stats[..., 0] > 0
    assert k is None or u is None, "either k or u"
    if k is None and u is None:                              # 32 uniform bits per pair, held as int32 (ops.label_pick reads the bits)
        u = torch.randint(-2 ** 31, 2 ** 31, (D, n), dtype=torch.int64, device=dev, generator=generator).to(torch.int32)
    stats, xy = _tables(labels, ids, slices_per_call, k=None if k is None else k.to(device=dev, dtype=torch.int32).contiguous(),
                        u=None if u is None else u.to(dev).contiguous())
    present = stats[..., 0] > 0
    point_labels = torch.where(present, 1, -1).to(torch.int32).unsqueeze(-1)
    return xy.to(F32).unsqueeze(2), point_labels, present


@torch.no_grad()
def corrective_clicks(pred: torch.Tensor, gt: torch.Tensor, obj_ids: Sequence[int], mode: str = "center", u: Optional[torch.Tensor] = None,
                      k: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None, slices_per_call: int = 8):
    """The next click of an interactive round, per (slice, object): pred and gt are uint8 [D, H, W] label volumes on the GPU (a prediction of
    `volume_labels.label_volume` and the ground truth), obj_ids the label values.  Returns (points float32 [D, n, 1, 2] = (x, y),
    point_labels int32 [D, n, 1], errors int32 [D, n, 2] = (|FN|, |FP|)) on the device (`ops.label_error_clicks`, csrc/clicks.hip).
    mode="center": the voxel farthest from the border of the larger of the object's two error regions on that slice -- missed voxels (FN:
    label 1) or voxels claimed wrongly (FP: label 0); SAM 2's `sample_one_point_from_error_center`.  mode="uniform": a voxel drawn uniformly
    from FN | FP, labelled by the region it lies in (`sample_random_points_from_errors`): k int32 [D, n] selects the voxel in raster order,
    or u uint32 [D, n] uniform words (k = (u * count) >> 32); without either the words are drawn on the device with `generator`
    (a generator of the volumes' device, or None for the default one).
    A pair without an error voxel gives label -1 at (-1, -1), `label_prompts`' absent convention (SAM 2 returns a negative click at (0, 0)).
    The volume goes through `slices_per_call` slices at a time (the workspace is one chunk's; every slice is on its own, so the results do not
    depend on the chunking); nothing is copied to the host."""
    if mode not in ops.CLICK_MODES:
        raise ValueError("Mode not recognized")
    pred, gt = _volume(pred), _volume(gt)
    assert pred.shape == gt.shape and pred.device == gt.device, "pred and gt: label volumes of one shape on one device"
    dev = pred.device
    ids = ops.label_ids(obj_ids, dev)
    (D, H, W), n = pred.shape, ids.numel()
    if mode == "uniform":
        assert k is None or u is None, "either k or u"
        if k is None and u is None:                          # 32 uniform bits per pair, held as int32 (the kernel reads the bits)
            assert generator is None or generator.device.type == dev.type, f"generator on {generator.device}: the words are drawn on {dev}"
            u = torch.randint(-2 ** 31, 2 ** 31, (D, n), dtype=torch.int64, device=dev, generator=generator).to(torch.int32)
        k = None if k is None else k.to(device=dev, dtype=torch.int32).contiguous()
        u = None if u is None else u.to(dev).contiguous()
    else:
        assert k is None and u is None, "k and u belong to mode='uniform'"
    step = max(1, min(int(slices_per_call), D))
    ws = ops._workspace8(ops.label_error_clicks_workspace_bytes(step, H, W, n, mode), dev)
    table = torch.empty(D, n, 8, dtype=torch.int32, device=dev)
    for i in range(0, D, step):
        j = min(D, i + step)
        ops.label_error_clicks(pred[i:j], gt[i:j], ids, mode, k=None if k is None else k[i:j], u=None if u is None else u[i:j], workspace=ws,
                               out=table[i:j])
    return table[..., :2].to(F32).unsqueeze(2), table[..., 2:3].contiguous(), table[..., 3:5].contiguous()


def worst_slices(errors: torch.Tensor, per_object: int = 1) -> torch.Tensor:
    """errors: int [D, n, 2] = (|FN|, |FP|) per slice and object (`corrective_clicks`) -> int64 [n, per_object]: per object the slices with
    the most error voxels |FN| + |FP|, most first, ties to the lower slice; -1 where fewer than per_object slices of the object have an
    error voxel (a slice without one is never named).  One composite integer key per (slice, object), total * D + (D - 1 - slice), ranks
    them, so the order is defined; torch ops on errors' device only."""
    assert errors.dim() == 3 and errors.shape[-1] == 2 and not errors.is_floating_point(), "errors: int [D, n, 2]"
    per_object = int(per_object)
    assert per_object >= 1, "per_object >= 1"
    D, n, _ = errors.shape
    total = errors.to(torch.int64).sum(-1)                                              # [D, n]
    down = torch.arange(D - 1, -1, -1, dtype=torch.int64, device=errors.device)         # D - 1 - slice
    key = total * D + down[:, None]
    top = torch.topk(key, min(per_object, D), dim=0).values                            # keys are distinct per object
    out = torch.full((per_object, n), -1, dtype=torch.int64, device=errors.device)
    out[: top.shape[0]] = torch.where(top >= D, D - 1 - top % D, torch.full_like(top, -1))   # total >= 1 iff key >= D
    return out.t().contiguous()


def review_slices(counts: torch.Tensor, band: int, per_object: int = 1) -> torch.Tensor:
    """`worst_slices` without a ground truth: counts int [D, n, 2 + 2K] of `volume_labels.volume_confidence` -> int64 [n, per_object]: per
    object the slices with the most uncertain voxels of band `band` (labelled it with a margin below margins[band], plus background that
    nears it within margins[band]), most first, ties to the lower slice, -1 where fewer slices have one: `worst_slices` on those two columns."""
    assert counts.dim() == 3 and counts.shape[-1] >= 4 and counts.shape[-1] % 2 == 0 and not counts.is_floating_point(), "counts: int [D, n, 2 + 2K]"
    K, band = (counts.shape[-1] - 2) // 2, int(band)
    assert 0 <= band < K, f"band {band} of 0 .. {K - 1}"
    return worst_slices(torch.stack([counts[..., 2 + band], counts[..., 2 + K + band]], dim=-1), per_object)


def _jitter(r0, r1, c0, c1, variation: float, seed: Optional[int]) -> np.ndarray:
    """data.generate_bbox from the extents on: its arithmetic on the numbers np.argwhere's min / max give it (numpy int64)"""
    r0, r1, c0, c1 = (np.int64(v) for v in (r0, r1, c0, c1))
    if variation > 0:
        rng = np.random.RandomState(seed)
        dw, dh = rng.randn(2) * variation
        mr, mc, h, w = (r0 + r1) / 2, (c0 + c1) / 2, (r1 - r0) * (1 + dw), (c1 - c0) * (1 + dh)
        r0, r1, c0, c1 = mr - h / 2, mr + h / 2, mc - w / 2, mc + w / 2
    return np.array([c0, r0, c1, r1])


@torch.no_grad()
def prompts_pack(labels: torch.Tensor, obj_list: Sequence[int], prompt: str = "bbox", prompt_freq: int = 1, seed: Optional[int] = None,
                 variation: float = 0, slices_per_call: int = 8):
    """The prompt dictionaries of `data.BTCVVolumes.__getitem__` for every `prompt_freq`-th slice of a label volume (1: every slice, as
    the dataset): prompt="bbox" returns bbox = {frame: {obj: float32 [4]}}; prompt="click" returns (pt, p_label) = ({frame: {obj: float32
    [1, 2]}}, {frame: {obj: int32 [1]}}); present objects only, same dtypes and shapes.  Boxes come from one device-to-host copy of the
    stats table; `variation` > 0 jitters them on the host with `data.generate_bbox`'s arithmetic and its RandomState(seed).  Clicks: the
    host draws k = Random(seed).randint(0, count - 1) per pair, exactly as `data.random_click` does (the `random` module's stream
    without a seed), one k table goes up and one xy table comes back; the per-row workspace covers the whole volume here."""
    if prompt not in ("bbox", "click"):
        raise ValueError("Prompt not recognized")
    labels = _volume(labels)
    ids = ops.label_ids(obj_list, labels.device)
    D, n = labels.shape[0], ids.numel()
    frames = range(0, D, max(1, int(prompt_freq)))
    if prompt == "bbox":
        st = _tables(labels, ids, slices_per_call)[0].cpu().numpy()
        return {f: {o: torch.tensor(_jitter(*st[f, j, 1:], variation, seed), dtype=F32) for j, o in enumerate(obj_list) if st[f, j, 0] > 0}
                for f in frames}
    stats, rows = ops.label_stats(labels, ids)
    st = stats.cpu().numpy()
    k = np.zeros((D, n), dtype=np.int32)
    for f in frames:
        for j in range(n):
            if st[f, j, 0] > 0:
                rnd = random.Random(seed) if seed is not None else random
                k[f, j] = rnd.randint(0, int(st[f, j, 0]) - 1)
    xy = ops.label_pick(labels, ids, stats, rows, k=torch.from_numpy(k).to(labels.device)).cpu().numpy()
    pt = {f: {o: torch.tensor(xy[f, j].astype(np.int64)[None], dtype=F32) for j, o in enumerate(obj_list) if st[f, j, 0] > 0} for f in frames}
    p_label = {f: {o: torch.tensor([1], dtype=torch.int32) for o in pt[f]} for f in frames}
    return pt, p_label


@torch.no_grad()
def segment_prompts(labels: torch.Tensor, obj_list: Sequence[int], prompt: str = "bbox", prompt_freq: int = 2, u: Optional[torch.Tensor] = None,
                    k: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None, slices_per_call: int = 8) -> Dict[int, dict]:
    """The prompts of `volume.segment_volume` / `training_3d.train_step_3d` for the conditioning slices 0, prompt_freq, 2 prompt_freq ..:
    {slice: {"boxes": [n, 4]}} or {slice: {"point_coords": [n, 1, 2], "point_labels": [n, 1]}}, views of `label_prompts`' device tables.
    Those callers need the same n objects on every conditioning slice: raises ValueError naming the first (slice, object) pair that is
    absent on one (the one host copy of this call: the [D, n] presence table)."""
    out = label_prompts(labels, obj_list, prompt, u=u, k=k, generator=generator, slices_per_call=slices_per_call)
    cond = list(range(0, labels.shape[0], max(1, int(prompt_freq))))
    present = out[-1].cpu()
    for t in cond:
        for j, o in enumerate(obj_list):
            if not bool(present[t, j]):
                raise ValueError(f"object {int(o)} is absent on conditioning slice {t}: every conditioning slice needs all {len(obj_list)} objects")
    if prompt == "bbox":
        return {t: {"boxes": out[0][t]} for t in cond}
    return {t: {"point_coords": out[0][t], "point_labels": out[1][t]} for t in cond}


@torch.no_grad()
def targets_from_labels(labels: torch.Tensor, obj_list: Sequence[int]) -> Dict[int, torch.Tensor]:
    """{slice: float32 [n, 1, S, S] in {0, 1}}: the targets of `train_step_3d` for every slice of a label volume."""
    labels = _volume(labels)
    ids = ops.label_ids(obj_list, labels.device).view(-1, 1, 1, 1)
    return {t: (labels[t][None, None] == ids).to(F32) for t in range(labels.shape[0])}
