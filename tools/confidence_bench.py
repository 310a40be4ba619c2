#!/usr/bin/env python3
"""Label confidence from low-res logits: fp32 logits of 13 organs at 256^2, 8 slices to 512^2 and 64 slices to 1024^2, one call each.

- `ops.label_confidence` with labels only, with each map added (core, envelope, conf), with every map and the counts, and the counts alone;
  the last once more on white-noise logits, where a wave holds every object (the worst case of the walk over a wave's distinct objects);
- `ops.label_slices` for the labels alone on the same inputs: the kernel this one was shaped after;
- the torch composition of all five outputs: `ops.bilinear_upsample`, `topk(2)` over the objects, comparisons, per-slice sums.

HIP events around `reps` back-to-back calls, the median of `rounds` such windows, the arms taking turns.  Prints one line per figure and a
JSON line at the end; asserts nothing about time."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import medical_sam2_amd.ops as ops  # noqa: E402
from medical_sam2_amd.volume_labels import margins_from_probabilities  # noqa: E402

N, LOW = 13, 256
CASES = ((8, 512), (64, 1024))
SELECT = 1


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def medians(fns, reps, rounds=7, warm=2):
    """seconds per call of each fn: median over `rounds` windows, the arms taking turns"""
    for f in fns:
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for i, f in enumerate(fns):
            ts[i].append(window(f, reps))
    return [float(np.median(t)) for t in ts]


def composed(x, ids, H, W, margins, select):
    """labels, core, envelope, conf, counts with torch ops on the up-sampled logits (label_thr 0)"""
    T, n = x.shape[:2]
    up = ops.bilinear_upsample(x.view(T * n, *x.shape[2:]), H, W).view(T, n, H, W)
    top = up.topk(2, dim=1)
    tv, sv, to = top.values[:, 0], top.values[:, 1], top.indices[:, 0]
    lab = tv > 0
    m = torch.where(lab, tv - sv.clamp(min=0), -tv)
    mk = torch.tensor(margins, dtype=torch.float32, device=x.device)
    id_to, zero = ids[to], torch.zeros((), dtype=torch.uint8, device=x.device)
    labels = torch.where(lab, id_to, zero)
    core = torch.where(lab & (m >= mk[select]), id_to, zero)
    envelope = torch.where(lab | (m < mk[select]), id_to, zero)
    below = m[:, None] < mk[None, :, None, None]                                            # [T, K, H, W]
    conf = (len(margins) - below.sum(1)).to(torch.uint8)
    K = len(margins)
    counts = torch.empty(T, n, 2 + 2 * K, dtype=torch.int32, device=x.device)
    for o in range(n):
        mine = to == o
        inside, outside = mine & lab, mine & ~lab
        counts[:, o, 0] = inside.sum((-1, -2))
        counts[:, o, 1] = (up[:, o] > 0).sum((-1, -2)) - counts[:, o, 0]
        counts[:, o, 2: 2 + K] = (inside[:, None] & below).sum((-1, -2))
        counts[:, o, 2 + K:] = (outside[:, None] & below).sum((-1, -2))
    return labels, core, envelope, conf, counts


def main():
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    margins = margins_from_probabilities((0.6, 0.75, 0.9))
    res = {"objects": N, "low": LOW, "margins": margins, "select": SELECT, "cases": []}
    for T, S in CASES:
        g = torch.Generator().manual_seed(T)
        smooth = torch.nn.functional.interpolate(torch.randn(T, N, 32, 32, generator=g), size=(LOW, LOW), mode="bilinear", align_corners=False)
        x = (smooth * 6 - 2).to(dev).contiguous()                 # organ-like blobs: most voxels background, every object somewhere
        noise = (torch.randn(T, N, LOW, LOW, generator=g) * 4).to(dev).contiguous()
        ids = ops.label_ids(list(range(1, N + 1)), dev)
        vols = [torch.empty(T, S, S, dtype=torch.uint8, device=dev) for _ in range(4)]
        counts = torch.empty(T, N, 2 + 2 * len(margins), dtype=torch.int32, device=dev)
        off = [False] * 4

        def conf_arm(k, with_counts, logits=x):
            maps = vols[:k] + off[k:]
            return lambda: ops.label_confidence(logits, ids, S, S, margins, SELECT, 0.0, *maps, counts=counts if with_counts else False)
        arms = {"label_slices_labels": lambda: ops.label_slices(x, ids, S, S, labels=vols[0]),
                "labels": conf_arm(1, False), "labels_core": conf_arm(2, False), "labels_core_envelope": conf_arm(3, False),
                "four_maps": conf_arm(4, False), "four_maps_counts": conf_arm(4, True), "counts_only": conf_arm(0, True),
                "counts_only_noise": conf_arm(0, True, noise), "torch_composition": lambda: composed(x, ids, S, S, margins, SELECT)}
        # same results first (differences are reported, not asserted away: topk's choice among tied values is its own)
        fused = [t.clone() for t in arms["four_maps_counts"]()]
        ref = composed(x, ids, S, S, margins, SELECT)
        differing = [int((a != b).sum()) for a, b in zip(fused, ref)]
        uncertain = int(fused[4][..., 2 + SELECT].sum() + fused[4][..., 2 + len(margins) + SELECT].sum())
        del fused, ref
        torch.cuda.empty_cache()
        times = dict(zip(arms, medians(list(arms.values()), reps=20 if T == 8 else 3)))
        voxels = T * S * S
        case = dict(slices=T, size=S, voxels=voxels, uncertain_voxels_of_the_band=uncertain, differing_from_composition=differing,
                    seconds={k: v for k, v in times.items()})
        res["cases"].append(case)
        print(f"{T} slices of {S}^2, {N} organs from {LOW}^2 logits ({voxels / 1e6:.1f} M voxels, {uncertain} in band {SELECT}); "
              f"elements differing from the composition (labels, core, envelope, conf, counts): {differing}")
        base = times["label_slices_labels"]
        for name, t in times.items():
            print(f"  {name:24s} {t * 1e6:10.1f} us   x{t / base:6.2f} of label_slices   {voxels / t / 1e9:7.2f} G voxels/s")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
