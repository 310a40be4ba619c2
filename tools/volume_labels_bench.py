#!/usr/bin/env python3
"""Label volumes from low-res logits at the workload's sizes: fp32 logits of n = 1, 4, 13 objects at 256^2 -> 1024^2, 8 slices per call.

- `ops.label_slices`: labels only, and labels + counts (5 thresholds) against a ground-truth volume;
- the composition it replaces, in the same process: `ops.bilinear_upsample` to [8 n, 1024, 1024] fp32 + torch max / compare / sums for the
  same labels and counts;
- the peak device memory of each, and the achieved fraction of 8 TB/s on the algorithmic bytes T n lh lw 4 + T H W (1 + 1).

HIP events around `reps` back-to-back calls, the median of `rounds` such windows, both arms alternating.  Prints one line per figure
and a JSON line at the end; asserts nothing about time."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import medical_sam2_amd.ops as ops  # noqa: E402

T, LOW, S = 8, 256, 1024
THRESHOLDS = (0.1, 0.3, 0.5, 0.7, 0.9)
PEAK_BYTES_PER_S = 8e12


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def medians(fns, reps=20, rounds=9, warm=3):
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


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def composed_labels(x, ids, H, W):
    Tn = x.shape[0] * x.shape[1]
    up = ops.bilinear_upsample(x.view(Tn, *x.shape[2:]), H, W).view(x.shape[0], x.shape[1], H, W)
    best_v, best = up.max(dim=1)                                   # first maximum: the lower index on ties
    return up, torch.where(best_v > 0, ids[best], torch.zeros((), dtype=torch.uint8, device=x.device))


def composed_counts(x, ids, H, W, gt, thr):
    up, labels = composed_labels(x, ids, H, W)
    G = gt[:, None] == ids[None, :, None, None]
    out = torch.empty(len(thr), x.shape[0], x.shape[1], 3, dtype=torch.int32, device=x.device)
    out[..., 2] = G.sum((-1, -2))
    for k, t in enumerate(thr):
        P = up > t
        out[k, ..., 1] = P.sum((-1, -2))
        out[k, ..., 0] = (P & G).sum((-1, -2))
    return labels, out


def main():
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    res = {"slices_per_call": T, "low": LOW, "size": S, "cases": []}
    for n in (1, 4, 13):
        g = torch.Generator().manual_seed(n)
        smooth = torch.nn.functional.interpolate(torch.randn(T, n, 32, 32, generator=g), size=(LOW, LOW), mode="bilinear", align_corners=False)
        x = (smooth * 6 - 2).to(dev).contiguous()                 # organ-like blobs: most voxels background, every object somewhere
        ids = ops.label_ids(list(range(1, n + 1)), dev)
        gt = torch.randint(0, n + 1, (T, S // 64, S // 64), generator=g).to(torch.uint8).repeat_interleave(64, 1).repeat_interleave(64, 2).to(dev).contiguous()
        thr = torch.tensor(THRESHOLDS, dtype=torch.float32, device=dev)
        labels = torch.empty(T, S, S, dtype=torch.uint8, device=dev)
        fused_l = lambda: ops.label_slices(x, ids, S, S, labels=labels)
        fused_c = lambda: ops.label_slices(x, ids, S, S, gt=gt, thresholds=thr, labels=labels)
        comp_l = lambda: composed_labels(x, ids, S, S)
        comp_c = lambda: composed_counts(x, ids, S, S, gt, THRESHOLDS)
        # same results first (differences are reported, not asserted away: the two up-sampling forms agree bit for bit by construction)
        lab_f, cnt_f = fused_c()
        lab_c, cnt_c = comp_c()
        diff_l, diff_c = int((lab_f != lab_c).sum()), int((cnt_f != cnt_c).sum())
        t_fl, t_cl, t_fc, t_cc = medians([fused_l, comp_l, fused_c, comp_c])
        p_fl, p_cl, p_fc, p_cc = peak(fused_l), peak(comp_l), peak(fused_c), peak(comp_c)
        alg = T * n * LOW * LOW * 4 + T * S * S * 2
        case = dict(n=n, label_voxels_differing=diff_l, counts_differing=diff_c, labels_s=t_fl, labels_composed_s=t_cl, counts_s=t_fc,
                    counts_composed_s=t_cc, labels_peak_bytes=p_fl, labels_composed_peak_bytes=p_cl, counts_peak_bytes=p_fc,
                    counts_composed_peak_bytes=p_cc, algorithmic_bytes=alg, labels_fraction_of_8TBps=alg / t_fl / PEAK_BYTES_PER_S,
                    counts_fraction_of_8TBps=alg / t_fc / PEAK_BYTES_PER_S)
        res["cases"].append(case)
        print(f"n = {n:2d}: labels {t_fl * 1e6:8.1f} us (composition {t_cl * 1e6:9.1f} us, x{t_cl / t_fl:.1f}), labels + counts {t_fc * 1e6:8.1f} us "
              f"(composition {t_cc * 1e6:9.1f} us, x{t_cc / t_fc:.1f}); peak memory {p_fl / 2**20:.1f} / {p_fc / 2**20:.1f} MiB against "
              f"{p_cl / 2**20:.0f} / {p_cc / 2**20:.0f} MiB; {alg / 2**20:.1f} MiB algorithmic = {100 * alg / t_fl / PEAK_BYTES_PER_S:.1f} % / "
              f"{100 * alg / t_fc / PEAK_BYTES_PER_S:.1f} % of 8 TB/s; differing label voxels {diff_l}, counts {diff_c}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
