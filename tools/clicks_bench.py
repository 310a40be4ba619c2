#!/usr/bin/env python3
"""Corrective clicks from error regions at the workload's sizes: 8 and 64 slices of 1024^2 with 13 organs, the prediction = the ground truth
moved by (5, 7) voxels with two organs missing on every third slice.

- `ops.label_error_clicks` in both modes on the device (workspace and table allocated once);
- the centre mode on thick regions, where a voxel's column scan is as long as its distance to the border: every organ missing from the
  prediction, and one region that fills every slice (the worst case); medians of 3 windows of 2 calls;
- the host alternative, on the same box: per (slice, object) pair with an error voxel the two full-resolution error masks, a zero-padded
  `scipy.ndimage.distance_transform_edt` of each and an argmax (wall clock around those calls; at most `HOST_PAIRS` pairs are run, the time
  of all pairs is that sample's mean times the pair count and printed as an extrapolation); asserts the sampled clicks equal;
- the scoring half of one refinement round as `interactive.refine_volume` runs it, without the predictor's propagation: `label_volume` of
  fp32 low-res logits [D, 13, 256, 256] at 1024^2, `ops.label_overlap`, `corrective_clicks`, `worst_slices` and the round's one
  device-to-host copy (host clock around the work, which ends in that copy);
- the achieved fraction of 8 TB/s on the algorithmic bytes of the centre mode: both volumes read by the row pass and by the column pass, the
  row distances of both kinds written and read once: 12 D H W.

HIP events around `reps` back-to-back calls, the median of `rounds` such windows, the two device arms alternating.  Prints one line per
case and a JSON line at the end; nothing about time is asserted."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import medical_sam2_amd.ops as ops  # noqa: E402
from medical_sam2_amd.prompts import corrective_clicks, worst_slices  # noqa: E402
from medical_sam2_amd.volume_labels import label_volume  # noqa: E402
from tools.prompts_bench import medians, organs  # noqa: E402

S, N, LOW = 1024, 13, 256
HOST_PAIRS = 24
PEAK_BYTES_PER_S = 8e12


def host_clicks(pred, gt, pairs):
    """seconds over `pairs` (slice, object index) pairs, and their (x, y, label)"""
    from scipy.ndimage import distance_transform_edt
    out, t = [], 0.0
    for d, j in pairs:
        t0 = time.perf_counter()
        v = j + 1
        fn, fp = (gt[d] == v) & (pred[d] != v), (pred[d] == v) & (gt[d] != v)
        d_fn, d_fp = (distance_transform_edt(np.pad(r, 1))[1:-1, 1:-1] for r in (fn, fp))
        positive = d_fn.max() > d_fp.max()
        y, x = np.unravel_index(int(np.argmax(d_fn if positive else d_fp)), fn.shape)
        t += time.perf_counter() - t0
        out.append((int(x), int(y), int(positive)))
    return t, out


def main():
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    res = {"size": S, "n": N, "cases": []}
    obj_ids = list(range(1, N + 1))
    for D in (8, 64):
        gt = organs(D, N, 10 * D + N)
        pred = np.roll(gt, (5, 7), axis=(1, 2))
        pred[2::3][np.isin(pred[2::3], (2, 9))] = 0
        p, g = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
        ids = ops.label_ids(obj_ids, dev)
        table = torch.empty(D, N, 8, dtype=torch.int32, device=dev)
        ws = {m: ops._workspace8(ops.label_error_clicks_workspace_bytes(D, S, S, N, m), dev) for m in ops.CLICK_MODES}
        u = torch.randint(-2 ** 31, 2 ** 31, (D, N), dtype=torch.int64).to(torch.int32).to(dev)
        center = lambda: ops.label_error_clicks(p, g, ids, workspace=ws["center"], out=table)
        uniform = lambda: ops.label_error_clicks(p, g, ids, "uniform", u=u, workspace=ws["uniform"], out=table)
        t_center, t_uniform = medians([center, uniform])
        # thick regions: the column scan of a voxel is as long as its distance to the region's border.  Every organ missing from the
        # prediction (a first round before any mask), and the worst case, one region that fills every slice
        empty, filled = torch.zeros_like(p), torch.full_like(g, 1)
        missing = lambda: ops.label_error_clicks(empty, g, ids, workspace=ws["center"], out=table)
        full = lambda: ops.label_error_clicks(empty, filled, ids, workspace=ws["center"], out=table)
        t_missing, t_full = medians([missing, full], reps=2, rounds=3, warm=1)
        got = center().cpu().numpy()
        with_error = [(d, j) for d in range(D) for j in range(N) if got[d, j, 3] + got[d, j, 4] > 0]
        sample = with_error[:: max(1, len(with_error) // HOST_PAIRS)][:HOST_PAIRS]
        t_host, host = host_clicks(pred, gt, sample)
        assert [tuple(got[d, j, :3]) for d, j in sample] == host, "device and host clicks differ"
        host_all = t_host / len(sample) * len(with_error)
        # the scoring half of a refinement round
        logits = torch.randn(D, N, LOW, LOW, device=dev)

        def scoring():
            labels = label_volume(logits, S, S, obj_ids)
            counts = ops.label_overlap(labels, g, ids)
            points, point_labels, errors = corrective_clicks(labels, g, obj_ids)
            where = worst_slices(errors)
            return torch.cat([counts.reshape(-1).to(torch.int64), where.reshape(-1), point_labels.reshape(-1).to(torch.int64)]).cpu()
        for _ in range(3):
            scoring()
        rounds = []
        for _ in range(9):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            scoring()
            rounds.append(time.perf_counter() - t0)
        t_round = float(np.median(rounds))
        alg = 12 * D * S * S
        res["cases"].append(dict(slices=D, pairs_with_error=len(with_error), error_clicks_center_s=t_center, error_clicks_uniform_s=t_uniform,
                                 error_clicks_center_all_organs_missing_s=t_missing, error_clicks_center_full_slices_s=t_full,
                                 host_pairs_run=len(sample), host_s_per_pair=t_host / len(sample), host_all_pairs_s_extrapolated=host_all,
                                 round_scoring_s=t_round, algorithmic_bytes=alg, center_fraction_of_8TBps=alg / t_center / PEAK_BYTES_PER_S))
        print(f"{D:2d} slices, n = {N} ({len(with_error)} pairs with error): centre {t_center * 1e6:8.1f} us ({100 * alg / t_center / PEAK_BYTES_PER_S:.1f} % "
              f"of 8 TB/s on 12 D H W), uniform {t_uniform * 1e6:8.1f} us, centre with every organ missing {t_missing * 1e3:.2f} ms, with one region filling "
              f"every slice {t_full * 1e3:.2f} ms; host {t_host / len(sample) * 1e3:.1f} ms per pair over {len(sample)} pairs, "
              f"all pairs {host_all:.2f} s extrapolated (x{host_all / t_center:.0f}); scoring half of a round {t_round * 1e3:.2f} ms")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
