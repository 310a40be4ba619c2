#!/usr/bin/env python3
"""Box and click prompts from a label volume at the workload's sizes: 8 and 64 slices of 1024^2 with 1, 4 and 13 organs.

- `ops.label_stats` (the boxes), and `ops.label_stats` + `ops.label_pick` (the clicks, from uniform words), on the device;
- the host path of `data.BTCVVolumes`, on the same box: `data.generate_bbox` and `data.random_click` once per (slice, present object)
  pair on numpy masks (wall clock around the calls alone; building the masks is not counted);
- the achieved fraction of 8 TB/s on the algorithmic bytes: one read of the volume, D H W.

HIP events around `reps` back-to-back calls, the median of `rounds` such windows, the two device arms alternating.  Prints one line per
case and a JSON line at the end; asserts the two paths' boxes equal, nothing about time."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import medical_sam2_amd.data as data  # noqa: E402
import medical_sam2_amd.ops as ops  # noqa: E402

S = 1024
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


def organs(D, n, seed):
    """uint8 [D, S, S]: n ellipsoids labelled 1 .. n, each cutting about half of the slices"""
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:S, 0:S].astype(np.float32)
    vol = np.zeros((D, S, S), dtype=np.uint8)
    for o in range(n):
        cz, cy, cx = rng.uniform(0.3, 0.7, 3)
        rz, ry, rx = rng.uniform(0.25, 0.4), rng.uniform(0.05, 0.15), rng.uniform(0.05, 0.15)
        for d in range(D):
            dz = ((d + 0.5) / D - cz) / rz
            if abs(dz) < 1:
                s = np.sqrt(1 - dz * dz)
                vol[d][((ys / S - cy) / (ry * s)) ** 2 + ((xs / S - cx) / (rx * s)) ** 2 <= 1.0] = o + 1
    return vol


def host_path(vol, n):
    """seconds inside generate_bbox / random_click over all present pairs, and the boxes [D, n, 4] (-1 where absent)"""
    t_box = t_click = 0.0
    boxes = np.full((vol.shape[0], n, 4), -1, dtype=np.int64)
    pairs = 0
    for d in range(vol.shape[0]):
        for o in np.unique(vol[d][vol[d] > 0]):
            mask = vol[d] == o
            t0 = time.perf_counter()
            boxes[d, o - 1] = data.generate_bbox(mask)
            t1 = time.perf_counter()
            data.random_click(mask, 1, seed=0)
            t2 = time.perf_counter()
            t_box, t_click, pairs = t_box + t1 - t0, t_click + t2 - t1, pairs + 1
    return t_box, t_click, pairs, boxes


def main():
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    res = {"size": S, "cases": []}
    for D in (8, 64):
        for n in (1, 4, 13):
            vol = organs(D, n, 10 * D + n)
            labels = torch.from_numpy(vol).to(dev)
            ids = ops.label_ids(list(range(1, n + 1)), dev)
            rows = torch.empty(D, n, S, dtype=torch.int32, device=dev)
            u = torch.randint(-2 ** 31, 2 ** 31, (D, n), dtype=torch.int64).to(torch.int32).to(dev)
            stats_only = lambda: ops.label_stats(labels, ids, rows=rows)
            stats_pick = lambda: ops.label_pick(labels, ids, *ops.label_stats(labels, ids, rows=rows), u=u)
            t_stats, t_both = medians([stats_only, stats_pick])
            h_box, h_click, pairs, boxes = host_path(vol, n)
            st = stats_only()[0].cpu().numpy()
            assert np.array_equal(st[..., [3, 1, 4, 2]], boxes), "device and host boxes differ"
            alg = D * S * S
            case = dict(slices=D, n=n, pairs=pairs, label_stats_s=t_stats, label_stats_pick_s=t_both, host_bbox_s=h_box, host_click_s=h_click,
                        algorithmic_bytes=alg, stats_fraction_of_8TBps=alg / t_stats / PEAK_BYTES_PER_S,
                        stats_pick_fraction_of_8TBps=alg / t_both / PEAK_BYTES_PER_S)
            res["cases"].append(case)
            print(f"{D:2d} slices, n = {n:2d} ({pairs:3d} pairs): label_stats {t_stats * 1e6:7.1f} us ({100 * alg / t_stats / PEAK_BYTES_PER_S:.1f} % of 8 TB/s), "
                  f"+ label_pick {t_both * 1e6:7.1f} us ({100 * alg / t_both / PEAK_BYTES_PER_S:.1f} %); host generate_bbox {h_box * 1e3:8.1f} ms "
                  f"(x{h_box / t_stats:.0f}), random_click {h_click * 1e3:8.1f} ms (x{h_click / t_both:.0f})")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
