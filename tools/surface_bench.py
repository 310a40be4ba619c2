#!/usr/bin/env python3
"""Surface-distance scores (HD95, ASSD, NSD) of a label volume at the workload's sizes: 8 and 64 slices of 1024^2 with 13 ellipsoid organs.
The prediction is the ground truth shifted by a few voxels, with a few dozen small islands of every organ's value scattered around the organ.

- `volume_labels.surface_scores` on the device (two `ops.label_stats`, `ops.surface_segments`, then sorting and the reductions);
- `ops.surface_segments` alone (the distance kernels and the two stats passes);
- the host alternative on the same box's CPU share, wall clock: device -> host copy of both volumes, then per organ, cropped to the same
  boxes: the two surfaces by erosion and two `scipy.ndimage.distance_transform_edt` calls with the spacing.

HIP events around `reps` back-to-back calls, the median of `rounds` such windows, the two device arms alternating.  Prints one line per
case and a JSON line at the end; asserts that the two sets of scores agree (hd95 / assd to 1e-9 relative: scipy sums in another order),
nothing about time."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import medical_sam2_amd.ops as ops  # noqa: E402
from medical_sam2_amd.volume_labels import surface_scores  # noqa: E402

SPACING = (3.0, 0.76, 0.76)
ISLANDS = 24
SHIFT = (1, 3, -4)
WORKSPACE_BYTES = 4 << 30


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def medians(fns, reps=3, rounds=5, warm=1):
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


def organs(D, S, n, seed):
    """(pred, gt) uint8 [D, S, S]: n ellipsoids labelled 1 .. n in gt, each cutting about half of the slices; pred = gt rolled by SHIFT plus
    ISLANDS small blobs of each value within a few dozen voxels of its organ"""
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:S, 0:S].astype(np.float32)
    gt = np.zeros((D, S, S), dtype=np.uint8)
    centres = []
    for o in range(n):
        cz, cy, cx = rng.uniform(0.3, 0.7, 3)
        rz, ry, rx = rng.uniform(0.25, 0.4), rng.uniform(0.05, 0.15), rng.uniform(0.05, 0.15)
        centres.append((cz, cy, cx, rz, ry, rx))
        for d in range(D):
            dz = ((d + 0.5) / D - cz) / rz
            if abs(dz) < 1:
                s = np.sqrt(1 - dz * dz)
                gt[d][((ys / S - cy) / (ry * s)) ** 2 + ((xs / S - cx) / (rx * s)) ** 2 <= 1.0] = o + 1
    pred = np.roll(gt, SHIFT, axis=(0, 1, 2))
    for o, (cz, cy, cx, rz, ry, rx) in enumerate(centres):
        for _ in range(ISLANDS):
            d = int(np.clip(rng.normal(cz, rz) * D, 0, D - 1))
            r = int(np.clip((cy + rng.uniform(-1.3, 1.3) * ry) * S, 0, S - 12))
            c = int(np.clip((cx + rng.uniform(-1.3, 1.3) * rx) * S, 0, S - 12))
            h, w = rng.randint(2, 12, 2)
            pred[d, r: r + h, c: c + w] = o + 1
    return np.ascontiguousarray(pred), gt


def host_path(pred_d, gt_d, n, percentile, tolerances):
    """seconds of the host alternative, and its scores"""
    cross = ndimage.generate_binary_structure(3, 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pred, gt = pred_d.cpu().numpy(), gt_d.cpu().numpy()
    bp, bg = ndimage.find_objects(pred, max_label=n), ndimage.find_objects(gt, max_label=n)
    out = {"hd": np.full(n, np.nan), "hd95": np.full(n, np.nan), "assd": np.full(n, np.nan), "nsd": np.full((n, len(tolerances)), np.nan)}
    for v in range(1, n + 1):
        a, b = bp[v - 1], bg[v - 1]
        if a is None or b is None:
            continue
        box = tuple(slice(min(p.start, q.start), max(p.stop, q.stop)) for p, q in zip(a, b))   # everything equal to v lies inside
        mp, mg = pred[box] == v, gt[box] == v
        sp, sg = mp ^ ndimage.binary_erosion(mp, cross, border_value=0), mg ^ ndimage.binary_erosion(mg, cross, border_value=0)
        d_pg = ndimage.distance_transform_edt(~sg, sampling=SPACING)[sp]
        d_gp = ndimage.distance_transform_edt(~sp, sampling=SPACING)[sg]
        m = len(d_pg) + len(d_gp)
        out["hd"][v - 1] = max(d_pg.max(), d_gp.max())
        out["hd95"][v - 1] = max(np.percentile(d_pg, percentile), np.percentile(d_gp, percentile))
        out["assd"][v - 1] = (d_pg.sum() + d_gp.sum()) / m
        out["nsd"][v - 1] = [((d_pg <= t).sum() + (d_gp <= t).sum()) / m for t in tolerances]
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--slices", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--organs", type=int, default=13)
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    S, n = args.size, args.organs
    tol = (1.0, 2.0)
    res = {"size": S, "organs": n, "spacing": SPACING, "workspace_bytes": WORKSPACE_BYTES, "cases": []}
    for D in args.slices:
        pred_h, gt_h = organs(D, S, n, 10 * D + n)
        pred, gt = torch.from_numpy(pred_h).to(dev), torch.from_numpy(gt_h).to(dev)
        ids = ops.label_ids(list(range(1, n + 1)), dev)
        distances = lambda: ops.surface_segments(pred, gt, ids, SPACING, WORKSPACE_BYTES)                       # noqa: E731
        scores = lambda: surface_scores(pred, gt, ids, SPACING, 95.0, tol, WORKSPACE_BYTES)              # noqa: E731
        t_dist, t_scores = medians([distances, scores])
        got = scores()
        _, _, caps, counts = distances()
        t_host, want = host_path(pred, gt, n, 95.0, tol)
        for k in ("hd", "hd95", "assd", "nsd"):
            assert np.allclose(got[k], want[k], rtol=1e-9, atol=0.0, equal_nan=True), (k, got[k], want[k])
        case = dict(slices=D, surface_voxels=int(counts.sum()), organ_voxels=int(np.sum(caps)), surface_segments_s=t_dist,
                    surface_scores_s=t_scores, host_s=t_host, mean_hd95=float(np.nanmean(got["hd95"])), mean_assd=float(np.nanmean(got["assd"])))
        res["cases"].append(case)
        print(f"{D:2d} slices, {n} organs ({case['surface_voxels']} surface voxels): surface_segments {t_dist * 1e3:8.2f} ms, surface_scores "
              f"{t_scores * 1e3:8.2f} ms; host {t_host * 1e3:9.1f} ms (x{t_host / t_scores:.0f}); mean HD95 {case['mean_hd95']:.3f} mm", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
