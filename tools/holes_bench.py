#!/usr/bin/env python3
"""Hole filling of a label volume at the workload's sizes: 64 and 8 slices of 1024^2 with 13 ellipsoid organs, each with CAVITIES enclosed
cavities of mixed sizes (1 to 128 voxels) and one enclosed blob of another label.

- `ops.label_fill_holes` on the device, flood connectivity 6 (3-D) and 4 (slice by slice), max_voxels 0 (no limit) and 64; the box call it
  starts with (`ops.label_stats` and the device-to-host copy of its table) is also timed on its own;
- `ops.label_components` (26) on the same volume beside them, as a sanity figure: one union-find pass over the whole volume;
- the host alternative on the same box's CPU share, wall clock: device -> host copy of the volume, `scipy.ndimage.binary_fill_holes` once per
  organ on the organ's bounding box (once per slice of it for connectivity 4; with a limit also `ndimage.label` and a bincount), copy back.

HIP events around `reps` back-to-back calls, the median of `rounds` such windows, the device arms alternating (every label_fill_holes call
holds one host synchronisation: the copy of the boxes).  Prints one line per case and a JSON line at the end; asserts that the device and
the host volumes are equal, nothing about time."""
import json
import os
import sys
import time

import numpy as np
import torch
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import medical_sam2_amd.ops as ops  # noqa: E402

S = 1024
N_ORGANS = 13
CAVITIES = 12
BLOB = 200                                                   # the enclosed blob's value: nobody's id


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def medians(fns, reps=10, rounds=7, warm=2):
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
    """uint8 [D, S, S]: n ellipsoids labelled 1 .. n, each cutting about half of the slices; inside each CAVITIES boxes of background (1 or 2
    slices deep, up to 8 x 8 in plane) and one box of BLOB, every one of them enclosed by the organ's own voxels on all 26 sides"""
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
    carved = 0
    for o in range(n):
        z, y, x = np.nonzero(vol == o + 1)
        if len(z) == 0:
            continue
        made = 0
        for _ in range(4000):
            if made == CAVITIES + 1:
                break
            i = rng.randint(len(z))
            d, h, w = rng.randint(1, 3), rng.randint(1, 9), rng.randint(1, 9)
            a, b, c = z[i], y[i], x[i]
            if a < 1 or b < 1 or c < 1 or a + d + 1 > D or b + h + 1 > S or c + w + 1 > S:
                continue
            if not (vol[a - 1: a + d + 1, b - 1: b + h + 1, c - 1: c + w + 1] == o + 1).all():
                continue
            vol[a: a + d, b: b + h, c: c + w] = BLOB if made == CAVITIES else 0
            made += 1
        carved += made
    return vol, carved


def host_path(labels, boxes, n, connectivity, max_voxels):
    """seconds of the host alternative (copy, fill per organ on its box, copy back) and its volume on the device"""
    st3 = ndimage.generate_binary_structure(3, 1)
    st2 = ndimage.generate_binary_structure(2, 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vol = labels.cpu().numpy()
    t_down = time.perf_counter() - t0
    out = vol.copy()

    def holes_of(organ, st):
        holes = ndimage.binary_fill_holes(organ, structure=st) & ~organ
        if max_voxels and holes.any():
            lab, k = ndimage.label(holes, structure=st)
            big = np.flatnonzero(np.bincount(lab.reshape(-1), minlength=k + 1) > max_voxels)
            holes &= ~np.isin(lab, big)
        return holes

    for v in range(1, n + 1):
        if boxes[v - 1] is None:
            continue
        z0, z1, y0, y1, x0, x1 = boxes[v - 1]
        sub, dst = vol[z0: z1 + 1, y0: y1 + 1, x0: x1 + 1], out[z0: z1 + 1, y0: y1 + 1, x0: x1 + 1]
        organ = sub == v
        if connectivity == 6:
            take = holes_of(organ, st3)
        else:
            take = np.stack([holes_of(organ[d], st2) for d in range(organ.shape[0])])
        take &= (sub == 0) & (dst == sub)                    # background voxels nobody before claimed
        dst[take] = v
    t1 = time.perf_counter()
    back = torch.from_numpy(out).to(labels.device)
    torch.cuda.synchronize()
    t_up = time.perf_counter() - t1
    return time.perf_counter() - t0, t_down, t_up, back


def main():
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    n = N_ORGANS
    res = {"size": S, "organs": n, "cavities_per_organ": CAVITIES, "cases": []}
    for D in (64, 8):
        vol, carved = organs(D, n, 100 + D)
        labels = torch.from_numpy(vol).to(dev)
        ids = ops.label_ids(list(range(1, n + 1)), dev)
        out = torch.empty_like(labels)
        st, _ = ops.label_stats(labels, ids)
        boxes = [b for _, b in ops._organ_extents(st.cpu().numpy().astype("int64"))]
        box_voxels = int(sum((b[1] - b[0] + 1) * (b[3] - b[2] + 1) * (b[5] - b[4] + 1) for b in boxes if b is not None))
        box_call = lambda: ops.label_stats(labels, ids)[0].cpu()                                           # noqa: E731
        components = lambda: ops.label_components(labels, 26)                                              # noqa: E731
        t_box, t_comp = medians([box_call, components])
        print(f"{D:2d} slices of {S}^2, {n} organs, {carved} carved boxes, {box_voxels / 1e6:.1f} M box voxels of {vol.size / 1e6:.1f} M: "
              f"box call {t_box * 1e6:.1f} us, label_components(26) {t_comp * 1e6:.1f} us", flush=True)
        for c in (6, 4):
            for mv in (0, 64):
                call = lambda: ops.label_fill_holes(labels, ids, c, max_voxels=mv or None, out=out)        # noqa: E731
                (t_fill,) = medians([call])
                filled, info = call()
                t_host, t_down, t_up, host_filled = host_path(labels, boxes, n, c, mv)
                assert torch.equal(filled, host_filled), "device and host volumes differ"
                info = info.cpu().numpy()
                case = dict(slices=D, connectivity=c, max_voxels=mv, holes=int(info[:, 0].sum()), hole_voxels=int(info[:, 1].sum()),
                            holes_filled=int(info[:, 2].sum()), voxels_filled=int(info[:, 3].sum()), box_voxels=box_voxels, box_call_s=t_box,
                            label_fill_holes_s=t_fill, label_components_s=t_comp, host_s=t_host, host_copy_down_s=t_down, host_copy_back_s=t_up)
                res["cases"].append(case)
                print(f"   c = {c}, max_voxels {mv:2d}: {case['holes']:4d} holes ({case['hole_voxels']} voxels), {case['holes_filled']:4d} filled "
                      f"({case['voxels_filled']} voxels): label_fill_holes {t_fill * 1e6:9.1f} us; host {t_host * 1e3:8.1f} ms (copy down "
                      f"{t_down * 1e3:.1f} ms, fill {(t_host - t_down - t_up) * 1e3:.1f} ms, copy back {t_up * 1e3:.1f} ms; x{t_host / t_fill:.0f})", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
