#!/usr/bin/env python3
"""3-D connected components and island removal of a label volume at the workload's sizes: 8 and 64 slices of 1024^2 with 1, 4 and 13
ellipsoid organs, each with a few dozen small islands of its own value scattered over the volume.

- `ops.label_components` at 26-connectivity, and `ops.label_components` + `ops.label_clean` (keep the largest component per organ), on the
  device;
- the achieved fraction of 8 TB/s on the algorithmic bytes: one read of the volume, one write each of comp, size (int32) and out: 10 D H W;
- the host alternative on the same box's CPU share, wall clock: device -> host copy of the volume, `scipy.ndimage.label` once per organ,
  largest-component selection in numpy, copy back.

HIP events around `reps` back-to-back calls, the median of `rounds` such windows, the two device arms alternating.  Prints one line per
case and a JSON line at the end; asserts the two cleaned volumes equal, nothing about time."""
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
PEAK_BYTES_PER_S = 8e12
ISLANDS = 36


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
    """uint8 [D, S, S]: n ellipsoids labelled 1 .. n, each cutting about half of the slices, plus ISLANDS small blobs of each value"""
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
    for o in range(n):
        for _ in range(ISLANDS):
            d, r, c = rng.randint(0, D), rng.randint(0, S - 12), rng.randint(0, S - 12)
            h, w = rng.randint(2, 12, 2)
            vol[d, r: r + h, c: c + w] = o + 1
    return vol


def host_path(labels, n):
    """seconds of the host alternative, and its cleaned volume (on the device again)"""
    st = ndimage.generate_binary_structure(3, 3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vol = labels.cpu().numpy()
    out = vol.copy()
    for v in range(1, n + 1):
        lab, k = ndimage.label(vol == v, structure=st)
        if k > 1:
            count = np.bincount(lab.reshape(-1), minlength=k + 1)
            count[0] = 0
            out[(lab > 0) & (lab != int(np.argmax(count)))] = 0          # argmax: the first maximum = the smaller canonical index
    back = torch.from_numpy(out).to(labels.device)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, back


def main():
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    res = {"size": S, "connectivity": 26, "cases": []}
    for D in (8, 64):
        for n in (1, 4, 13):
            vol = organs(D, n, 10 * D + n)
            labels = torch.from_numpy(vol).to(dev)
            ids = ops.label_ids(list(range(1, n + 1)), dev)
            out = torch.empty_like(labels)
            label_only = lambda: ops.label_components(labels, 26)
            label_clean = lambda: ops.label_clean(labels, *ops.label_components(labels, 26), ids, keep_largest=True, out=out)
            t_label, t_both = medians([label_only, label_clean])
            cleaned, info = label_clean()
            t_host, host_clean = host_path(labels, n)
            assert torch.equal(cleaned, host_clean), "device and host cleaned volumes differ"
            info = info.cpu().numpy()
            alg = 10 * D * S * S
            case = dict(slices=D, n=n, components=int(info[:, 0].sum()), voxels_removed=int((info[:, 1] - info[:, 5]).sum()),
                        label_components_s=t_label, label_components_clean_s=t_both, host_s=t_host, algorithmic_bytes=alg,
                        label_fraction_of_8TBps=(alg - D * S * S) / t_label / PEAK_BYTES_PER_S, clean_fraction_of_8TBps=alg / t_both / PEAK_BYTES_PER_S)
            res["cases"].append(case)
            print(f"{D:2d} slices, n = {n:2d} ({case['components']:4d} components): label_components {t_label * 1e6:8.1f} us, + label_clean "
                  f"{t_both * 1e6:8.1f} us ({100 * case['clean_fraction_of_8TBps']:.1f} % of 8 TB/s on {alg / 1e6:.0f} MB); host {t_host * 1e3:8.1f} ms "
                  f"(x{t_host / t_both:.0f})", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
