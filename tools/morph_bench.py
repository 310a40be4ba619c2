#!/usr/bin/env python3
"""Morphology of a label volume at the workload's sizes: 64 and 8 slices of 1024^2 with 13 ellipsoid organs (tools/holes_bench.py's volume,
cavities included) at spacing (3, 0.76, 0.76) mm; erode, dilate, open and close at 2 mm and 5 mm.

- `ops.label_morph` on the device, out of place, claim="background"; the box call it starts with (`ops.label_stats` and the device-to-host
  copy of its table) is also timed on its own;
- the host alternative on the same box's CPU share, wall clock, once: device -> host copy of the volume, `scipy.ndimage.binary_*` with the
  ellipsoid structure of the radius once per organ on the organ's box grown as the device grows it (erosions with border_value=1), copy
  back.  It writes a dilation or closing back in the order of ids (no nearest-wins rule), so only erode and open are compared with the
  device volume, voxel for voxel.  The host arm stops being measured once it has used --host-budget seconds in all: such cases print
  "not measured".

HIP events around `reps` back-to-back calls, the median of `rounds` such windows (every label_morph call holds one host synchronisation: the
copy of the boxes).  Prints one line per case and a JSON line at the end; asserts nothing about time."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import medical_sam2_amd.ops as ops  # noqa: E402
from holes_bench import N_ORGANS, S, medians, organs  # noqa: E402

SPACING = (3.0, 0.76, 0.76)
RADII_MM = (2.0, 5.0)
OPS = ("erode", "dilate", "open", "close")


def ellipsoid(r2):
    """(structure, reach per axis): the offsets with ((sx2 dx^2 + sy2 dy^2) + sz2 dz^2) <= r2"""
    reach = [int(np.floor(np.sqrt(r2) / s)) for s in SPACING]
    z, y, x = np.mgrid[-reach[0]: reach[0] + 1, -reach[1]: reach[1] + 1, -reach[2]: reach[2] + 1].astype(np.float64)
    sz2, sy2, sx2 = (np.float64(s) * np.float64(s) for s in SPACING)
    return (sx2 * (x * x) + sy2 * (y * y)) + sz2 * (z * z) <= r2, reach


def host_path(labels, boxes, n, op, r2):
    """seconds of the host alternative (copy, one scipy call per organ and stage on its grown box, copy back) and its volume on the device"""
    st, reach = ellipsoid(r2)
    grow = [(0 if op == "dilate" else 1) + (k if op in ("dilate", "close") else 0) for k in reach]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vol = labels.cpu().numpy()
    t_down = time.perf_counter() - t0
    out = vol.copy()
    for v in range(1, n + 1):
        if boxes[v - 1] is None:
            continue
        b = boxes[v - 1]
        sl = tuple(slice(max(b[2 * a] - grow[a], 0), min(b[2 * a + 1] + grow[a], vol.shape[a] - 1) + 1) for a in range(3))
        sub, dst = vol[sl], out[sl]
        organ = sub == v
        if op == "erode":
            res = ndimage.binary_erosion(organ, st, border_value=1)
        elif op == "dilate":
            res = ndimage.binary_dilation(organ, st)
        elif op == "open":
            res = ndimage.binary_dilation(ndimage.binary_erosion(organ, st, border_value=1), st)
        else:
            res = ndimage.binary_erosion(ndimage.binary_dilation(organ, st), st, border_value=1)
        if op in ("erode", "open"):
            dst[organ & ~res] = 0
        else:
            dst[res & (sub == 0) & (dst == 0)] = v
    t1 = time.perf_counter()
    back = torch.from_numpy(out).to(labels.device)
    torch.cuda.synchronize()
    t_up = time.perf_counter() - t1
    return time.perf_counter() - t0, t_down, t_up, back


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-budget", type=float, default=240.0, help="seconds of the host arm in all; later cases are not measured on the host")
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    n = N_ORGANS
    res = {"size": S, "organs": n, "spacing": SPACING, "cases": []}
    host_used = 0.0
    for D in (8, 64):
        vol, _ = organs(D, n, 100 + D)
        labels = torch.from_numpy(vol).to(dev)
        ids = ops.label_ids(list(range(1, n + 1)), dev)
        out = torch.empty_like(labels)
        st, _ = ops.label_stats(labels, ids)
        boxes = [b for _, b in ops._organ_extents(st.cpu().numpy().astype("int64"))]
        box_voxels = int(sum((b[1] - b[0] + 1) * (b[3] - b[2] + 1) * (b[5] - b[4] + 1) for b in boxes if b is not None))
        (t_box,) = medians([lambda: ops.label_stats(labels, ids)[0].cpu()])
        print(f"{D:2d} slices of {S}^2, {n} organs, {box_voxels / 1e6:.1f} M box voxels of {vol.size / 1e6:.1f} M, spacing {SPACING}: "
              f"box call {t_box * 1e6:.1f} us", flush=True)
        for mm in RADII_MM:
            for op in OPS:
                call = lambda: ops.label_morph(labels, ids, op, radius=mm, spacing=SPACING, out=out)      # noqa: E731
                (t_dev,) = medians([call], reps=5, rounds=5)
                got, info = call()
                info = info.cpu().numpy()
                case = dict(slices=D, op=op, radius_mm=mm, voxels_before=int(info[:, 0].sum()), voxels_result=int(info[:, 1].sum()),
                            voxels_after=int(info[:, 2].sum()), box_voxels=box_voxels, box_call_s=t_box, label_morph_s=t_dev, host_s=None)
                host = "host not measured"
                if host_used < args.host_budget:
                    t_host, t_down, t_up, back = host_path(labels, boxes, n, op, mm * mm)
                    host_used += t_host
                    if op in ("erode", "open"):
                        assert torch.equal(got, back), "device and host volumes differ"
                    case.update(host_s=t_host, host_copy_down_s=t_down, host_copy_back_s=t_up)
                    host = (f"host {t_host * 1e3:8.1f} ms (copy down {t_down * 1e3:.1f} ms, scipy {(t_host - t_down - t_up) * 1e3:.1f} ms, copy back "
                            f"{t_up * 1e3:.1f} ms; x{t_host / t_dev:.0f})")
                res["cases"].append(case)
                print(f"   {op:6s} {mm:.0f} mm: {case['voxels_before']} -> {case['voxels_after']} voxels (result sets {case['voxels_result']}): "
                      f"label_morph {t_dev * 1e6:9.1f} us; {host}", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
