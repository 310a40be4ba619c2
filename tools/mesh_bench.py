#!/usr/bin/env python3
"""Surface meshes at the workload's sizes: 8 slices of 512^2 and 64 slices of 1024^2, 13 organs (the ellipsoids of tools/measure_bench.py).

- `ops.label_mesh_sizes` (msam2_label_mesh_count: one pass over the volume);
- msam2_label_mesh alone, on caller-owned tables and workspace with the boxes and sizes prepared once (no allocation, no host round trip in
  the window), as "corner", "nets" and "nets" + 3 relaxation sweeps; and `ops.label_mesh` as a user calls it ("nets"): label_stats, the sizes,
  the one device-to-host copy, the allocations and the entry;
- `ops.label_measure(faces=True)` on the same labels, caller-owned tables: it reads the same bytes and is the yardstick;
- the vertices and quads produced, and the achieved fraction of 8 TB/s on the algorithmic bytes: one read of the labels, D H W, plus the
  tables written (12 bytes per vertex, 16 per quad; the count entry writes nothing to speak of);
- the host alternative on the same box: the device-to-host copy of the volume plus the vectorised numpy restatement
  (tests/mesh_restate.organ_mesh, "nets"), wall clock, once.  No third-party mesher (skimage, trimesh, vtk) is installed to compare with.

HIP events around `reps` back-to-back calls, the median of `rounds` such windows, the device arms alternating.  Prints one line per case
and a JSON line at the end (--profile: before it, the device time per kernel of the last case); asserts that the device tables equal
the restatement's bit for bit, nothing about time.  --out FILE also writes the lines there."""
import argparse
import ctypes
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_restate as R  # noqa: E402

import medical_sam2_amd.ops as ops  # noqa: E402
from medical_sam2_amd import _lib  # noqa: E402
from tools.measure_bench import medians, organs  # noqa: E402

N_ORGANS = 13
PEAK_BYTES_PER_S = 8e12
SPACING, ORIGIN = (3.0, 0.76, 0.76), (0.0, 0.0, 0.0)
FORMS = {"corner": ("corner", 0), "nets": ("nets", 0), "nets_relax3": ("nets", 3)}


class Entry:
    """msam2_label_mesh on tables, workspace and host arrays made once"""

    def __init__(self, labels, values, boxes, sizes, placement, relax):
        self.L, n = _lib.lib(), len(values)
        D, H, W = labels.shape
        v_offs, q_offs = np.concatenate([[0], np.cumsum(sizes[:, 0])]), np.concatenate([[0], np.cumsum(sizes[:, 1])])
        dev = labels.device
        self.vertices = torch.empty(int(v_offs[-1]), 3, dtype=torch.float32, device=dev)
        self.quads = torch.empty(int(q_offs[-1]), 4, dtype=torch.int32, device=dev)
        self.counts = torch.empty(n, 2, dtype=torch.int32, device=dev)
        self.offs = (v_offs, q_offs)
        self.nb = sum(self.L.msam2_label_mesh_workspace_bytes((ctypes.c_int32 * 6)(*b), relax) for b in boxes)
        self.ws = torch.empty((self.nb + 15) // 16 * 2, dtype=torch.int64, device=dev)
        i64 = lambda rows: (ctypes.c_int64 * n)(*[int(r) for r in rows])                                   # noqa: E731
        self.args = (labels.data_ptr(), D, H, W, (ctypes.c_uint8 * n)(*values), (ctypes.c_int32 * (6 * n))(*[v for b in boxes for v in b]),
                     i64(v_offs[:-1]), i64(sizes[:, 0]), i64(q_offs[:-1]), i64(sizes[:, 1]), n, ops.MESH_PLACEMENTS[placement], relax,
                     (ctypes.c_double * 3)(*SPACING), (ctypes.c_double * 3)(*ORIGIN), self.vertices.data_ptr(), self.quads.data_ptr(),
                     self.counts.data_ptr(), self.ws.data_ptr(), self.nb)
        self.keep = labels

    def __call__(self):
        ops.check(self.L.msam2_label_mesh(*self.args, ops._stream()))


def kernel_profile(entry, sizes_fn, what, calls=5):
    """device time per kernel of msam2_label_mesh ("nets" + 3 sweeps) and of the count pass: torch.profiler over `calls` calls of each"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            entry()
            sizes_fn()
        torch.cuda.synchronize()
    found = [(re.search(r"mesh_\w+_kernel", e.key), e) for e in prof.key_averages()]
    rows = [(m.group(0), e.count, getattr(e, "device_time_total", 0.0) / e.count) for m, e in found if m]
    rows.sort(key=lambda r: -r[1] * r[2])
    return [f"kernels of {what}, nets + 3 sweeps and the count pass, {calls} calls each (torch.profiler):"] + \
           [f"  {name:26s} {count // calls} per call, {us:7.1f} us each" for name, count, us in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="8x512,64x1024", help="slices x side, comma separated")
    ap.add_argument("--profile", action="store_true", help="also the device time per kernel of the last case (torch.profiler, five calls)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mesh_bench needs the MI355X"
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    res, lines = {"organs": N_ORGANS, "cases": []}, []
    idl = list(range(1, N_ORGANS + 1))
    for D, S in (tuple(int(x) for x in c.split("x")) for c in args.cases.split(",")):
        vol = organs(D, S, N_ORGANS, 10 * D + S)
        labels = torch.from_numpy(vol).to(dev)
        ids = ops.label_ids(idl, dev)
        values, (extents,), sizes = ops._organ_boxes("mesh_bench", (labels,), ids, extra=ops.label_mesh_sizes(labels, ids))
        boxes, sizes = ops._boxes_or_empty(extents), sizes.reshape(N_ORGANS, 2)
        entries = {k: Entry(labels, values, boxes, sizes, *form) for k, form in FORMS.items()}
        measure_out = ops.label_measure(labels, ids, faces=True)
        fns = [lambda: ops.label_mesh_sizes(labels, ids)] + list(entries.values())
        fns += [lambda: ops.label_mesh(labels, ids, SPACING, ORIGIN, "nets", 0), lambda: ops.label_measure(labels, ids, faces=True, out=measure_out)]
        names = ["sizes"] + list(entries) + ["ops_label_mesh_nets", "label_measure_faces"]
        t = dict(zip(names, medians(fns, reps=10, rounds=7)))
        torch.cuda.synchronize()
        nv, nq = int(sizes[:, 0].sum()), int(sizes[:, 1].sum())
        assert torch.equal(entries["nets"].counts.cpu().to(torch.int64), torch.from_numpy(sizes))
        assert torch.equal(measure_out[3].sum(dim=1).cpu(), torch.from_numpy(sizes[:, 1]))
        t0 = time.perf_counter()
        host_vol = labels.cpu().numpy()
        t_copy = time.perf_counter() - t0
        host = [R.organ_mesh(host_vol, v, SPACING, ORIGIN, "nets", 0) for v in idl]
        t_host = time.perf_counter() - t0
        e = entries["nets"]
        gv, gq = e.vertices.cpu().numpy(), e.quads.cpu().numpy()
        for j, r in enumerate(host):
            assert np.array_equal(gq[e.offs[1][j]: e.offs[1][j + 1]], r["quads"]), j
            assert np.array_equal(gv[e.offs[0][j]: e.offs[0][j + 1]].view(np.int32), r["vertices"].view(np.int32)), j
        lattice = sum((b[1] - b[0] + 2) * (b[3] - b[2] + 2) * (b[5] - b[4] + 2) for b in boxes)
        alg = {k: D * S * S + 12 * nv + 16 * nq for k in list(entries) + ["ops_label_mesh_nets"]}
        alg.update(sizes=D * S * S, label_measure_faces=D * S * S)
        frac = {k: alg[k] / t[k] / PEAK_BYTES_PER_S for k in t}
        case = dict(slices=D, size=S, vertices=nv, quads=nq, box_lattice_points=int(lattice), workspace_bytes={k: entries[k].nb for k in entries},
                    seconds=t, algorithmic_bytes=alg, fraction_of_8TBps=frac, ratio_to_label_measure_faces={k: t[k] / t["label_measure_faces"] for k in t},
                    host_copy_s=t_copy, host_total_s=t_host)
        res["cases"].append(case)
        line = (f"{D:2d} x {S}^2, {N_ORGANS} organs, {nv} vertices, {nq} quads, {lattice} lattice points in the boxes: " +
                ", ".join(f"{k} {t[k] * 1e6:8.1f} us ({100 * frac[k]:5.2f} % of 8 TB/s, x{t[k] / t['label_measure_faces']:.2f} label_measure)"
                          for k in names) +
                f"; host copy {t_copy * 1e3:7.1f} ms, copy + numpy restatement (nets) {t_host * 1e3:8.1f} ms (x{t_host / t['nets']:.0f} the entry); "
                "no third-party mesher is installed")
        print(line, flush=True)
        lines.append(line)
    if args.profile:
        lines += kernel_profile(entries["nets_relax3"], lambda: ops.label_mesh_sizes(labels, ids), f"{D} x {S}^2")
        print("\n".join(lines[-9:]), flush=True)
    lines.append(json.dumps(res))
    print(lines[-1])
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
