#!/usr/bin/env python3
"""Instance tables and scores at the workload's sizes: 8 slices of 512^2 and 64 slices of 1024^2 with about 500 instances per map.

- `ops.instance_remap` of the ground-truth map (random non-contiguous ids) with caller-owned tables;
- `ops.instance_pairs` of the two remapped maps with caller-owned tables and workspace (no allocation in the window);
- the whole `instances.instance_scores`: two remaps, the pairs, the one device-to-host copy and the host scores, wall clock;
- the host alternative on the same box: the two device-to-host copies of the maps, then the numpy restatement of the tests
  (tests/instances_restate.host_alternative: np.unique with the inverse for the remaps, np.unique on combined keys, np.bincount) and the
  same host scores, wall clock, once.  The reference's own functions (one boolean mask per instance, three times over) are not timed.

HIP events around `reps` back-to-back calls, the median of `rounds` such windows.  Prints one line per case and a JSON line at the end;
asserts that the device tables equal the host alternative's, nothing about time.  --out FILE also writes the lines there."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import instances_restate as R  # noqa: E402

import medical_sam2_amd.instances as I  # noqa: E402
import medical_sam2_amd.ops as ops  # noqa: E402

N_INSTANCES = 500
CAP = 1024


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def median(fn, reps=10, rounds=7, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    return float(np.median([window(fn, reps) for _ in range(rounds)]))


def balls(D, S, n, seed):
    """int32 [D, S, S]: n balls with random distinct ids below 10^6, later ones overwrite earlier ones"""
    rng = np.random.RandomState(seed)
    vol = np.zeros((D, S, S), dtype=np.int32)
    ids = rng.choice(np.arange(1, 1_000_000), n, replace=False)
    for k in range(n):
        r = int(rng.uniform(0.012, 0.03) * S)
        rz = max(1, min(r, D // 3))
        cz, cy, cx = rng.randint(0, D), rng.randint(r, S - r), rng.randint(r, S - r)
        z0, z1 = max(0, cz - rz), min(D, cz + rz + 1)
        zz, yy, xx = np.ogrid[z0 - cz: z1 - cz, -r: r + 1, -r: r + 1]
        inside = (zz / rz) ** 2 + (yy / r) ** 2 + (xx / r) ** 2 <= 1.0
        box = vol[z0:z1, cy - r: cy + r + 1, cx - r: cx + r + 1]
        box[inside] = ids[k]
    return vol


def prediction(true):
    """the truth shifted by 2 columns and 1 row, every seventh id missing, the ids inside one corner block merged"""
    pred = np.roll(true, (1, 2), axis=(1, 2))
    pred[pred % 7 == 0] = 0
    corner = pred[:, : true.shape[1] // 4, : true.shape[2] // 4]
    corner[corner > 0] = 1_000_001
    return pred


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="8x512,64x1024")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "instances_bench needs the MI355X"
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    res, lines = {"instances": N_INSTANCES, "cases": []}, []
    for D, S in (tuple(int(v) for v in c.split("x")) for c in args.cases.split(",")):
        true_h = balls(D, S, N_INSTANCES, D + S)
        pred_h = prediction(true_h)
        true, pred = torch.from_numpy(true_h).to(dev), torch.from_numpy(pred_h).to(dev)
        bound = 1_000_002
        rt = ops.instance_remap(true, bound, CAP)
        rp = ops.instance_remap(pred, bound, CAP)
        ws = ops.instance_pairs_workspace(CAP, 4 * CAP, dev)
        tabs = ops.instance_pairs(rt[0], rp[0], CAP, CAP, 4 * CAP, workspace=ws)
        t_remap = median(lambda: ops.instance_remap(true, bound, CAP, out=rt))
        t_pairs = median(lambda: ops.instance_pairs(rt[0], rp[0], CAP, CAP, 4 * CAP, out=tabs, workspace=ws))
        torch.cuda.synchronize()
        walls = []
        for _ in range(5):
            t0 = time.perf_counter()
            got = I.instance_scores(true, pred, max_instances=CAP)
            walls.append(time.perf_counter() - t0)
        t_scores = float(np.median(walls))
        t0 = time.perf_counter()
        th, ph = true.cpu().numpy(), pred.cpu().numpy()
        t_copy = time.perf_counter() - t0
        rows, at, ap_ = R.host_alternative(th, ph)
        t_tables = time.perf_counter() - t0
        want = I.instance_scores_from_tables(rows, at, ap_)
        t_host = time.perf_counter() - t0
        n_rows = int(tabs[3][0])
        assert n_rows == len(rows) and np.array_equal(tabs[0][:n_rows].cpu().numpy(), rows)
        assert np.array_equal(tabs[1].cpu().numpy()[: len(at)], at) and np.array_equal(tabs[2].cpu().numpy()[: len(ap_)], ap_)
        assert all(got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])) for k in I.SCORE_KEYS) and got["paired_true"] == want["paired_true"]
        case = dict(slices=D, size=S, true_instances=len(at), pred_instances=len(ap_), pairs=len(rows), remap_s=t_remap, pairs_s=t_pairs,
                    instance_scores_wall_s=t_scores, host_copy_s=t_copy, host_tables_s=t_tables, host_total_s=t_host, pq=got["pq"], aji=got["aji"])
        res["cases"].append(case)
        line = (f"{D:2d} x {S}^2, {len(at)} true / {len(ap_)} predicted instances, {len(rows)} pairs: remap {t_remap * 1e6:8.1f} us, pairs "
                f"{t_pairs * 1e6:8.1f} us, instance_scores (two remaps, pairs, one copy, host scores; wall) {t_scores * 1e3:7.2f} ms; host: copies "
                f"{t_copy * 1e3:7.1f} ms, copies + numpy tables {t_tables * 1e3:9.1f} ms, + scores {t_host * 1e3:9.1f} ms "
                f"(x{t_host / t_scores:.0f} instance_scores)")
        print(line, flush=True)
        lines.append(line)
    lines.append(json.dumps(res))
    print(lines[-1])
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
