#!/usr/bin/env python3
"""Per-organ measurements at the workload's sizes: 8 and 64 slices of 512^2 and of 1024^2, 13 organs, a synthetic int16 image.

- `ops.label_measure` with caller-owned tables (no allocation in the window) in four forms: geometry only; with the image; with the image
  and a 4096-bin histogram; with the image, the histogram and the faces (what `organ_measurements` runs);
- `ops.label_stats` on the same labels: the yardstick for a one-pass label kernel that is launch- and atomics-bound at this size;
- the host alternative on the same box: the two device-to-host copies plus the per-organ numpy reductions of the restatement's fast path
  (tests/measure_restate.host_alternative: no faces), wall clock, once;
- the achieved fraction of 8 TB/s on the algorithmic bytes: one read of the labels, D H W, plus 2 bytes per organ voxel for the forms that
  read the image.

HIP events around `reps` back-to-back calls, the median of `rounds` such windows, the device arms alternating.  Prints one line per case
and a JSON line at the end; asserts that the device tables equal the host alternative's figures, nothing about time.  --out FILE also writes
the lines there."""
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
import measure_restate as R  # noqa: E402

import medical_sam2_amd.ops as ops  # noqa: E402

N_ORGANS = 13
LO, BINS = -1024, 4096
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


def organs(D, S, n, seed):
    """uint8 [D, S, S]: n ellipsoids labelled 1 .. n, each cutting about half of the slices (the label volumes of the other benches)"""
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


def hounsfield(vol, seed):
    """int16: air outside, a soft-tissue mean per organ, Gaussian noise of 30 HU everywhere"""
    rng = np.random.RandomState(seed)
    means = np.concatenate([[-1000.0], 20.0 + 15.0 * np.arange(N_ORGANS), np.zeros(255 - N_ORGANS)])
    img = means[vol]
    for d in range(vol.shape[0]):
        img[d] += rng.normal(0.0, 30.0, vol.shape[1:])
    return np.clip(np.rint(img), -32768, 32767).astype(np.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--slices", default="8,64")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "measure_bench needs the MI355X"
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    res, lines = {"organs": N_ORGANS, "hist": [LO, BINS], "cases": []}, []
    idl = list(range(1, N_ORGANS + 1))
    for S in (int(s) for s in args.sizes.split(",")):
        for D in (int(d) for d in args.slices.split(",")):
            vol = organs(D, S, N_ORGANS, 10 * D + S)
            image = hounsfield(vol, D + S)
            labels, img = torch.from_numpy(vol).to(dev), torch.from_numpy(image).to(dev)
            ids = ops.label_ids(idl, dev)
            rows = torch.empty(D, N_ORGANS, S, dtype=torch.int32, device=dev)
            forms = {"geometry": dict(faces=False), "image": dict(image=img, hist_lo=LO, faces=False),
                     "hist": dict(image=img, hist_lo=LO, bins=BINS, faces=False), "hist_faces": dict(image=img, hist_lo=LO, bins=BINS, faces=True)}
            outs = {k: ops.label_measure(labels, ids, **kw) for k, kw in forms.items()}
            fns = [lambda k=k, kw=kw: ops.label_measure(labels, ids, out=outs[k], **kw) for k, kw in forms.items()]
            fns.append(lambda: ops.label_stats(labels, ids, rows=rows))
            t = dict(zip(list(forms) + ["label_stats"], medians(fns)))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hv, hi = labels.cpu().numpy(), img.cpu().numpy()
            t_copy = time.perf_counter() - t0
            host = R.host_alternative(hv, idl, hi, LO, BINS)
            t_host = time.perf_counter() - t0
            m, _, v, _, h = (x.cpu().numpy() for x in outs["hist_faces"])
            for j, (geometry, sv, svv, vmin, vmax, hh) in enumerate(host):
                assert m[j, :10].tolist() == geometry and (m[j, 10], m[j, 11]) == (sv, svv) and v[j].tolist() == [vmin, vmax], j
                assert np.array_equal(h[j], hh), j
            assert torch.equal(outs["geometry"][0][:, :10], outs["hist_faces"][0][:, :10])
            organ_voxels = int(m[:, 0].sum())
            alg = {"geometry": D * S * S, "label_stats": D * S * S}
            alg.update({k: D * S * S + 2 * organ_voxels for k in ("image", "hist", "hist_faces")})
            frac = {k: alg[k] / t[k] / PEAK_BYTES_PER_S for k in t}
            case = dict(slices=D, size=S, organ_voxels=organ_voxels, seconds=t, algorithmic_bytes=alg, fraction_of_8TBps=frac,
                        ratio_to_label_stats={k: t[k] / t["label_stats"] for k in forms}, host_copy_s=t_copy, host_total_s=t_host)
            res["cases"].append(case)
            line = (f"{D:2d} x {S}^2 ({100.0 * organ_voxels / (D * S * S):4.1f} % organ voxels): " +
                    ", ".join(f"{k} {t[k] * 1e6:7.1f} us ({100 * frac[k]:4.1f} % of 8 TB/s, x{t[k] / t['label_stats']:.2f} label_stats)" for k in forms) +
                    f"; label_stats {t['label_stats'] * 1e6:7.1f} us ({100 * frac['label_stats']:4.1f} %); host copies {t_copy * 1e3:7.1f} ms, "
                    f"copies + numpy {t_host * 1e3:8.1f} ms (x{t_host / t['hist_faces']:.0f} the full form)")
            print(line, flush=True)
            lines.append(line)
    lines.append(json.dumps(res))
    print(lines[-1])
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
