#!/usr/bin/env python3
"""Volume intake at the workload's sizes: 64 and 8 slices of int16 512^2 -> 1024^2 (one CT window) and of uint8 1024^2 -> 1024^2 (identity).

- `volume_prep.prepare_volume` with the raw volume on the device and `out=` given, in the fused form and in the two-launch form
  (MSAM2_VOLUME_PREP_FUSED=1 / 0): one launch, and 16 slices per launch pair;
- the path it replaces, on the same box: Pillow `convert("RGB").resize` per slice (from the windowed 8-bit slices: the window itself is
  not counted), the float [T, 3, S, S] stack, its upload and `load_video_frames_from_data` (wall clock, one run after one warm-up);
- the achieved fraction of 8 TB/s on the bytes written, T 3 S S 4 (the input is 1 / 24 of that or less).

HIP events around `reps` back-to-back calls, the median of `rounds` such windows, the two device arms alternating.  Prints one line per
case and a JSON line at the end; asserts that both forms and the host path give the same bits, nothing about time."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import medical_sam2_amd.volume_prep as vp  # noqa: E402
from medical_sam2_amd.video_predictor import load_video_frames_from_data  # noqa: E402

S = 1024
PEAK_BYTES_PER_S = 8e12
SWITCH = "MSAM2_VOLUME_PREP_FUSED"
CT = (-160, 240)


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def medians(fns, reps=5, rounds=7, warm=2):
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


def ct_series(T, side, seed):
    """int16 [T, side, side]: a body-like disc of soft tissue with organs and bone in air, in Hounsfield units, with noise"""
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:side, 0:side].astype(np.float32) / side - 0.5
    vol = np.full((T, side, side), -1000, dtype=np.int16)
    for t in range(T):
        r = np.sqrt((xs * 1.1) ** 2 + (ys * 1.4) ** 2)
        hu = np.where(r < 0.45, 40.0, -1000.0) + np.where(r < 0.1 + 0.002 * t, 90.0, 0.0) + np.where(np.abs(r - 0.4) < 0.01, 700.0, 0.0)
        vol[t] = (hu + rng.randn(side, side) * 20.0).astype(np.int16)
    return vol


def host_path(greys8):
    """the replaced path from 8-bit slices [T, H0, W0]: seconds (resize + stack, upload + normalise) and the frames on the device"""
    from PIL import Image
    t0 = time.perf_counter()
    img = torch.zeros(greys8.shape[0], 3, S, S)
    for t in range(greys8.shape[0]):
        img[t] = torch.tensor(np.array(Image.fromarray(greys8[t]).convert("RGB").resize((S, S)))).permute(2, 0, 1)
    t1 = time.perf_counter()
    frames = load_video_frames_from_data(img)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, frames


def timed(fn, form):
    def run():
        os.environ[SWITCH] = form
        fn()
    return run


def main():
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    res = {"size": S, "cases": []}
    for T in (64, 8):
        for name in ("int16_512", "uint8_1024"):
            if name == "int16_512":
                raw = ct_series(T, 512, T)
                h = np.clip(raw.astype(np.int32), *CT)
                greys8 = ((510 * (h - CT[0]) + (CT[1] - CT[0])) // (2 * (CT[1] - CT[0]))).astype(np.uint8)
                win = CT
            else:
                raw = greys8 = np.random.RandomState(T).randint(0, 256, (T, S, S)).astype(np.uint8)
                win = None
            src = torch.from_numpy(raw).to(dev)
            out = torch.empty(T, 3, S, S, dtype=torch.float32, device=dev)
            call = lambda: vp.prepare_volume(src, window=win, size=S, out=out)  # noqa: E731
            t_fused, t_two = medians([timed(call, "1"), timed(call, "0")])
            bits = {}
            for form in ("1", "0"):
                out.fill_(float("nan"))
                timed(call, form)()
                bits[form] = out.view(torch.int32).clone()
            os.environ.pop(SWITCH, None)
            assert torch.equal(bits["1"], bits["0"]), "the fused and the two-launch form differ"
            host_path(greys8[:1])                                            # warm-up (allocator, Pillow)
            h_resize, h_upload, frames = host_path(greys8)
            assert torch.equal(frames.view(torch.int32), bits["1"]), "device and host frames differ"
            del frames, bits
            written = T * 3 * S * S * 4
            case = dict(slices=T, source=name, raw_bytes=int(raw.nbytes), written_bytes=written, fused_s=t_fused, two_launch_s=t_two,
                        fused_fraction_of_8TBps=written / t_fused / PEAK_BYTES_PER_S, two_launch_fraction_of_8TBps=written / t_two / PEAK_BYTES_PER_S,
                        host_resize_stack_s=h_resize, host_upload_normalise_s=h_upload)
            res["cases"].append(case)
            print(f"{T:2d} slices {name:10s}: fused {t_fused * 1e6:8.1f} us ({100 * case['fused_fraction_of_8TBps']:.1f} % of 8 TB/s written), "
                  f"two launches {t_two * 1e6:8.1f} us ({100 * case['two_launch_fraction_of_8TBps']:.1f} %); host Pillow resize + stack "
                  f"{h_resize * 1e3:7.1f} ms, upload + normalise {h_upload * 1e3:7.1f} ms (x{(h_resize + h_upload) / t_fused:.0f})")
            del src, out
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
