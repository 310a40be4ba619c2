"""Start of the 3-D path, first step: volume intake on the device.  From the arrays a user holds -- a CT series `int16 [T, H0, W0]` in
Hounsfield units (or decoded 8-bit slices, or float32), and an integer label map `[T, H0, W0]` -- to the model input, the ground-truth
label volume and the prompts, without a host pixel loop.

The path this replaces runs on the host: `data.BTCVVolumes.__getitem__` (`func_3d/dataset/btcv.py:60-104`) opens one image per slice,
`PIL.Image.resize`s it and one boolean mask per (slice, object), stacks a float `[T, 3, S, S]` tensor (805 MB at 64 slices of 1024^2),
`load_video_frames_from_data` uploads and normalises it, `volume_labels.labels_from_pack` rebuilds the label volume mask by mask.  Here the
raw arrays go up as they are (33 MB for 64 int16 slices of 512^2) and `ops.volume_prep` / `ops.label_resize` (csrc/volume_prep.hip) do the
rest.

The contract is exact equality with that host path: Pillow's 8-bit bicubic resize byte for byte (fixed point at 22 fractional bits; the
integer coefficient tables are computed here in float64, the operations of Pillow's `precompute_coeffs` / `normalize_coeffs_8bpc` in their
order, and the kernel only multiplies and adds integers), Pillow's nearest map for the labels, and `(x / 255 - mean) / std` in fp32.  No
Pillow import in this module.

Windows: an int16 / float32 volume needs `window=(lo, hi)` (one CT window replicated to RGB, what `.convert("RGB")` does to a grey slice)
or three pairs (one window per output channel: a multi-window input).  uint8 sources are taken as they are.

Not built: JPEG / NIfTI / DICOM decoding, spacing-aware 3-D resampling, Pillow's other filters, uint16, and the crop of leading / trailing
unlabelled slices (the caller's: `ops.label_stats` gives the per-slice counts)."""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops

F32 = torch.float32
PRECISION_BITS = 32 - 8 - 2                      # Pillow's fixed point for 8-bit images
IMG_MEAN = (0.485, 0.456, 0.406)
IMG_STD = (0.229, 0.224, 0.225)


def resample_tables(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """Pillow's bicubic (a = -0.5, support 2) resampling of `in_size` samples to `out_size`, 8-bit: (coefficients int32 [out_size, ksize],
    bounds int32 [out_size, 2] = (first source sample, tap count)).  numpy float64, the operations of `precompute_coeffs` and
    `normalize_coeffs_8bpc` in their order; the weights of an output are summed left to right (a cumulative sum: np.sum adds pairwise)."""
    in_size, out_size = int(in_size), int(out_size)
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)                      # (int): towards zero, as astype
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    a = np.abs(((x + xmin[:, None]) - center[:, None] + 0.5) * ss)
    w = np.where(a < 1.0, (1.5 * a - 2.5) * a * a + 1, np.where(a < 2.0, (((a - 5) * a + 8) * a - 4) * -0.5, 0.0))
    w = np.where(x < xmax[:, None], w, 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]
    k = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    fixed = k * float(1 << PRECISION_BITS)
    kk = np.where(k < 0, -0.5 + fixed, 0.5 + fixed).astype(np.int64).astype(np.int32)
    return np.ascontiguousarray(kk), np.ascontiguousarray(np.stack([xmin, xmax], axis=1).astype(np.int32))


def nearest_map(in_size: int, out_size: int) -> np.ndarray:
    """Pillow's nearest resize of `in_size` samples to `out_size` (ImagingScaleAffine): int32 [out_size] source index per output, int(xo)
    with xo = 0.5 * in / out advanced by repeated addition of in / out in float64."""
    a = float(in_size) / int(out_size)
    xo = a * 0.5
    m = np.empty(int(out_size), dtype=np.int32)
    for i in range(int(out_size)):
        m[i] = int(xo)
        xo += a
    return m


_TABLES: Dict[tuple, tuple] = {}
_WORKSPACE: Dict[torch.device, torch.Tensor] = {}


def device_tables(H0: int, W0: int, size: int, device) -> tuple:
    """(tables_x | None, tables_y | None, ymap, xmap) of ops.volume_prep / ops.label_resize on `device`, cached per (H0, W0, size, device):
    a second volume of the same shape computes and uploads nothing."""
    device = torch.device(device)
    key = (int(H0), int(W0), int(size), device)
    if key not in _TABLES:
        def up(n):
            return None if n == size else tuple(torch.from_numpy(t).to(device) for t in resample_tables(n, size))
        _TABLES[key] = (up(int(W0)), up(int(H0)), torch.from_numpy(nearest_map(H0, size)).to(device), torch.from_numpy(nearest_map(W0, size)).to(device))
    return _TABLES[key]


def _workspace(nbytes: int, device) -> Optional[torch.Tensor]:
    """grow-only uint8 scratch per device for the two-launch form"""
    if nbytes == 0:
        return None
    ws = _WORKSPACE.get(device)
    if ws is None or ws.numel() < nbytes:
        ws = _WORKSPACE[device] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def _on_device(raw, device, dtypes, what: str) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(raw)) if isinstance(raw, np.ndarray) else raw
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes:
        raise ValueError(f"{what}: a numpy array or tensor of type {' / '.join(str(d).replace('torch.', '') for d in dtypes)} is needed")
    return t.to(device).contiguous()


def _windows(window, dtype) -> Optional[list]:
    if dtype == torch.uint8:
        return None
    if window is None:
        raise ValueError("prepare_volume: an int16 / float32 volume needs window=(lo, hi) or three (lo, hi) pairs")
    w = [tuple(float(v) for v in window)] * 3 if np.ndim(window) == 1 else [tuple(float(v) for v in p) for p in window]
    if len(w) != 3 or any(len(p) != 2 for p in w):
        raise ValueError("prepare_volume: window is (lo, hi) or three (lo, hi) pairs")
    return w


@torch.no_grad()
def prepare_volume(raw, window=None, size: int = 1024, mean=IMG_MEAN, std=IMG_STD, out: Optional[torch.Tensor] = None, grey: bool = False,
                   slices_per_call: int = 16, device="cuda"):
    """raw: [T, H0, W0] or [T, Cin, H0, W0] (Cin 1 or 3), uint8 / int16 / float32, numpy array or tensor (moved to `device` as it is).
    Returns the normalised fp32 [T, 3, size, size] model input on the device -- `load_video_frames_from_data` of the Pillow-resized
    slices, bit for bit -- and with grey=True (frames, greys uint8 [T, 3, size, size]).  out: a tensor to fill in place; with it, a raw
    volume already on the device and warm tables the call allocates no device memory and can be captured into a graph.  The fused form
    takes all slices in one launch; the two-launch form takes `slices_per_call` at a time, so that its workspace is one chunk's."""
    src = _on_device(raw, device, tuple(ops.PREP_SOURCE_TYPES), "prepare_volume")
    if src.dim() == 3:
        src = src.unsqueeze(1)
    if src.dim() != 4 or src.shape[1] not in (1, 3):
        raise ValueError("prepare_volume: raw must be [T, H0, W0] or [T, Cin, H0, W0] with Cin 1 or 3")
    T, _, H0, W0 = src.shape
    S, dev = int(size), src.device
    win = _windows(window, src.dtype)
    tx, ty, _, _ = device_tables(H0, W0, S, dev)
    frames = torch.empty(T, 3, S, S, dtype=F32, device=dev) if out is None else out
    greys = torch.empty(T, 3, S, S, dtype=torch.uint8, device=dev) if grey else None
    step = T if ops.volume_prep_workspace_bytes(T, H0, W0, S) == 0 else max(1, min(int(slices_per_call), T))
    ws = _workspace(ops.volume_prep_workspace_bytes(step, H0, W0, S), dev)
    for i in range(0, T, step):
        j = min(T, i + step)
        ops.volume_prep(src[i:j], S, tx, ty, win, mean, std, out=frames[i:j], grey=greys[i:j] if grey else False, workspace=ws)
    return (frames, greys) if grey else frames


@torch.no_grad()
def prepare_labels(raw_labels, size: int = 1024, obj_ids: Optional[Sequence[int]] = None, device="cuda") -> torch.Tensor:
    """raw_labels: integer label map [T, H0, W0] (uint8 / int16 / int32 / int64), numpy array or tensor -> uint8 [T, size, size] label
    volume on the device: `volume_labels.labels_from_pack` of the dataset's per-object Pillow-nearest masks.  Values outside 1 .. 255, or
    outside obj_ids when given, become 0."""
    src = _on_device(raw_labels, device, tuple(ops.LABEL_SOURCE_TYPES), "prepare_labels")
    if src.dim() != 3:
        raise ValueError("prepare_labels: raw_labels must be [T, H0, W0]")
    _, H0, W0 = src.shape
    _, _, ymap, xmap = device_tables(H0, W0, int(size), src.device)
    return ops.label_resize(src, int(size), ymap, xmap, obj_ids)


@torch.no_grad()
def prepare_case(raw, raw_labels, window=None, size: int = 1024, obj_ids: Optional[Sequence[int]] = None, prompt: str = "bbox",
                 prompt_freq: int = 2, pack: bool = False, seed: Optional[int] = None, variation: float = 0, device="cuda", **prompt_args):
    """One validation / training case from raw arrays: (frames fp32 [T, 3, size, size], labels uint8 [T, size, size], prompts), all from
    the device.  prompts: `prompts.segment_prompts(labels, obj_ids, prompt, prompt_freq, **prompt_args)` -- what `volume.segment_volume`
    and `training_3d.train_step_3d` take -- or, with pack=True, the dictionaries of `data.BTCVVolumes.__getitem__` from
    `prompts.prompts_pack(labels, obj_ids, prompt, prompt_freq, seed, variation)` (bbox, or (pt, p_label)), what `data.validate_volume`
    takes.  obj_ids None: the values 1 .. 255 present in the label volume (one device-to-host copy)."""
    from . import prompts as P
    frames = prepare_volume(raw, window, size, device=device)
    labels = prepare_labels(raw_labels, size, obj_ids, device=device)
    if labels.shape[0] != frames.shape[0]:
        raise ValueError(f"prepare_case: {frames.shape[0]} slices, {labels.shape[0]} label maps")
    if obj_ids is None:
        obj_ids = [int(v) for v in torch.unique(labels).tolist() if v]
    if pack:
        return frames, labels, P.prompts_pack(labels, obj_ids, prompt, prompt_freq=prompt_freq, seed=seed, variation=variation)
    return frames, labels, P.segment_prompts(labels, obj_ids, prompt, prompt_freq=prompt_freq, **prompt_args)
