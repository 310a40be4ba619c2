"""Plain-numpy restatement of the volume intake (csrc/volume_prep.hip, medical_sam2_amd/volume_prep.py): the arbiter of the GPU tests.

It restates Pillow's 8-bit resampling (src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc
/ Vertical_8bpc with the bicubic filter, a = -0.5, support 2), Pillow's nearest map (Geometry.c: ImagingScaleAffine), the three window
rules and the fp32 normalisation of `load_video_frames_from_data`, each as the loop the C code runs, nothing vectorised across the
roundings.  tests/test_volume_prep_cpu.py ties it to Pillow itself, to the committed Pillow outputs of tests/golden/volume_prep_pillow.npz
and to `data.BTCVVolumes`; no product code is imported here."""
import math
from fractions import Fraction

import numpy as np

PRECISION_BITS = 32 - 8 - 2
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
# (H0, W0, S): the size pairs the contract was checked on
PAIRS = [(37, 53, 64), (64, 64, 64), (100, 130, 64), (512, 512, 1024), (33, 64, 64), (64, 17, 32), (300, 200, 128), (7, 5, 64), (191, 257, 96),
         (700, 300, 16)]


def bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def resample_tables(in_size: int, out_size: int):
    """(coefficients int32 [out, ksize], bounds int32 [out, 2] = (first source index, tap count)) of one axis"""
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return kk, bounds


def _pass(img: np.ndarray, kk: np.ndarray, bounds: np.ndarray) -> np.ndarray:
    """one pass along the LAST axis of uint8 [..., n] -> uint8 [..., out]; int32 accumulator, as Pillow's `int ss`"""
    out = np.empty(img.shape[:-1] + (kk.shape[0],), dtype=np.uint8)
    src = img.astype(np.int32)
    for xx in range(kk.shape[0]):
        xmin, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        ss = np.full(img.shape[:-1], 1 << (PRECISION_BITS - 1), dtype=np.int32)
        for x in range(n):
            ss = ss + src[..., xmin + x] * kk[xx, x]
        out[..., xx] = np.clip(ss >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def resize_bicubic(img: np.ndarray, size: int, passes: bool = False):
    """uint8 [..., H0, W0] -> uint8 [..., size, size]: horizontal pass, then vertical, each skipped when its dimension is already `size`.
    passes=True also returns the image between the two passes [..., H0, size]."""
    H0, W0 = img.shape[-2:]
    mid = img if W0 == size else _pass(img, *resample_tables(W0, size))
    out = mid if H0 == size else np.swapaxes(_pass(np.ascontiguousarray(np.swapaxes(mid, -1, -2)), *resample_tables(H0, size)), -1, -2)
    out = np.ascontiguousarray(out)
    return (out, np.ascontiguousarray(mid)) if passes else out


def nearest_map(in_size: int, out_size: int) -> np.ndarray:
    a = float(in_size) / out_size
    xo = a * 0.5
    m = np.empty(out_size, dtype=np.int32)
    for x in range(out_size):
        m[x] = int(xo)
        xo += a
    return m


def resize_nearest(img: np.ndarray, size: int) -> np.ndarray:
    """[..., H0, W0] -> [..., size, size], any dtype"""
    H0, W0 = img.shape[-2:]
    return np.ascontiguousarray(img[..., nearest_map(H0, size), :][..., nearest_map(W0, size)])


def window_i16(v, lo: int, hi: int) -> np.ndarray:
    h = np.clip(np.asarray(v).astype(np.int32), lo, hi)
    return ((510 * (h - lo) + (hi - lo)) // (2 * (hi - lo))).astype(np.uint8)


def window_i16_exact(v: int, lo: int, hi: int) -> int:
    """floor(255 (clamp(v) - lo) / (hi - lo) + 1/2) in rational arithmetic"""
    h = min(max(int(v), lo), hi)
    return math.floor(Fraction(255 * (h - lo), hi - lo) + Fraction(1, 2))


def window_f32(v, lo: float, hi: float) -> np.ndarray:
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        t = np.clip(v.astype(np.float64), np.float64(lo), np.float64(hi))
        g = np.floor(((t - np.float64(lo)) * np.float64(255.0)) / (np.float64(hi) - np.float64(lo)) + np.float64(0.5))
    return np.where(np.isnan(v), 0.0, g).astype(np.uint8)


def window(raw: np.ndarray, lo, hi) -> np.ndarray:
    if raw.dtype == np.uint8:
        return raw
    return window_i16(raw, int(lo), int(hi)) if raw.dtype == np.int16 else window_f32(raw, lo, hi)


def greys(raw: np.ndarray, windows, size: int) -> np.ndarray:
    """raw [T, Cin, H0, W0] (uint8 / int16 / float32), windows: three (lo, hi) -> uint8 [T, 3, size, size]: channel c = plane c % Cin, window c"""
    Cin = raw.shape[1]
    windows = [(None, None)] * 3 if windows is None else windows          # (uint8 needs none)
    return np.stack([resize_bicubic(window(raw[:, c % Cin], *windows[c]), size) for c in range(3)], axis=1)


def normalise(g: np.ndarray, mean=MEAN, std=STD) -> np.ndarray:
    """uint8 [T, 3, S, S] -> fp32: (x / 255 - mean) / std, every operation in fp32 (video_predictor.load_video_frames_from_data)"""
    m = np.asarray(mean, dtype=np.float32)[:, None, None]
    s = np.asarray(std, dtype=np.float32)[:, None, None]
    return ((g.astype(np.float32) / np.float32(255.0) - m) / s).astype(np.float32)


def labels(raw: np.ndarray, size: int, keep=None) -> np.ndarray:
    """integer [T, H0, W0] -> uint8 [T, size, size]: the nearest gather, values outside 1 .. 255 or outside `keep` -> 0"""
    r = resize_nearest(raw, size).astype(np.int64)
    ok = (r >= 1) & (r <= 255)
    if keep is not None:
        ok &= np.isin(r, np.asarray(list(keep), dtype=np.int64))
    return np.where(ok, r, 0).astype(np.uint8)


def sample_image(H0: int, W0: int, seed: int, noise: float = 25.0) -> np.ndarray:
    """uint8 [H0, W0]: smooth structure plus noise plus saturated patches (overshoot of the negative lobes, clipped at both ends)"""
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:H0, 0:W0]
    img = 127.0 + 90.0 * np.sin(xs / 3.1 + seed) * np.cos(ys / 4.3) + rng.randn(H0, W0) * noise
    img = np.clip(img, 0, 255).astype(np.uint8)
    img[: max(1, H0 // 5), : max(1, W0 // 4)] = 255
    img[-max(1, H0 // 6):, -max(1, W0 // 5):] = 0
    img[H0 // 2, :] = rng.randint(0, 2, W0) * 255
    return img
