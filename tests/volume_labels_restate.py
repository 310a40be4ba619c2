"""Float64 numpy restatement of ops.label_slices (csrc/volume_labels.hip), the fixtures its CPU and GPU tests share, and the label / count
rule on its own (`apply_rule`), which the GPU test also applies to ops.bilinear_upsample's output (the composition the kernel replaces).

Semantics per output voxel (t, Y, X): v_o = value of the (H, W) bilinear resize (align_corners=False) of plane (t, o); best_v = label_thr,
best = background; for o = 0 .. n-1: if v_o > best_v: best_v, best = v_o, o; label = ids[best] or 0.  Counts per threshold k and object o:
P = v_o > thr[k] (exclusive: and best == o), G = gt == ids[o]; (|P & G|, |P|, |G|); without gt only |P|.

The source coordinates fy, fx, y0, x0, ly, lx are computed in fp32 exactly as the kernel computes them (one fused multiply-add, emulated
in float64 where the product of two fp32 numbers is exact); the interpolation and every comparison run in float64."""
import numpy as np
import torch

REFERENCE_THRESHOLDS = (0.1, 0.3, 0.5, 0.7, 0.9)
EIGHT_THRESHOLDS = (-1.0, 0.0, 0.1, 0.3, 0.5, 0.7, 0.9, 2.0)
MARGIN = 1e-3          # ten times the fp32 error of one bilinear sample at |v| <= ~18 (4 products and 3 sums of ulp(16)/2 = 1e-6 each, plus the
#                        rounding of the coordinates: |dv| <= |slope| * ulp(lx) ~ 36 * 6e-8 * lw) -- see test_volume_labels_gpu.py item 3
UNDECIDED_CAP = 0.05

# (T, n, (lh, lw), (H, W)) of the bit-equality test; the random-field test uses the first, second, third and fifth
SHAPES = [(3, 3, (16, 16), (37, 53)),       # scalar path, H * W not a multiple of a workgroup's voxels
          (2, 9, (64, 64), (40, 24)),       # down-sampling, W % 4 == 0
          (1, 1, (16, 16), (64, 64)),
          (2, 32, (8, 8), (19, 23)),        # the object limit
          (3, 13, (16, 16), (64, 64)),
          (1, 2, (1, 1), (5, 7)),
          (1, 4, (64, 64), (256, 256))]     # the workload's ratio of 4
RANDOM_FIELD_SHAPES = [SHAPES[0], SHAPES[1], SHAPES[2], SHAPES[4]]
SEEDS = (0, 1, 2)


def random_logits(T, n, lh, lw, seed):
    return torch.randn(T, n, lh, lw, generator=torch.Generator().manual_seed(seed)) * 4


def random_ids(n, seed):
    """n distinct label values in 1 .. 255, not in order"""
    return torch.randperm(255, generator=torch.Generator().manual_seed(100 + seed))[:n].add(1).tolist()


def random_gt(T, H, W, ids, seed):
    """uint8 [T, H, W]: each voxel one of the ids, background or a value that is nobody's id"""
    pool = torch.tensor([0] + list(ids) + [next(v for v in range(1, 256) if v not in ids)], dtype=torch.uint8)
    pick = torch.randint(0, pool.numel(), (T, H, W), generator=torch.Generator().manual_seed(200 + seed))
    return pool[pick]


def dyadic_logits(T, lh, lw, seed):
    """[T, 6, lh, lw] integer logits in -3 .. 3: plane 2 repeats plane 0 and plane 5 repeats plane 3 (ties), plane 4 is all zeros (values at
    exactly label_thr = 0).  Up-sampled by 2 or 4 every weight is a multiple of 1/8, so fp32 and float64 are both exact."""
    x = torch.randint(-3, 4, (T, 6, lh, lw), generator=torch.Generator().manual_seed(300 + seed)).float()
    x[:, 2] = x[:, 0]
    x[:, 5] = x[:, 3]
    x[:, 4] = 0.0
    return x


DYADIC_CASES = [((8, 8), (16, 16)), ((8, 8), (32, 32)), ((16, 16), (64, 64))]
DYADIC_THRESHOLDS = (-2.5, -1.5, -0.5, 0.0, 0.5, 1.5, 2.5)


def f32_thresholds(thresholds):
    """the thresholds as the device compares with them: rounded to fp32 (metrics.seg_counts passes them as an fp32 tensor)"""
    return [float(np.float32(t)) for t in thresholds]


def source_coords(l, L):
    """fp32 source coordinate of every output index 0 .. L-1 of an l -> L resize: (i0, i1, lam) with lam = f - i0 in fp32"""
    s = np.float32(l) / np.float32(L)
    i = np.arange(L, dtype=np.float32) + np.float32(0.5)
    f = np.maximum((i.astype(np.float64) * np.float64(s) - 0.5).astype(np.float32), np.float32(0))   # one rounding: the kernel's fma
    i0 = f.astype(np.int32)
    i1 = np.minimum(i0 + 1, l - 1)
    lam = f - i0.astype(np.float32)
    return i0, i1, lam


def resize64(logits, H, W):
    """float64 [T, n, H, W]: the bilinear resize with fp32 coordinates and float64 interpolation"""
    x = np.asarray(logits, dtype=np.float64)
    lh, lw = x.shape[-2:]
    y0, y1, ly = source_coords(lh, H)
    x0, x1, lx = source_coords(lw, W)
    ly = ly.astype(np.float64)[:, None]
    lx = lx.astype(np.float64)[None, :]
    a, b = x[..., y0[:, None], x0[None, :]], x[..., y0[:, None], x1[None, :]]
    c, d = x[..., y1[:, None], x0[None, :]], x[..., y1[:, None], x1[None, :]]
    return (1 - ly) * ((1 - lx) * a + lx * b) + ly * ((1 - lx) * c + lx * d)


def apply_rule(v, ids, label_thr, thresholds=None, gt=None, exclusive=False):
    """v [T, n, H, W] (any float type; compared as given) -> (labels uint8 [T, H, W], counts int64 [K, T, n, 3] | None, best int [T, H, W])"""
    v = np.asarray(v)
    T, n, H, W = v.shape
    best_v = np.full((T, H, W), label_thr, dtype=v.dtype)
    best = np.full((T, H, W), -1, dtype=np.int64)
    for o in range(n):
        win = v[:, o] > best_v                       # strict; NaN compares false
        best_v = np.where(win, v[:, o], best_v)
        best = np.where(win, o, best)
    table = np.array(list(ids) + [0], dtype=np.uint8)     # index -1 = background
    labels = table[best]
    counts = None
    if thresholds is not None:
        thr = f32_thresholds(thresholds)
        counts = np.zeros((len(thr), T, n, 3), dtype=np.int64)
        for k, t in enumerate(thr):
            for o in range(n):
                P = v[:, o] > v.dtype.type(t)
                if exclusive:
                    P = P & (best == o)
                counts[k, :, o, 1] = P.sum(axis=(1, 2))
                if gt is not None:
                    G = np.asarray(gt) == ids[o]
                    counts[k, :, o, 0] = (P & G).sum(axis=(1, 2))
                    counts[k, :, o, 2] = G.sum(axis=(1, 2))
    return labels, counts, best


def decision_margin(v, label_thr, thresholds=None):
    """float64 [T, H, W]: the smallest of |v_o - thr| over all objects and all thresholds including label_thr, and |v_best - v_second|
    (the two largest values of the voxel): a voxel with a margin above the device's error gets the same label and the same P bits."""
    v = np.asarray(v, dtype=np.float64)
    thr = [float(label_thr)] + (f32_thresholds(thresholds) if thresholds is not None else [])
    with np.errstate(invalid="ignore"):
        d = np.stack([np.abs(v - t) for t in thr])
        m = np.min(np.where(np.isnan(d), np.inf, d), axis=(0, 2))          # a NaN value decides nothing: it never compares true
        if v.shape[1] > 1:
            top = np.sort(np.where(np.isnan(v), -np.inf, v), axis=1)
            gap = top[:, -1] - top[:, -2]
            m = np.minimum(m, np.where(np.isnan(gap), np.inf, gap))
    return m


def restate(logits, ids, H, W, label_thr=0.0, thresholds=None, gt=None, exclusive=False):
    """-> (labels uint8 [T, H, W], counts int64 [K, T, n, 3] | None, margin float64 [T, H, W])"""
    v = resize64(logits, H, W)
    labels, counts, _ = apply_rule(v, ids, label_thr, thresholds, gt, exclusive)
    return labels, counts, decision_margin(v, label_thr, thresholds)
