"""Brute-force restatement of msam2_label_measure (csrc/measure.hip) with numpy and Python integers: one boolean mask per organ, np.nonzero
for the coordinate sums, shifted comparisons for the faces, np.bincount on the clipped range for the histogram, np.sort plus the definition
for the percentiles.  No code is shared with the package."""
import numpy as np

INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


def tables(vol, ids, image=None, hist_lo=0, bins=0):
    """-> dict(moments int64 [n, 14], extent int64 [n, 6], vrange int64 [n, 2], faces int64 [n, 6], hist int64 [n, bins])"""
    D, H, W = vol.shape
    n = len(ids)
    moments = np.zeros((n, 14), dtype=np.int64)
    extent = np.full((n, 6), -1, dtype=np.int64)
    vrange = np.tile(np.array([INT32_MAX, INT32_MIN], dtype=np.int64), (n, 1))
    faces = np.zeros((n, 6), dtype=np.int64)
    hist = np.zeros((n, bins), dtype=np.int64)
    for j, v in enumerate(ids):
        m = vol == v
        z, y, x = (c.astype(np.int64) for c in np.nonzero(m))
        count = len(z)
        row = [count] + [int(c.sum()) for c in (z, y, x, z * z, y * y, x * x, z * y, z * x, y * x)] + [0, 0, 0, 0]
        if count:
            extent[j] = [z.min(), z.max(), y.min(), y.max(), x.min(), x.max()]
        for axis in range(3):
            a = np.moveaxis(m, axis, 0)
            faces[j, axis] = int((a[1:] != a[:-1]).sum())
            faces[j, 3 + axis] = int(a[0].sum()) + int(a[-1].sum())
        if image is not None and count:
            val = image[m].astype(np.int64)
            below, above = int((val < hist_lo).sum()), int((val >= hist_lo + bins).sum())
            row[10:14] = [int(val.sum()), int((val * val).sum()), below, above]      # int64: |v| <= 2^15 and fewer than 2^31 voxels
            vrange[j] = [val.min(), val.max()]
            if bins:
                inside = val[(val >= hist_lo) & (val < hist_lo + bins)] - hist_lo
                hist[j] = np.bincount(inside, minlength=bins)
        moments[j] = row
    return dict(moments=moments, extent=extent, vrange=vrange, faces=faces, hist=hist)


def host_alternative(vol, ids, image, hist_lo, bins):
    """what a user runs on the host today (the fast path of the above: no faces, no clipped counts): tools/measure_bench.py times it.
    -> per organ (the ten geometry columns, Sv, Svv, min, max, histogram)"""
    out = []
    for v in ids:
        m = vol == v
        z, y, x = (c.astype(np.int64) for c in np.nonzero(m))
        geometry = [len(z)] + [int(c.sum()) for c in (z, y, x, z * z, y * y, x * x, z * y, z * x, y * x)]
        val = image[m].astype(np.int64)
        inside = val[(val >= hist_lo) & (val < hist_lo + bins)] - hist_lo
        out.append((geometry, int(val.sum()), int((val * val).sum()), int(val.min()) if len(val) else INT32_MAX,
                    int(val.max()) if len(val) else INT32_MIN, np.bincount(inside, minlength=bins)))
    return out


def order_statistics(vol, v, image, qs):
    """numpy's "linear" percentile of the values under vol == v, spelled out: -> (percentiles [len(qs)], order statistics [len(qs), 2])"""
    val = np.sort(image[vol == v].astype(np.int64))
    c = len(val)
    out, pair = [], []
    for q in qs:
        pos = (c - 1) * (float(q) / 100.0)
        lo = int(np.floor(pos))
        hi = min(lo + 1, c - 1)
        a, b, t = float(val[lo]), float(val[hi]), pos - lo
        pair.append((a, b))
        out.append(a + (b - a) * t if t < 0.5 else b - (b - a) * (1.0 - t))
    return np.array(out), np.array(pair)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------------
def blobs(shape, n, seed, absent=True):
    """ellipsoids of n organs (later ones cover earlier ones: organs touch) plus one value that is nobody's id; ids include 255; with
    `absent` the last listed id is 0xAB and has no voxel (the GPU tests pad the volume with 0xAB: an over-read would give it some).
    Radii up to half the volume, centres anywhere: organs touch every frame."""
    D, H, W = shape
    rng = np.random.RandomState(seed)
    pool = [v for v in range(2, 255) if v != 0xAB]                        # 1 is the stray value
    ids = [255] + [pool[i] for i in rng.permutation(len(pool))[: n - 1]]
    if absent and n > 1:
        ids[-1] = 0xAB
    zs, ys, xs = np.mgrid[0:D, 0:H, 0:W]
    vol = np.zeros(shape, dtype=np.uint8)
    drawn = ids[:-1] if absent and n > 1 else ids
    for v in drawn + [1]:
        cz, cy, cx = rng.uniform(0, D), rng.uniform(0, H), rng.uniform(0, W)
        rz, ry, rx = rng.uniform(0.6, max(D / 2, 1)), rng.uniform(0.6, max(H / 2, 1)), rng.uniform(0.6, max(W / 2, 1))
        vol[((zs - cz) / rz) ** 2 + ((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2 <= 1.0] = v
    return vol, ids


def hu_image(shape, seed, lo, bins):
    """int16: a smooth ramp plus noise around the histogram range, with the range's two ends, one below, one above and the type's two
    extremes planted everywhere (so that every organ of a blob fixture is likely to hold some of them)"""
    rng = np.random.RandomState(seed)
    D, H, W = shape
    ramp = np.add.outer(np.add.outer(np.arange(D) * 7, np.arange(H) * 3), np.arange(W))
    img = (lo + (ramp + rng.randint(0, max(bins, 2), shape)) % max(bins, 1)).astype(np.int64)
    special = np.array([lo, lo + bins - 1, lo - 1, lo + bins, -32768, 32767], dtype=np.int64)
    where = rng.randint(0, 5, shape) == 0
    img[where] = special[rng.randint(0, len(special), int(where.sum()))]
    img[img == 23456] = 23457                                            # IMAGE_PAD below
    return np.clip(img, -32768, 32767).astype(np.int16)


IMAGE_PAD = {np.dtype(np.int16): 23456, np.dtype(np.uint8): 0xEE}        # no fixture image holds these: the GPU tests pad with them


def grey_image(shape, seed):
    img = np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)
    img[img == 0xEE] = 0xEF
    return img
