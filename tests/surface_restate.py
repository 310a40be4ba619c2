"""Host restatement of msam2_label_edt / msam2_label_surface_distances and of volume_labels.surface_scores (helper of the tests, not a test).

surface(): the scipy erosion formula, a unit D squeezed away.  d2(): brute force over the feature coordinates in the defined operation order,
((sx2 dx^2 + sy2 dy^2) + sz2 dz^2) in float64 -- numpy rounds every product and sum on its own.  scores(): np.percentile, np.sum and so on.
Boxes are (z0, z1, y0, y1, x0, x1), inclusive.  The fixtures at the end are shared by tests/test_surface_cpu.py and tests/test_surface_gpu.py."""
import numpy as np
from scipy import ndimage

import components_restate as C

SPACINGS = ((1.0, 1.0, 1.0), (3.0, 0.76, 0.76), (2.5, 0.9, 0.7))


def surface(vol, v):
    """bool mask: voxels equal to v with a face neighbour that differs or lies outside the volume (D == 1: a 2-D image)"""
    mask = np.asarray(vol) == v
    if mask.shape[0] == 1:
        m = mask[0]
        return (m ^ ndimage.binary_erosion(m, ndimage.generate_binary_structure(2, 1), border_value=0))[None]
    return mask ^ ndimage.binary_erosion(mask, ndimage.generate_binary_structure(3, 1), border_value=0)


def whole(shape):
    return (0, shape[0] - 1, 0, shape[1] - 1, 0, shape[2] - 1)


def box_slices(box):
    return (slice(box[0], box[1] + 1), slice(box[2], box[3] + 1), slice(box[4], box[5] + 1))


def in_box(mask, box):
    """the mask with everything outside the box cleared"""
    out = np.zeros_like(mask)
    out[box_slices(box)] = mask[box_slices(box)]
    return out


def d2(queries, feats, spacing):
    """float64 [m]: min over the k features of ((sx2 dx^2 + sy2 dy^2) + sz2 dz^2) for integer coordinates queries [m, 3], feats [k, 3]"""
    sz, sy, sx = (np.float64(s) for s in spacing)
    sz2, sy2, sx2 = sz * sz, sy * sy, sx * sx
    queries, feats = np.asarray(queries).reshape(-1, 3), np.asarray(feats).reshape(-1, 3)
    out = np.full(len(queries), np.inf)
    if len(feats) == 0 or len(queries) == 0:
        return out
    fz, fy, fx = (feats[:, k].astype(np.float64)[None, :] for k in range(3))
    step = max(1, 6_000_000 // len(feats))
    for i in range(0, len(queries), step):
        q = queries[i: i + step].astype(np.float64)
        dz, dy, dx = q[:, 0, None] - fz, q[:, 1, None] - fy, q[:, 2, None] - fx
        out[i: i + step] = ((sx2 * (dx * dx) + sy2 * (dy * dy)) + sz2 * (dz * dz)).min(axis=1)
    return out


def feature_mask(vol, v, features, box):
    return in_box(surface(vol, v) if features == "surface" else np.asarray(vol) != v, box)


def edt(vol, v, spacing, features="surface", box=None):
    """float64 of the box's shape: the dense transform"""
    box = whole(vol.shape) if box is None else box
    f = np.argwhere(feature_mask(vol, v, features, box))
    q = np.argwhere(in_box(np.ones(vol.shape, dtype=bool), box))
    return d2(q, f, spacing).reshape(box[1] - box[0] + 1, box[3] - box[2] + 1, box[5] - box[4] + 1)


def union_box(pred, gt, v):
    """the box of everything equal to v in either volume, or None"""
    at = np.argwhere((np.asarray(pred) == v) | (np.asarray(gt) == v))
    if len(at) == 0:
        return None
    lo, hi = at.min(axis=0), at.max(axis=0)
    return (int(lo[0]), int(hi[0]), int(lo[1]), int(hi[1]), int(lo[2]), int(hi[2]))


def surface_distances(pred, gt, v, spacing, box=None):
    """(sorted d2 of pred's surface voxels to gt's surface, sorted d2 of gt's to pred's), both surfaces cut to the box"""
    box = whole(pred.shape) if box is None else box
    sp, sg = np.argwhere(in_box(surface(pred, v), box)), np.argwhere(in_box(surface(gt, v), box))
    return np.sort(d2(sp, sg, spacing)), np.sort(d2(sg, sp, spacing))


def scores(lists, percentile=95.0, tolerances=(1.0,)):
    """the dict of volume_labels.surface_scores from per-organ (d2_pg, d2_gp) lists"""
    n, K = len(lists), len(tolerances)
    out = {"hd": np.full(n, np.nan), "hd95": np.full(n, np.nan), "assd": np.full(n, np.nan), "nsd": np.full((n, K), np.nan),
           "surface_voxels": np.zeros((n, 2), dtype=np.int64)}
    for j, (a, b) in enumerate(lists):
        a, b = np.sort(np.sqrt(np.asarray(a, dtype=np.float64))), np.sort(np.sqrt(np.asarray(b, dtype=np.float64)))
        out["surface_voxels"][j] = (len(a), len(b))
        if len(a) == 0 or len(b) == 0:
            continue
        out["hd"][j] = max(a.max(), b.max())
        out["hd95"][j] = max(np.percentile(a, percentile), np.percentile(b, percentile))
        out["assd"][j] = (np.sum(a) + np.sum(b)) / (len(a) + len(b))
        out["nsd"][j] = [((a <= t).sum() + (b <= t).sum()) / (len(a) + len(b)) for t in tolerances]
    return out


# ---- fixtures: name -> (pred, gt, ids) ------------------------------------------------------------------------------------------------
def shifted(shape, n, seed):
    """ellipsoid organs with islands (components_restate.ellipsoids) as the ground truth; the prediction is it rolled by (1, 2, 3) (a unit
    axis stays) plus its own islands"""
    gt, ids = C.ellipsoids(shape, n, seed, islands=6)
    pred = np.roll(gt, tuple(s if d > 1 else 0 for s, d in zip((1, 2, 3), shape)), axis=(0, 1, 2))
    rng = np.random.RandomState(seed + 1)
    for v in ids:
        for _ in range(3):
            d, r, c = (rng.randint(0, s) for s in shape)
            pred[d, r: r + rng.randint(1, 3), c: c + rng.randint(1, 5)] = v
    return np.ascontiguousarray(pred), gt, ids


def specials():
    """[9, 33, 100], one id per case:
    40 touches three faces of the volume; 30 has slices and rows without a feature between ones that have some (gt: two plates far apart);
    20 / 21 sit in opposite corners (the pruned scans run their full length); 9 is a single voxel in both; 8 is absent from gt, 7 from pred;
    5: the nearest gt voxel in voxels (one slice away) is not the nearest in millimetres (two columns away) at spacing (3, 0.76, 0.76);
    6: two gt voxels at equal distance left and right, a third as far along y"""
    S = (9, 33, 100)
    pred, gt = np.zeros(S, dtype=np.uint8), np.zeros(S, dtype=np.uint8)
    pred[0:3, 0:5, 0:7] = 40
    gt[0:2, 0:6, 0:9] = 40
    gt[1, 10:12, 20:60] = 30
    gt[7, 25:27, 30:90] = 30
    pred[1:8, 10:27, 40:44] = 30
    pred[0, 32, 98:100] = 20
    gt[8, 0, 96:98] = 20
    pred[8, 30:33, 0:2] = 21
    gt[0:2, 0, 98:100] = 21
    pred[4, 16, 70] = gt[5, 18, 75] = 9
    pred[3, 20:22, 64:70] = 8
    gt[6, 5:7, 62:66] = 7
    pred[4, 29, 50] = 5
    gt[5, 29, 50] = gt[4, 29, 52] = 5
    pred[2, 6, 80] = 6
    gt[2, 6, 77] = gt[2, 6, 83] = gt[2, 3, 80] = 6
    return pred, gt, [40, 9, 30, 5, 21, 20, 8, 7, 6]


def wide():
    """[9, 33, 100]: one organ (77) that spans columns 18 .. 98, so rows carry across the 64-column chunks, with a hollow and a second value
    (3) inside; the prediction is it rolled by (1, 2, 3) plus islands"""
    S = (9, 33, 100)
    z, y, x = np.indices(S)
    r = ((z - 4) / 3.2) ** 2 + ((y - 15.5) / 9.0) ** 2 + ((x - 58) / 40.5) ** 2
    gt = np.zeros(S, dtype=np.uint8)
    gt[r <= 1.0] = 77
    gt[4, 14:17, 50:75] = 0
    gt[3:6, 10:13, 30:40] = 3
    pred = np.roll(gt, (1, 2, 3), axis=(0, 1, 2))
    pred[0, 1, 5:8] = pred[8, 30:32, 60:66] = 77
    pred[2, 2, 90] = 3
    return np.ascontiguousarray(pred), gt, [77, 3]


def every_voxel_surface(shape, seed):
    """noise of three values on a volume of two rows: every voxel touches the border"""
    return C.noise(shape, 3, seed), C.noise(shape, 3, seed + 1), [2, 1]


def cases():
    yield "specials_9x33x100", specials()
    yield "wide_9x33x100", wide()
    yield "shifted3_9x33x100", shifted((9, 33, 100), 3, 31)
    yield "shifted32_9x33x100", shifted((9, 33, 100), 32, 14)
    yield "shifted1_1x12x66", shifted((1, 12, 66), 1, 33)
    yield "shifted3_1x12x66", shifted((1, 12, 66), 3, 36)
    yield "noise_3x2x65", every_voxel_surface((3, 2, 65), 40)
    yield "noise_4x9x70", (C.noise((4, 9, 70), 4, 20), C.noise((4, 9, 70), 4, 21), [3, 1, 2])
