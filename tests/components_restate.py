"""Host restatement of msam2_label_components / msam2_label_clean / msam2_label_overlap (helper of the tests, not a test).

restate() is scipy.ndimage.label once per distinct value; the canonical name of a component is 1 + the smallest linear index of its voxels
(np.minimum.at), its size the bincount of its voxels, stored at that smallest voxel.  clean() and overlap() are plain numpy.  Everything is
int64 numpy.  flood() is an independent pure-numpy flood fill that restate() itself is checked against on tiny volumes."""
import itertools

import numpy as np
from scipy import ndimage

CONNECTIVITIES = (4, 8, 6, 18, 26)


def structure(connectivity):
    if connectivity in (6, 18, 26):
        return ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])
    s = np.zeros((3, 3, 3), dtype=bool)
    s[1] = ndimage.generate_binary_structure(2, {4: 1, 8: 2}[connectivity])      # the d = +-1 planes are empty: slice by slice
    return s


def offsets(connectivity):
    return [tuple(int(x) - 1 for x in o) for o in np.argwhere(structure(connectivity)) if tuple(o) != (1, 1, 1)]


def restate(vol, connectivity):
    """(comp, size) int64 [D, H, W] of a uint8 volume"""
    vol = np.asarray(vol)
    comp = np.zeros(vol.shape, dtype=np.int64)
    size = np.zeros(vol.shape, dtype=np.int64)
    lin = np.arange(vol.size, dtype=np.int64).reshape(vol.shape)
    st = structure(connectivity)
    for v in np.unique(vol):
        if v == 0:
            continue
        lab, k = ndimage.label(vol == v, structure=st)
        m = lab > 0
        first = np.full(k + 1, vol.size, dtype=np.int64)
        np.minimum.at(first, lab[m], lin[m])
        comp[m] = first[lab[m]] + 1
        count = np.bincount(lab[m], minlength=k + 1)
        size.reshape(-1)[first[1:]] = count[1:]
    return comp, size


def flood(vol, connectivity):
    """the same two tables from a stack-based flood fill in raster order (tiny volumes only)"""
    vol = np.asarray(vol)
    D, H, W = vol.shape
    offs = offsets(connectivity)
    comp = np.zeros(vol.shape, dtype=np.int64)
    size = np.zeros(vol.shape, dtype=np.int64)
    for d, r, c in itertools.product(range(D), range(H), range(W)):
        if vol[d, r, c] == 0 or comp[d, r, c]:
            continue
        name = (d * H + r) * W + c + 1                       # raster order: the first voxel met is the smallest
        comp[d, r, c] = name
        stack, count = [(d, r, c)], 0
        while stack:
            z, y, x = stack.pop()
            count += 1
            for dz, dy, dx in offs:
                a, b, e = z + dz, y + dy, x + dx
                if 0 <= a < D and 0 <= b < H and 0 <= e < W and vol[a, b, e] == vol[d, r, c] and not comp[a, b, e]:
                    comp[a, b, e] = name
                    stack.append((a, b, e))
        size[d, r, c] = count
    return comp, size


def clean(vol, comp, size, ids, min_voxels=None, largest_mask=0):
    """(out uint8 like vol, info int64 [n, 6]): the rule of msam2_label_clean"""
    vol = np.asarray(vol)
    comp, size = np.asarray(comp, dtype=np.int64), np.asarray(size, dtype=np.int64)
    out = vol.copy()
    info = np.zeros((len(ids), 6), dtype=np.int64)
    flat_vol, flat_size = vol.reshape(-1), size.reshape(-1)
    for j, v in enumerate(ids):
        need = max(1, 0 if min_voxels is None else int(min_voxels[j]))
        heads = np.flatnonzero((flat_size > 0) & (flat_vol == v))               # canonical voxels of this value, ascending
        sizes = flat_size[heads]
        kept = np.zeros(len(heads), dtype=bool)
        if len(heads):
            big = int(np.argmax(sizes))                                         # first maximum: ties to the smaller index
            kept = sizes >= need
            if (largest_mask >> j) & 1:
                only = np.zeros(len(heads), dtype=bool)
                only[big] = True
                kept &= only
            info[j] = (len(heads), sizes.sum(), sizes[big], heads[big] + 1, kept.sum(), sizes[kept].sum())
        drop = (vol == v) & ~np.isin(comp, heads[kept] + 1)
        out[drop] = 0
    return out, info


def overlap(pred, gt, ids):
    """counts int64 [D, n, 3] = (|P & G|, |P|, |G|) per slice and object"""
    pred, gt = np.asarray(pred), np.asarray(gt)
    out = np.zeros((pred.shape[0], len(ids), 3), dtype=np.int64)
    for j, v in enumerate(ids):
        p, g = pred == v, gt == v
        out[:, j, 0] = (p & g).sum(axis=(1, 2))
        out[:, j, 1] = p.sum(axis=(1, 2))
        out[:, j, 2] = g.sum(axis=(1, 2))
    return out


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
def parity_lattice(shape):
    """(d + r + c) % 2 == 0: joined only through edge / corner offsets"""
    d, r, c = np.indices(shape)
    return ((d + r + c) % 2 == 0).astype(np.uint8)


def diagonal_lattice(shape):
    """d % 2 == r % 2 == c % 2: the body-diagonal lattice -- alone under 18, one component under 26"""
    d, r, c = np.indices(shape)
    return ((d % 2 == r % 2) & (r % 2 == c % 2)).astype(np.uint8)


def ellipsoids(shape, n, seed, islands=24):
    """n ellipsoid organs of values ids (later ones cover earlier ones), a few dozen small islands of every value scattered over the volume,
    and some of a value that is nobody's id -> (vol, ids)"""
    D, H, W = shape
    rng = np.random.RandomState(seed)
    ids = (rng.permutation(255)[:n] + 1).tolist()
    stray = next(v for v in range(1, 256) if v not in ids)
    z, y, x = np.indices(shape)
    vol = np.zeros(shape, dtype=np.uint8)
    for v in ids:
        cz, cy, cx = rng.uniform(0, D), rng.uniform(0, H), rng.uniform(0, W)
        rz, ry, rx = rng.uniform(0.6, max(D / 2, 1)), rng.uniform(0.6, max(H / 3, 1)), rng.uniform(0.6, max(W / 3, 1))
        vol[((z - cz) / rz) ** 2 + ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0] = v
    for v in ids + [stray]:
        for _ in range(islands):
            d, r, c = rng.randint(0, D), rng.randint(0, H), rng.randint(0, W)
            h, w = rng.randint(1, 4), rng.randint(1, 6)
            vol[d, r: r + h, c: c + w] = v
    return vol, ids


def noise(shape, values, seed):
    """every voxel drawn from 0 .. values - 1: the many-components worst case"""
    return np.random.RandomState(seed).randint(0, values, shape).astype(np.uint8)


def serpentine(shape):
    """even rows fully set, odd row r one voxel (column W-1 if r % 4 == 1, column 0 if r % 4 == 3) in the even slices; the odd slices hold
    only voxel (0, 0): one component under 6 / 18 / 26, one per non-empty slice under 4 / 8; long chains, deep trees"""
    D, H, W = shape
    vol = np.zeros(shape, dtype=np.uint8)
    for d in range(D):
        if d % 2:
            vol[d, 0, 0] = 1
            continue
        vol[d, 0::2, :] = 1
        vol[d, 1::4, W - 1] = 1
        vol[d, 3::4, 0] = 1
    return vol


def n_components(size):
    return int((np.asarray(size) > 0).sum())
