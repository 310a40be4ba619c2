"""Numpy restatement of ops.label_stats / ops.label_pick (csrc/prompts.hip), one np.argwhere per (slice, object) pair as the reference's
dataset does it, and the fixtures the CPU and GPU tests share.

stats[d, j] = (count, r0, r1, c0, c1) of vol[d] == ids[j] (inclusive extents; (0, -1, -1, -1, -1) when absent); rows[d, j, y] = the count in
row y; xy[d, j] = argwhere(vol[d] == ids[j])[k][::-1] = (column, row) with k outside [0, count) clamped to count - 1, (-1, -1) when absent;
from a uniform word, k = (u * count) >> 32."""
import numpy as np

SHAPES = [(1, 1, 1), (2, 5, 37), (3, 64, 64), (9, 130, 100), (2, 33, 1024), (1, 1024, 1024),
          (2, 700, 48)]      # 700 rows: 11 row bands of 64 per slice in the stats kernel, 3 rounds of 256 rows in the pick kernel


def stats(vol, ids):
    D, H, _ = vol.shape
    st = np.full((D, len(ids), 5), -1, dtype=np.int64)
    rows = np.zeros((D, len(ids), H), dtype=np.int64)
    for d in range(D):
        for j, v in enumerate(ids):
            idx = np.argwhere(vol[d] == v)
            st[d, j, 0] = len(idx)
            if len(idx):
                st[d, j, 1:] = idx[:, 0].min(), idx[:, 0].max(), idx[:, 1].min(), idx[:, 1].max()
                rows[d, j] = np.bincount(idx[:, 0], minlength=H)
    return st, rows


def k_from_u(u, count):
    """the kernel's rule on numpy integers: u uint32 words, count < 2^27, so the product fits 64 bits"""
    return ((np.asarray(u).astype(np.uint64) * np.asarray(count).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)


def pick(vol, ids, k):
    D = vol.shape[0]
    xy = np.full((D, len(ids), 2), -1, dtype=np.int64)
    for d in range(D):
        for j, v in enumerate(ids):
            idx = np.argwhere(vol[d] == v)
            if len(idx):
                kk = int(k[d, j])
                xy[d, j] = idx[kk if 0 <= kk < len(idx) else len(idx) - 1][::-1]
    return xy


# ---- fixtures: name -> (vol uint8 [D, H, W], ids) ------------------------------------------------------------------------------------
def _ids(n, rng):
    return (rng.permutation(255)[:n] + 1).tolist()


def blobs(shape, n, seed):
    """ellipses of n objects (later ones cover earlier ones) and of one value that is nobody's id; every object misses some slices"""
    D, H, W = shape
    rng = np.random.RandomState(seed)
    ids = _ids(n, rng)
    stray = next(v for v in range(1, 256) if v not in ids)
    ys, xs = np.mgrid[0:H, 0:W]
    vol = np.zeros(shape, dtype=np.uint8)
    for d in range(D):
        for j, v in enumerate(ids + [stray]):
            if (d + j) % 4 == 3 or (n > 1 and D == 1 and j == n - 1):
                continue
            cy, cx = rng.uniform(0, H), rng.uniform(0, W)
            ry, rx = rng.uniform(0.5, max(H / 3, 1)), rng.uniform(0.5, max(W / 3, 1))
            vol[d][((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2 <= 1.0] = v
    return vol, ids


def noise(shape, n, seed):
    """every voxel drawn from {0, the ids, a value that is nobody's id}: every lane sees many runs"""
    rng = np.random.RandomState(seed)
    ids = _ids(n, rng)
    pool = np.array([0] + ids + [next(v for v in range(1, 256) if v not in ids)], dtype=np.uint8)
    return pool[rng.randint(0, len(pool), shape)], ids


def checkerboard(shape):
    D, H, W = shape
    d, y, x = np.mgrid[0:D, 0:H, 0:W]
    vol = np.where((x + y + d) % 2 == 0, 3, 250).astype(np.uint8)
    vol[(x + 2 * y) % 5 == 0] = 77                           # present in the volume, not in ids
    return vol, [3, 250]


def full(shape):
    """slice 0 all 3, slice 1 all 250, the rest split at an odd column; 9 is nobody's id"""
    vol = np.full(shape, 3, dtype=np.uint8)
    if shape[0] > 1:
        vol[1] = 250
    vol[2:, :, shape[2] // 3:] = 250
    vol[2:, : shape[1] // 2, : shape[2] // 5] = 9
    return vol, [3, 250]


def corners(shape):
    """one-voxel objects at the four corners (where corners coincide the later one stays), nothing else"""
    D, H, W = shape
    vol = np.zeros(shape, dtype=np.uint8)
    vol[:, 0, 0], vol[:, 0, W - 1], vol[:, H - 1, 0], vol[:, H - 1, W - 1] = 1, 2, 3, 4
    return vol, [1, 2, 3, 4]


def lines(shape):
    """one object that is a single whole row, one that is a single column (it cuts the row; the segment below takes its last voxel), one
    that is a row segment"""
    D, H, W = shape
    vol = np.zeros(shape, dtype=np.uint8)
    vol[:, H // 2, :] = 10
    vol[:, :, W // 3] = 20
    vol[:, H - 1, W // 4: W // 4 + max(1, W // 2)] = 30
    return vol, [20, 10, 30]


def cases():
    """(name, vol, ids), built on demand: every shape with blobs of 1, 4 or 13 objects, and the adversarial fixtures on the shapes where
    they take another path (one row, rows shorter than a lane's 16 voxels, rows that are no multiple of 16, several bands, a whole band
    per wave)"""
    for i, shape in enumerate(SHAPES):
        yield "blobs%d_%dx%dx%d" % ((1, 4, 13)[i % 3], *shape), *blobs(shape, (1, 4, 13)[i % 3], i)
    for shape in [(1, 1, 1), (2, 5, 37), (3, 64, 64), (9, 130, 100), (2, 33, 1024), (2, 700, 48)]:
        for fn in (checkerboard, full, corners, lines):
            yield "%s_%dx%dx%d" % (fn.__name__, *shape), *fn(shape)
    yield "blobs13_1x1024x1024b", *blobs((1, 1024, 1024), 13, 50)
    yield "blobs32_9x130x100", *blobs((9, 130, 100), 32, 51)
    yield "noise32_3x64x64", *noise((3, 64, 64), 32, 52)
    yield "noise32_2x5x37", *noise((2, 5, 37), 32, 53)
    yield "noise4_2x33x1024", *noise((2, 33, 1024), 4, 54)
    yield "lines_1x1024x1024", *lines((1, 1024, 1024))


def k_choices(st, seed):
    """name -> ("k" | "u", table [D, n]): first and last voxel, indices outside the range, and uniform words with the extremes"""
    count = st[..., 0]
    rng = np.random.RandomState(seed)
    u = rng.randint(0, 2 ** 32, count.shape, dtype=np.int64)
    return {"first": ("k", np.zeros_like(count)), "last": ("k", np.maximum(count - 1, 0)), "beyond": ("k", count + rng.randint(0, 3, count.shape)),
            "negative": ("k", np.full_like(count, -1)), "inside": ("k", (rng.uniform(size=count.shape) * count).astype(np.int64)),
            "u_zero": ("u", np.zeros_like(count)), "u_max": ("u", np.full_like(count, 2 ** 32 - 1)), "u_random": ("u", u)}


def row_edges(slice2d, v):
    """a volume of copies of one slice and k [D, 1] = the first and the last voxel of every occupied row of value v"""
    per_row = (slice2d == v).sum(axis=1)
    incl = np.cumsum(per_row)
    ks = [int(x) for y in np.nonzero(per_row)[0] for x in (incl[y] - per_row[y], incl[y] - 1)]
    return np.repeat(slice2d[None], len(ks), axis=0), np.array(ks, dtype=np.int64)[:, None]
