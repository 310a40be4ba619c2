"""Numpy restatement of ops.label_error_clicks (csrc/clicks.hip) and the fixtures the CPU and GPU tests share.

Per slice and object v = ids[j]: FN = {gt == v and pred != v}, FP = {pred == v and gt != v}; d2(q) of a region's voxel = the brute-force
minimum of |q - z|^2 over every pixel z outside the region, the one-pixel frame around the image included; centre mode takes np.argmax of d2
(the first maximum in raster order) of the region with the larger maximum (FN only if strictly larger), uniform mode the k-th voxel of
np.argwhere(FN | FP).  table[d, j] = (x, y, label, |FN|, |FP|, max d2(FN), max d2(FP), 0), the d2 fields -1 in uniform mode,
(-1, -1, -1, 0, 0, ...) without an error voxel.

`defect` turns one rule into a plausible mistake (DEFECTS names them); tests/test_clicks_cpu.py shows that the fixture group of each
mistake tells it from the rule."""
import numpy as np

MAX_OBJ = 32
IDS = [3, 200, 7]
STRAY = 9                                                    # present in the volumes, nobody's id
NO_PIXEL = 1 << 30                                           # d2 where nothing lies outside the region (defect "no_frame" on a full slice)

# defect -> the fixture group (name prefix) that must show it
DEFECTS = {"no_frame": "edges", "last_max": "ties", "ge": "ties", "pred_nonzero": "blobs", "swap_xy": "edges", "stray": "stray",
           "u_off_by_one": "blobs", "next_w": "carry", "next_chunk": "carry", "start_stale": "carry", "start_chunk": "carry"}


def regions(pred, gt, v, defect=None):
    """(FN, FP) of value v on one slice"""
    is_pred = pred != 0 if defect == "pred_nonzero" else pred == v
    return (gt == v) & ~is_pred, is_pred & (gt != v)


def d2_brute(region, frame=True, same=None):
    """int64 [H, W]: per voxel of the region the smallest squared distance to a pixel outside it (0 elsewhere); frame: the one-pixel
    frame around the image is outside; same: pixels that wrongly do not count as outside (defect "stray")"""
    out = np.zeros(region.shape, dtype=np.int64)
    q = np.argwhere(region).astype(np.int32)
    if len(q) == 0:
        return out
    inside = region if same is None else region | same
    pad = int(frame)
    z = (np.argwhere(~np.pad(inside, pad)) - pad).astype(np.int32)
    if len(z) == 0:
        out[region] = NO_PIXEL
        return out
    best = np.empty(len(q), dtype=np.int64)
    for i in range(0, len(q), 256):
        diff = q[i: i + 256, None, :] - z[None, :, :]
        best[i: i + 256] = (diff * diff).sum(-1).min(1)
    out[q[:, 0], q[:, 1]] = best
    return out


CARRY = ("next_w", "next_chunk", "start_stale", "start_chunk")


def d2_chunked(region, defect=None):
    """The same map by the kernel's route: per row the distance to the run's two ends, 64 columns at a time with the head of the run that
    reaches into a chunk (`start`) and the first head right of a chunk (`nxt`) carried between chunks, then the minimum over the rows.
    Without a defect it equals d2_brute.  The CARRY defects break one carry each: nxt never leaves W; nxt is the chunk's own end; start is
    only taken from chunk 0; start is the chunk's own first column."""
    H, W = region.shape
    g = np.zeros((H, W), dtype=np.int64)
    chunks = [np.arange(c, min(W, c + 64)) for c in range(0, W, 64)]
    for y in range(H):
        row = region[y]
        head = np.ones(W, dtype=bool)
        head[1:] = row[1:] != row[:-1]
        heads = [xs[head[xs]] for xs in chunks]
        dl, dr = np.zeros(W, dtype=np.int64), np.zeros(W, dtype=np.int64)
        start = 0
        for c, xs in enumerate(chunks):
            if defect == "start_chunk":
                start = xs[0]
            at = np.searchsorted(heads[c], xs, side="right") - 1
            dl[xs] = np.where(at >= 0, xs - np.append(heads[c], 0)[at], xs - start) + 1       # (at = -1 reads the appended 0: unused)
            if len(heads[c]) and not (defect == "start_stale" and c > 0):
                start = heads[c][-1]
        nxt = W
        for c in range(len(chunks) - 1, -1, -1):
            xs = chunks[c]
            if defect == "next_chunk":
                nxt = xs[-1] + 1
            at = np.searchsorted(heads[c], xs, side="right")
            dr[xs] = np.where(at < len(heads[c]), np.append(heads[c], 0)[np.minimum(at, len(heads[c]))], nxt) - xs
            if len(heads[c]) and defect != "next_w":
                nxt = heads[c][0]
        g[y] = np.minimum(dl, dr)
    cost = np.pad(np.where(region, g * g, 0), ((1, 1), (0, 0)))          # rows -1 and H of the frame, and every voxel outside: 0
    dy = np.arange(H)[:, None] - (np.arange(H + 2)[None, :] - 1)
    d2 = (dy[:, :, None] ** 2 + cost[None, :, :]).min(axis=1)
    return np.where(region, d2, 0)


def k_from_u(u, count):
    return (int(u) * int(count)) >> 32


def table(pred, gt, ids, mode="center", k=None, u=None, defect=None):
    """int64 [D, n, 8]"""
    D, H, W = pred.shape
    out = np.zeros((D, len(ids), 8), dtype=np.int64)
    out[..., :3] = -1
    listed = np.zeros(256, dtype=bool)
    listed[list(ids)] = True
    for d in range(D):
        differ = pred[d] != gt[d]
        stray = (differ & (gt[d] != 0) & ~listed[gt[d]], differ & (pred[d] != 0) & ~listed[pred[d]])      # per kind: another class, no region
        for j, v in enumerate(ids):
            fn, fp = regions(pred[d], gt[d], v, defect)
            row = out[d, j]
            row[3], row[4] = fn.sum(), fp.sum()
            if mode == "uniform":
                row[5] = row[6] = -1
                idx = np.argwhere(fn | fp)
                if len(idx):
                    kk = int(k[d, j]) if k is not None else k_from_u(u[d, j], len(idx)) + (defect == "u_off_by_one")
                    y, x = idx[kk if 0 <= kk < len(idx) else len(idx) - 1]
                    row[:3] = x, y, int(fn[y, x])
                continue
            best = []
            for kind, reg in enumerate((fn, fp)):
                if defect in CARRY:
                    m = d2_chunked(reg, defect)
                else:
                    m = d2_brute(reg, frame=defect != "no_frame", same=stray[kind] if defect == "stray" else None)
                flat = m.reshape(-1)
                at = int(np.argmax(flat)) if defect != "last_max" else len(flat) - 1 - int(np.argmax(flat[::-1]))
                best.append((int(flat[at]), at))
            row[5], row[6] = best[0][0], best[1][0]
            if row[3] + row[4] > 0:
                positive = best[0][0] >= best[1][0] if defect == "ge" else best[0][0] > best[1][0]
                y, x = divmod(best[0][1] if positive else best[1][1], W)
                row[:3] = (y, x, int(positive)) if defect == "swap_xy" else (x, y, int(positive))
    return out


# ---- fixtures: (name, pred, gt, ids), uint8 [D, H, W] ---------------------------------------------------------------------------------
def _ellipses(shape, values, rng, skip):
    D, H, W = shape
    ys, xs = np.mgrid[0:H, 0:W]
    vol = np.zeros(shape, dtype=np.uint8)
    for d in range(D):
        for j, v in enumerate(values):
            if skip(d, j):
                continue
            cy, cx = rng.uniform(0, H), rng.uniform(0, W)
            ry, rx = rng.uniform(0.5, max(H / 2.5, 1)), rng.uniform(0.5, max(W / 2.5, 1))
            vol[d][((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2 <= 1.0] = v
    return vol


def blobs(shape, ids, seed):
    """ellipses of every id but the last (absent everywhere when there are three or more) and of the stray value; the prediction is the
    ground truth moved by a few voxels with some objects missing and one painted over another: crescents, whole objects, voxels that are
    FP of one id and FN of another; every object has slices without error"""
    rng = np.random.RandomState(seed)
    drawn = list(ids[:-1]) if len(ids) >= 3 else list(ids)
    gt = _ellipses(shape, drawn + [STRAY], rng, lambda d, j: (d + j) % 4 == 3)
    pred = np.roll(gt, (min(1, shape[1] - 1), min(2, shape[2] - 1)), axis=(1, 2))
    for d in range(shape[0]):
        if d % 3 == 1:
            pred[d] = gt[d]                                  # a slice without error
        elif d % 3 == 2:
            pred[d][pred[d] == drawn[0]] = drawn[-1] if len(drawn) > 1 else 0
    return pred, gt, list(ids)


def noise(shape, n, seed):
    rng = np.random.RandomState(seed)
    ids = (rng.permutation(255)[:n] + 1).tolist()
    pool = np.array([0] + ids + [next(v for v in range(1, 256) if v not in ids)], dtype=np.uint8)
    return pool[rng.randint(0, len(pool), shape)], pool[rng.randint(0, len(pool), shape)], ids


def edges(shape):
    """slice 0: one FN region along every edge of the image (rows 0 and H - 1 in full width, so they span every 64-column chunk, columns 0
    and W - 1 between them) -- where H, W >= 5 three objects, else one; slice 1: one-voxel FP regions in the four corners; slice 2: FN
    fills the whole slice; slice 3: every voxel is FP of 200 and FN of 3; slice 4: an oblong FP block off the centre"""
    D, H, W = shape
    pred, gt = np.zeros(shape, dtype=np.uint8), np.zeros(shape, dtype=np.uint8)
    gt[0, 0, :], gt[0, H - 1, :] = 3, 200
    if H > 2:
        gt[0, 1: H - 1, 0], gt[0, 1: H - 1, W - 1] = 7, 3
    if D > 1:
        pred[1, 0, 0], pred[1, 0, W - 1], pred[1, H - 1, 0], pred[1, H - 1, W - 1] = 3, 200, 7, 3
    if D > 2:
        gt[2] = 200
    if D > 3:
        gt[3], pred[3] = 3, 200
    if D > 4:
        pred[4, H // 3: H // 3 + max(1, H // 4), W // 5: W // 5 + max(1, W // 2)] = 7
    return pred, gt, list(IDS)


def ties(shape):
    """symmetric regions: even-sided blocks (several voxels share the largest d2); slice 0: one FN block; slice 1: an FN and an FP block of
    the same object and size (equal maxima: the click is negative); slice 2: the FP block one row taller (FP wins or ties), slice 3: the FN
    block larger (positive); slice 4: two equal FN blocks of one object"""
    D, H, W = shape
    pred, gt = np.zeros(shape, dtype=np.uint8), np.zeros(shape, dtype=np.uint8)
    bh, bw = max(1, min(4, H // 2)), max(1, min(6, W // 4))

    def block(vol, d, y, x, h, w, v):
        vol[d, y: y + h, x: x + w] = v
    block(gt, 0, (H - bh) // 2, (W - bw) // 2, bh, bw, 3)
    for d, heights in enumerate([(bh, bh), (bh, min(bh + 1, H)), (min(bh + 2, H), bh), None], start=1):
        if d >= D:
            break
        if heights is None:
            block(gt, d, 0, 0, bh, bw, 200), block(gt, d, H - bh, W - bw, bh, bw, 200)
        else:
            block(gt, d, 0, 0, heights[0], bw, 7), block(pred, d, H - heights[1], W - bw, heights[1], bw, 7)
    return pred, gt, list(IDS)


def stray(shape):
    """an FN block of 3 whose right half the prediction calls 200 (FN of 3 and FP of 200 at once), with a block of the stray value at its
    left (gt stray, pred 0: another class of the FN kind, nobody's region) and one at its right in the prediction"""
    D, H, W = shape
    pred, gt = np.zeros(shape, dtype=np.uint8), np.zeros(shape, dtype=np.uint8)
    a, b, c, e = W // 8, 3 * W // 8, 5 * W // 8, 7 * W // 8
    gt[:, :, a:b], gt[:, :, b:c] = STRAY, 3
    pred[:, :, (b + c) // 2: c], pred[:, :, c:e] = 200, STRAY
    pred[:, :, :a] = 200
    return pred, gt, list(IDS)


def carry(shape):
    """Tall blocks (H = 37: a full-height block is 19 rows from the frame at its middle) whose largest d2 is decided by a row distance that
    crosses a 64-column boundary, so that a wrong carry in the row pass moves the click or changes its d2.
    slice 0: FN columns 40 .. 75 in every row: the maximum is in chunk 0 (columns 57, 58), and its right distance ends at the head in
    chunk 1; slice 1: FP columns 55 .. 85: the maximum (column 70) is in chunk 1, its run starts in chunk 0; slice 2 (W = 200): FN columns
    120 .. 150 with another block at columns 10 .. 20: the maximum (column 135) is in chunk 2, its run starts in chunk 1 and chunk 0 has
    heads of its own; slice 3: 30 rows by columns 10 .. 100; slice 4: FP columns 60 .. W - 6: the right end is up to three chunks away"""
    D, H, W = shape
    assert D == 5 and H == 37 and W >= 130
    pred, gt = np.zeros(shape, dtype=np.uint8), np.zeros(shape, dtype=np.uint8)
    gt[0, :, 40:76] = 3
    pred[1, :, 55:86] = 200
    gt[2, :, min(120, W - 12): min(151, W)], gt[2, :, 10:21] = 7, 3
    gt[3, 3:33, 10:101] = 3
    pred[4, :, 60: W - 5] = 7
    return pred, gt, list(IDS)


def cases():
    """Widths 1, 63, 64, 65, 130 (three 64-column chunks, one ragged) and 200; heights 1, 2 and 37; 1 and 5 slices.  The entry's lower size
    limit is 1 x 1."""
    yield "blobs_1x1x1", *blobs((1, 1, 1), [3], 1)
    yield "blobs_5x37x65", *blobs((5, 37, 65), IDS, 2)
    yield "blobs_5x2x130", *blobs((5, 2, 130), IDS, 3)
    yield "blobs_1x37x200", *blobs((1, 37, 200), IDS, 4)
    yield "blobs1_5x37x63", *blobs((5, 37, 63), [200], 5)
    yield "blobs_5x37x1", *blobs((5, 37, 1), IDS, 6)
    yield "blobs_5x1x200", *blobs((5, 1, 200), IDS, 7)
    yield "blobs32_5x37x64", *blobs((5, 37, 64), list(range(40, 40 + MAX_OBJ)), 8)
    yield "noise32_1x37x65", *noise((1, 37, 65), MAX_OBJ, 9)
    yield "noise3_5x2x63", *noise((5, 2, 63), 3, 10)
    for shape in [(5, 37, 130), (5, 2, 64), (5, 37, 200), (5, 1, 65), (1, 37, 63)]:
        yield "edges_%dx%dx%d" % shape, *edges(shape)
    for shape in [(5, 37, 65), (5, 2, 130), (5, 37, 200)]:
        yield "ties_%dx%dx%d" % shape, *ties(shape)
    for shape in [(1, 37, 130), (5, 2, 200), (1, 1, 64)]:
        yield "stray_%dx%dx%d" % shape, *stray(shape)
    for shape in [(5, 37, 130), (5, 37, 200)]:
        yield "carry_%dx%dx%d" % shape, *carry(shape)
    vol = blobs((5, 37, 65), IDS, 11)[1]
    yield "equal_5x37x65", vol, vol.copy(), list(IDS)


def k_choices(counts, seed):
    """name -> ("k" | "u", table [D, n]) for uniform mode: first and last voxel, indices outside the range, uniform words with the extremes"""
    rng = np.random.RandomState(seed)
    u = rng.randint(0, 2 ** 32, counts.shape, dtype=np.int64)
    return {"first": ("k", np.zeros_like(counts)), "last": ("k", np.maximum(counts - 1, 0)), "beyond": ("k", counts + rng.randint(0, 3, counts.shape)),
            "negative": ("k", np.full_like(counts, -1)), "inside": ("k", (rng.uniform(size=counts.shape) * counts).astype(np.int64)),
            "u_zero": ("u", np.zeros_like(counts)), "u_max": ("u", np.full_like(counts, 2 ** 32 - 1)), "u_random": ("u", u)}


_REFERENCE = {}


def reference(name, pred, gt, ids):
    """the centre-mode table of a fixture, computed once per process and shared (read-only)"""
    if name not in _REFERENCE:
        t = table(pred, gt, ids)
        t.setflags(write=False)
        _REFERENCE[name] = t
    return _REFERENCE[name]
