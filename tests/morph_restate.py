"""Host restatement of msam2_label_morph / ops.label_morph / volume_labels.morph_labels (helper of the tests, not a test).

ball(): the integer offsets with d2 <= r2, d2 = ((sx2 dx^2 + sy2 dy^2) + sz2 dz^2) in float64 -- numpy rounds every product and sum on its
own.  dilate(): the OR of the mask shifted by every offset, inside the volume.  erode(): the dilation of the complement inside the volume,
taken away from the mask: beyond the volume there is nothing, so the frame does not erode.  open / close: one after the other.  restate():
the write-back rules, the nearest-wins rule with surface_restate.d2 against the ORIGINAL masks.  `mistake=` switches one deliberate error
on; tests/test_label_morph_cpu.py checks that each of them changes a fixture's result.  The fixtures at the end are shared by that file and
tests/test_label_morph_gpu.py."""
import collections

import numpy as np

import surface_restate as S

OPS = ("erode", "dilate", "open", "close")
CLAIMS = ("background", "any")
SPACINGS = S.SPACINGS
# (keyword, value): how the radius reaches the interface.  d2 = 2 is met with equality at unit spacing; 3.2 reaches the next slice at 3 mm
RADII = (("radius2", 2.0), ("radius", 3.2))
MISTAKES = ("lt", "no_spacing", "frame_erodes", "first_wins", "ties_later", "claims_swapped", "open_close_swapped", "features_tight",
            "growth_tight", "r2_f32")


def r2_of(kind, value):
    """the float64 squared radius the library receives: radius= is squared in float64, radius2= is taken as is; scalar or one per object"""
    vals = np.atleast_1d(np.asarray(value, dtype=np.float64))
    return [float(v * v) if kind == "radius" else float(v) for v in vals]


def ball(r2, spacing, shape, strict=False):
    """int [k, 3]: the offsets (dz, dy, dx) that can occur inside a volume of `shape` with d2 <= r2 (strict: <, a mistake)"""
    sz, sy, sx = (np.float64(s) for s in spacing)
    sz2, sy2, sx2 = sz * sz, sy * sy, sx * sx
    dz, dy, dx = (np.arange(-(n - 1), n, dtype=np.float64) for n in shape)
    dz, dy, dx = dz[:, None, None], dy[None, :, None], dx[None, None, :]
    d2 = (sx2 * (dx * dx) + sy2 * (dy * dy)) + sz2 * (dz * dz)
    inside = d2 < np.float64(r2) if strict else d2 <= np.float64(r2)
    return np.argwhere(inside) - (np.array(shape) - 1)


def _shifted_or(mask, offsets):
    out = np.zeros_like(mask)
    for off in offsets:
        dst, src = [], []
        for o, n in zip(off, mask.shape):                   # out[q] |= mask[q - off]
            dst.append(slice(max(o, 0), n + min(o, 0)))
            src.append(slice(max(-o, 0), n + min(-o, 0)))
        out[tuple(dst)] |= mask[tuple(src)]
    return out


def _tight(mask):
    at = np.argwhere(mask)
    box = np.zeros_like(mask)
    if len(at):
        lo, hi = at.min(axis=0), at.max(axis=0)
        box[lo[0]: hi[0] + 1, lo[1]: hi[1] + 1, lo[2]: hi[2] + 1] = True
    return box


def dilate(mask, r2, spacing, mistake=None):
    out = _shifted_or(mask, ball(r2, spacing, mask.shape, strict=mistake == "lt"))
    if mistake == "growth_tight":
        out &= _tight(mask)
    return out


def erode(mask, r2, spacing, mistake=None):
    outside = ~mask
    if mistake == "features_tight":
        outside &= _tight(mask)
    if mistake == "frame_erodes":                           # as if the volume sat in a sea of other voxels
        pad = [(n, n) for n in mask.shape]
        big = _shifted_or(np.pad(outside, pad, constant_values=True), ball(r2, spacing, tuple(3 * n for n in mask.shape)))
        reach = big[tuple(slice(n, 2 * n) for n in mask.shape)]
    else:
        reach = _shifted_or(outside, ball(r2, spacing, mask.shape, strict=mistake == "lt"))
    return mask & ~reach


def morph(mask, op, r2, spacing, mistake=None):
    """the result set of one organ"""
    if mistake == "open_close_swapped":
        op = {"open": "close", "close": "open"}.get(op, op)
    if op == "erode":
        return erode(mask, r2, spacing, mistake)
    if op == "dilate":
        return dilate(mask, r2, spacing, mistake)
    if op == "open":
        return dilate(erode(mask, r2, spacing, mistake), r2, spacing, mistake)
    assert op == "close", op
    return erode(dilate(mask, r2, spacing, mistake), r2, spacing, mistake)


def result_sets(vol, ids, op, r2, spacing, mistake=None):
    """per organ the bool result set; r2: one squared radius per organ"""
    if mistake == "r2_f32":
        r2 = [float(np.float32(r)) for r in r2]
    if mistake == "no_spacing":
        spacing = (1.0, 1.0, 1.0)
    return [morph(vol == v, op, r, spacing, mistake) for v, r in zip(ids, r2)]


def write_back(vol, ids, sets, op, spacing, claim="background", mistake=None):
    """(out uint8, info int64 [n, 4]) from the organs' result sets"""
    if mistake == "claims_swapped":
        claim = {"background": "any", "any": "background"}[claim]
    if mistake == "no_spacing":
        spacing = (1.0, 1.0, 1.0)
    if mistake == "open_close_swapped":
        op = {"open": "close", "close": "open"}.get(op, op)
    out = vol.copy()
    info = np.zeros((len(ids), 4), dtype=np.int64)
    if op in ("erode", "open"):
        for j, (v, R) in enumerate(zip(ids, sets)):
            out[(vol == v) & ~R] = 0
    else:
        eligible = vol == 0 if claim == "background" else ~np.isin(vol, ids)
        best = np.full(vol.shape, np.inf)
        for j, (v, R) in enumerate(zip(ids, sets)):
            cand = R & eligible
            q = np.argwhere(cand)
            d = S.d2(q, np.argwhere(vol == v), spacing)
            if mistake == "first_wins":
                take = out[cand] == vol[cand]
            elif mistake == "ties_later":
                take = d <= best[cand]
            else:
                take = d < best[cand]
            q = q[take]
            out[q[:, 0], q[:, 1], q[:, 2]] = v
            best[q[:, 0], q[:, 1], q[:, 2]] = d[take]
    for j, (v, R) in enumerate(zip(ids, sets)):
        info[j] = ((vol == v).sum(), R.sum(), (out == v).sum(), ((out == v) & (vol != v) & (vol != 0)).sum())
    return out, info


def restate(vol, ids, op, r2, spacing=(1.0, 1.0, 1.0), claim="background", mistake=None):
    r2 = list(r2) if np.ndim(r2) else [float(r2)] * len(ids)
    return write_back(vol, ids, result_sets(vol, ids, op, r2, spacing, mistake), op, spacing, claim, mistake)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
Fixture = collections.namedtuple("Fixture", "name vol ids radii")     # radii: tuple of (keyword, value or one value per organ)


def blobs(shape, values, seed, per_value=2):
    """ellipsoids of the given values painted over each other in turn"""
    rng = np.random.RandomState(seed)
    z, y, x = np.indices(shape)
    vol = np.zeros(shape, dtype=np.uint8)
    for _ in range(per_value):
        for v in values:
            c = [rng.uniform(0, n - 1) for n in shape]
            r = [rng.uniform(0.8, max(1.0, n / 4)) for n in shape]
            vol[((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2 <= 1.0] = v
    return vol


def fixtures():
    out = []

    def add(name, vol, ids, radii=RADII):
        assert vol.dtype == np.uint8 and vol.size <= 30000
        out.append(Fixture(name, np.ascontiguousarray(vol), list(ids), tuple(radii)))

    # random blobs of four organs and an unlisted value (9)
    add("blobs_7x24x40", blobs((7, 24, 40), [3, 1, 9, 7, 2], 5), [3, 1, 7, 2])
    add("odd_5x11x67", blobs((5, 11, 67), [4, 9, 6, 5], 8), [6, 4, 5])
    # facing plates: organ 1 at rows 6 and 12, organ 2 between them at rows 8 and 10, all through every slice and column.  Both closings claim
    # row 9 (organ 1's also rows 7 and 11); row 9 is nearer to organ 2, the later one
    v = np.zeros((5, 20, 20), dtype=np.uint8)
    v[:, [6, 12], :] = 1
    v[:, [8, 10], :] = 2
    add("facing_plates", v, [1, 2])
    # a lesion of an unlisted value (50) beside an organ; an absent organ in front
    v = np.zeros((5, 12, 20), dtype=np.uint8)
    v[1:4, 3:9, 4:10] = 1
    v[1:4, 4:8, 10:13] = 50
    add("lesion_and_absent", v, [99, 1])
    # two lobes and a one-voxel bridge between them; a 2 x 2 x 2 organ that every erosion erases
    v = np.zeros((5, 15, 40), dtype=np.uint8)
    v[0:5, 3:12, 3:15] = 1
    v[0:5, 3:12, 25:37] = 1
    v[2, 7, 15:25] = 1
    v[0:2, 13:15, 18:20] = 2
    add("bridge_and_speck", v, [1, 2])
    # an organ that touches all six faces, with a notch and a cavity
    v = np.full((4, 6, 8), 5, dtype=np.uint8)
    v[2, 3, 4] = 0
    v[0, 0, 5:8] = 0
    add("six_faces", v, [5])
    add("one_slice_1x16x70", blobs((1, 16, 70), [1, 2, 9, 3], 11), [2, 3, 1])
    add("two_rows_4x2x40", blobs((4, 2, 40), [1, 2, 3], 12, per_value=3), [1, 2])
    add("two_columns_4x30x2", blobs((4, 30, 2), [1, 2, 3], 13, per_value=3), [2, 1])
    # a row of 181 voxels: three wave chunks, with gaps a closing fills and a thin part an opening drops
    v = np.zeros((3, 5, 200), dtype=np.uint8)
    v[:, 1:4, 10:191] = 1
    v[1, 2, [40, 41, 100, 130]] = 0
    v[:, :, 150:153] = 0
    v[1, 2, 150:153] = 1
    v[0, 0, 60:70] = 2
    add("long_row_3x5x200", v, [1, 2])
    small = blobs((4, 9, 14), [1, 2, 9, 3], 21)
    add("radius_below_the_spacing", small, [1, 2, 3], [("radius", 0.5)])
    add("radius_beyond_the_volume", small[:3, :6, :8], [1, 2, 3], [("radius", 1000.0)])
    add("radius_per_object", blobs((6, 14, 30), [1, 2, 9, 3, 4], 22), [4, 1, 3, 2], [("radius", [1.0, 3.2, 2.0, 0.5]), ("radius2", [2.0, 0.0, 9.0, 1.0])])
    add("sqrt3", small, [2, 1, 3], [("radius", 3 ** 0.5), ("radius2", 3.0)])
    # 32 organs: a grid of boxes of 2 x 3 x 4 voxels, one voxel apart or touching
    v = np.zeros((6, 16, 40), dtype=np.uint8)
    order = np.random.RandomState(3).permutation(32) + 1
    for k, val in enumerate(order):
        a, b, c = k // 16, (k // 8) % 2, k % 8
        v[1 + 3 * a: 3 + 3 * a, 2 + 7 * b: 5 + 7 * b + (k % 3 == 0), 5 * c: 5 * c + 4 + (k % 2)] = val
    add("organs32", v, [int(x) for x in np.random.RandomState(4).permutation(32) + 1])
    return out
