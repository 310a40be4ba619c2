"""Brute-force numpy restatement of the surface meshes of label volumes, written from the definitions, not from the kernels' walk.

m = (labels == v), not-organ outside the volume.  Lattice point p = (k, j, i), 0 <= k <= D, 0 <= j <= H, 0 <= i <= W, is the common corner of
the eight voxels (k-1..k, j-1..j, i-1..i), its cell.  Everything below is a dense array over the lattice: cell[dz, dy, dx][k, j, i] is the
membership of voxel (k - 1 + dz, j - 1 + dy, i - 1 + dx).  A tight crop around the organ changes nothing (everything outside is not-organ
either way, and ascending lattice index is ascending (k, j, i) in any frame), so the work is done there and offsets are added back."""
import itertools

import numpy as np

AXES = (0, 1, 2)                                             # z, y, x
# (b, c) with e_b x e_c = e_a in the right-handed frame (x, y, z)
QUAD_AXES = {2: (1, 0), 1: (0, 2), 0: (2, 1)}


def _cells(m):
    """bool [D, H, W] -> dict (dz, dy, dx) -> bool [D + 1, H + 1, W + 1]"""
    D, H, W = m.shape
    mp = np.zeros((D + 2, H + 2, W + 2), dtype=bool)
    mp[1:-1, 1:-1, 1:-1] = m
    return {d: mp[d[0]: d[0] + D + 1, d[1]: d[1] + H + 1, d[2]: d[2] + W + 1] for d in itertools.product((0, 1), repeat=3)}


def _unit(a):
    e = [0, 0, 0]
    e[a] = 1
    return tuple(e)


def organ_mesh(labels, v, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), placement="nets", relax=0):
    """-> dict: vertices float32 [nv, 3] (z, y, x), quads int32 [nq, 4], u float64 [nv, 3] (voxel units), lattice int64 [nv, 3]"""
    assert placement in ("corner", "nets") and 0 <= relax <= 64
    labels = np.asarray(labels)
    full = labels == v
    empty = dict(vertices=np.zeros((0, 3), np.float32), quads=np.zeros((0, 4), np.int32), u=np.zeros((0, 3)), lattice=np.zeros((0, 3), np.int64))
    if not full.any():
        return empty
    nz = [np.flatnonzero(full.any(axis=tuple(b for b in AXES if b != a))) for a in AXES]
    off = np.array([int(s[0]) for s in nz], dtype=np.int64)
    m = full[nz[0][0]: nz[0][-1] + 1, nz[1][0]: nz[1][-1] + 1, nz[2][0]: nz[2][-1] + 1]
    cell = _cells(m)
    shape = cell[(0, 0, 0)].shape
    stack = np.stack([cell[d] for d in sorted(cell)])
    is_vertex = stack.any(axis=0) & ~stack.all(axis=0)
    number = np.cumsum(is_vertex.ravel()).reshape(shape) - 1          # valid where is_vertex
    lattice = np.argwhere(is_vertex).astype(np.int64)                 # ascending (k, j, i): the canonical order
    coord = lattice + off                                             # lattice coordinates in the volume

    # quads: voxel B = q0 is cell voxel (1, 1, 1), A = q0 - e_a
    keys, rows = [], []
    flat = np.arange(is_vertex.size, dtype=np.int64).reshape(shape)
    for a in AXES:
        d_a = tuple(1 - x for x in _unit(a))
        A, B = cell[d_a], cell[(1, 1, 1)]
        q0 = np.argwhere(A != B)
        if len(q0) == 0:
            continue
        b, c = QUAD_AXES[a]
        eb, ec = np.array(_unit(b)), np.array(_unit(c))
        a_is_organ = A[tuple(q0.T)]
        second = np.where(a_is_organ[:, None], q0 + eb, q0 + ec)
        fourth = np.where(a_is_organ[:, None], q0 + ec, q0 + eb)
        corners = [q0, second, q0 + eb + ec, fourth]
        for cn in corners:
            assert is_vertex[tuple(cn.T)].all()
        rows.append(np.stack([number[tuple(cn.T)] for cn in corners], axis=1))
        keys.append(3 * flat[tuple(q0.T)] + a)
    if rows:
        order = np.argsort(np.concatenate(keys), kind="stable")
        quads = np.concatenate(rows)[order].astype(np.int32)
    else:
        quads = np.zeros((0, 4), np.int32)

    # positions, dense over the lattice, in volume voxel units
    grid = np.stack(np.meshgrid(*[np.arange(s, dtype=np.int64) + o for s, o in zip(shape, off)], indexing="ij"), axis=-1)    # c_a
    if placement == "corner":
        U = grid.astype(np.float64) - 0.5
    else:
        n = np.zeros(shape, dtype=np.int64)
        S = np.zeros(shape + (3,), dtype=np.int64)
        for e in AXES:                                               # the 12 edges: along e, at the four offsets of the other two axes
            others = [a for a in AXES if a != e]
            for o0, o1 in itertools.product((0, 1), repeat=2):
                d0, d1 = [0, 0, 0], [0, 0, 0]
                d0[e], d1[e] = 0, 1
                d0[others[0]] = d1[others[0]] = o0
                d0[others[1]] = d1[others[1]] = o1
                differs = (cell[tuple(d0)] != cell[tuple(d1)]).astype(np.int64)
                n += differs
                for a in others:
                    S[..., a] += differs * (1 if d0[a] == 1 else -1)
        nn = np.where(n > 0, n, 1)
        U = ((2 * grid - 1) * nn[..., None] + S).astype(np.float64) / (2 * nn[..., None]).astype(np.float64)
        assert (n[is_vertex] >= 3).all() and (n[is_vertex] <= 12).all() and (np.abs(S[is_vertex]) <= 8).all()
    if relax:
        link = {}                                                    # (a, side) -> the four voxels with d_a = side are not all equal
        for a in AXES:
            for side in (0, 1):
                four = np.stack([cell[d] for d in cell if d[a] == side])
                link[(a, side)] = four.any(axis=0) & ~four.all(axis=0)
        count = sum(link[k].astype(np.int64) for k in link)
        assert (count[is_vertex] >= 3).all()
        lo, hi = (grid - 1).astype(np.float64), grid.astype(np.float64)
        for _ in range(relax):
            Up = np.pad(U, ((1, 1), (1, 1), (1, 1), (0, 0)))
            total = np.zeros_like(U)
            for a, side in ((0, 0), (1, 0), (2, 0), (2, 1), (1, 1), (0, 1)):          # -z, -y, -x, +x, +y, +z
                sl = [slice(1, -1)] * 3
                sl[a] = slice(2, None) if side else slice(0, -2)
                nb = Up[tuple(sl)]
                lk = link[(a, side)]
                total[lk] = total[lk] + nb[lk]
            new = total / np.where(count > 0, count, 1).astype(np.float64)[..., None]
            new = np.minimum(np.maximum(new, lo), hi)
            U = np.where(is_vertex[..., None], new, U)
    u = U[is_vertex]
    sp, og = np.asarray(spacing, dtype=np.float64), np.asarray(origin, dtype=np.float64)
    vertices = ((u * sp) + og).astype(np.float32)
    return dict(vertices=vertices, quads=quads, u=u, lattice=coord)


def sizes(labels, ids):
    """int64 [n, 2] = (vertices, quads) per id"""
    out = np.zeros((len(ids), 2), dtype=np.int64)
    for j, v in enumerate(ids):
        r = organ_mesh(labels, v, placement="corner")
        out[j] = len(r["vertices"]), len(r["quads"])
    return out


# ---- properties of a mesh -----------------------------------------------------------------------------------------------------------------
def triangles(quads):
    q = np.asarray(quads, dtype=np.int64).reshape(-1, 4)
    return np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], axis=1).reshape(-1, 3)


def directed_edges(quads):
    q = np.asarray(quads, dtype=np.int64).reshape(-1, 4)
    return np.concatenate([np.stack([q[:, e], q[:, (e + 1) % 4]], axis=1) for e in range(4)])


def is_closed(quads):
    """every directed edge (s -> t) occurs as often as (t -> s)"""
    e = directed_edges(quads)
    if len(e) == 0:
        return True
    n = int(e.max()) + 1
    fwd = np.sort(e[:, 0] * n + e[:, 1])
    bwd = np.sort(e[:, 1] * n + e[:, 0])
    return bool(np.array_equal(fwd, bwd))


def euler(nv, quads):
    e = directed_edges(quads)
    und = np.unique(np.sort(e, axis=1), axis=0)
    return int(nv) - len(und) + len(np.asarray(quads).reshape(-1, 4))


def _xyz(vertices):
    return np.asarray(vertices, dtype=np.float64)[:, ::-1]


def area(vertices, quads):
    p, t = _xyz(vertices), triangles(quads)
    if len(t) == 0:
        return 0.0
    return float(0.5 * np.linalg.norm(np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]]), axis=1).sum())


def volume(vertices, quads):
    """divergence theorem over the triangles, in the frame (x, y, z)"""
    p, t = _xyz(vertices), triangles(quads)
    if len(t) == 0:
        return 0.0
    return float((p[t[:, 0]] * np.cross(p[t[:, 1]], p[t[:, 2]])).sum() / 6.0)


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------------
def ball(size=16, radius=6.0, v=1):
    c = (size - 1) / 2.0
    z, y, x = np.meshgrid(*[np.arange(size) - c] * 3, indexing="ij")
    return ((z * z + y * y + x * x) <= radius * radius).astype(np.uint8) * v


def ring(v=1):
    vol = np.zeros((3, 5, 5), dtype=np.uint8)
    vol[1, 1:4, 1:4] = v
    vol[1, 2, 2] = 0
    return vol


def noise(shape, values, seed, p=0.5):
    """every voxel: with probability p one of values (uniform), else 0"""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(values), size=shape)
    return np.where(rng.random(shape) < p, np.asarray(values, dtype=np.uint8)[pick], 0).astype(np.uint8)


def blobs(shape, values, seed, cell=8):
    """piecewise-constant noise: blocks of `cell` voxels per side carry one of (0,) + values"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, len(values) + 1, size=[(s + cell - 1) // cell for s in shape])
    table = np.asarray((0,) + tuple(values), dtype=np.uint8)
    big = table[coarse]
    for a in range(3):
        big = np.repeat(big, cell, axis=a)
    return np.ascontiguousarray(big[:shape[0], :shape[1], :shape[2]])
