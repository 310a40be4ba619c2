"""Host restatement of msam2_label_fill_holes (helper of the tests, not a test).

restate() is scipy.ndimage.binary_fill_holes once per organ with components_restate.structure(c) as the structure of the background flood,
scipy.ndimage.label on the filled voxels for the holes and their sizes, and the rule of the definition in plain numpy: a hole qualifies iff
max_voxels[j] == 0 or size <= max_voxels[j], a voxel is eligible iff its input value is 0 (claim "background") or always ("any"), the smallest
j wins, every hole is a hole of the input.  Its keyword `mistake` swaps in one of the simulated mistakes of MISTAKES (the CPU test asserts
that each of them is caught by some fixture).  flood() is an independent pure-numpy flood from the frame that restate() itself is checked
against on the tiny fixtures.  Everything returned is numpy: out uint8 like the volume, info int64 [n, 4]."""
import collections

import numpy as np
from components_restate import offsets, structure
from scipy import ndimage

CONNECTIVITIES = (6, 18, 26, 4, 8)
CLAIMS = ("background", "any")
MISTAKES = ("organ_connectivity", "plane_box_z_exterior", "frame_ignored", "size_of_zeros", "less_than", "priority_reversed", "claims_swapped",
            "recomputed_per_organ")
_DUAL = {6: 26, 26: 6, 18: 18, 4: 8, 8: 4}


def per_object(max_voxels, n):
    if max_voxels is None:
        return [0] * n
    return [int(max_voxels)] * n if isinstance(max_voxels, (int, np.integer)) else [int(v) for v in max_voxels]


def hole_labels(vol, v, connectivity, mistake=None):
    """(lab int [D, H, W], k): the holes of value v in vol numbered 1 .. k, 0 elsewhere"""
    c = _DUAL[connectivity] if mistake == "organ_connectivity" else connectivity
    st = structure(c)
    organ = vol == v
    if mistake == "frame_ignored":
        holes = ~organ if organ.any() else np.zeros_like(organ)
    else:
        holes = ndimage.binary_fill_holes(organ, structure=st) & ~organ
    if mistake == "plane_box_z_exterior" and connectivity in (4, 8) and organ.any():
        zs = np.flatnonzero(organ.any(axis=(1, 2)))
        holes[zs[0]] = False
        holes[zs[-1]] = False
    return ndimage.label(holes, structure=st)


def restate(vol, ids, connectivity=6, max_voxels=None, claim="background", mistake=None):
    vol = np.asarray(vol, dtype=np.uint8)
    n = len(ids)
    mv = per_object(max_voxels, n)
    if mistake == "claims_swapped":
        claim = CLAIMS[1 - CLAIMS.index(claim)]
    out = vol.copy()
    info = np.zeros((n, 4), dtype=np.int64)
    claimed = np.zeros(vol.shape, dtype=bool)
    order = range(n - 1, -1, -1) if mistake == "priority_reversed" else range(n)
    for j in order:
        source = out.copy() if mistake == "recomputed_per_organ" else vol
        lab, k = hole_labels(source, ids[j], connectivity, mistake)
        counted = lab[source == 0] if mistake == "size_of_zeros" else lab.reshape(-1)
        sizes = np.bincount(counted, minlength=k + 1)[1:]
        fits = np.ones(k, dtype=bool) if mv[j] == 0 else (sizes < mv[j] if mistake == "less_than" else sizes <= mv[j])
        take = np.isin(lab, 1 + np.flatnonzero(fits)) & ~claimed
        if claim == "background":
            take &= source == 0
        out[take] = ids[j]
        claimed |= take
        info[j] = (k, sizes.sum(), fits.sum(), take.sum())
    return out, info


def _spread(seed, allowed, offs):
    """the voxels of `allowed` reachable from `seed` by steps of offs, by repeated shifting (tiny volumes only)"""
    reached = seed & allowed
    while True:
        p = np.pad(reached, 1)
        grown = reached.copy()
        for dz, dy, dx in offs:
            grown |= p[1 + dz: 1 + dz + reached.shape[0], 1 + dy: 1 + dy + reached.shape[1], 1 + dx: 1 + dx + reached.shape[2]]
        grown &= allowed
        if (grown == reached).all():
            return reached
        reached = grown


def flood(vol, ids, connectivity=6, max_voxels=None, claim="background"):
    """the same (out, info) without scipy: the complement of every organ is flooded from the frame, what stays dry is split into holes by
    further floods, and every voxel then looks for the first organ that may have it"""
    vol = np.asarray(vol, dtype=np.uint8)
    n = len(ids)
    mv = per_object(max_voxels, n)
    offs = offsets(connectivity)
    frame = np.zeros(vol.shape, dtype=bool)
    frame[:, 0, :] = frame[:, -1, :] = frame[:, :, 0] = frame[:, :, -1] = True
    if connectivity in (6, 18, 26):
        frame[0] = frame[-1] = True
    info = np.zeros((n, 4), dtype=np.int64)
    may_have = []                                            # per organ: the voxels of its qualifying holes
    for j, v in enumerate(ids):
        comp = vol != v
        dry = comp & ~_spread(frame, comp, offs) if (vol == v).any() else np.zeros(vol.shape, dtype=bool)
        good = np.zeros(vol.shape, dtype=bool)
        while dry.any():
            seed = np.zeros(vol.shape, dtype=bool)
            seed[tuple(np.argwhere(dry)[0])] = True
            hole = _spread(seed, dry, offs)
            dry &= ~hole
            size = int(hole.sum())
            fits = mv[j] == 0 or size <= mv[j]
            info[j, 0] += 1
            info[j, 1] += size
            info[j, 2] += fits
            if fits:
                good |= hole
        may_have.append(good)
    out = vol.copy()
    for x in np.ndindex(vol.shape):
        if claim == "background" and vol[x] != 0:
            continue
        for j in range(n):
            if may_have[j][x]:
                out[x] = ids[j]
                info[j, 3] += 1
                break
    return out, info


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
Fixture = collections.namedtuple("Fixture", "name vol ids max_voxels tiny")


def shell(side=7, value=1, lo=1, hi=5):
    """a 1-voxel-thick cubic shell lo .. hi of `value` in a side^3 volume: the cavity holds (hi - lo - 1)^3 voxels"""
    vol = np.zeros((side,) * 3, dtype=np.uint8)
    vol[lo: hi + 1, lo: hi + 1, lo: hi + 1] = value
    vol[lo + 1: hi, lo + 1: hi, lo + 1: hi] = 0
    return vol


def ring_slices(D, leak_slice=None):
    """D slices of 7 x 7, each a 5 x 5 ring of 1: a tunnel along z; the ring's corner (1, 1) is missing in leak_slice"""
    vol = np.zeros((D, 7, 7), dtype=np.uint8)
    vol[:, 1:6, 1:6] = 1
    vol[:, 2:5, 2:5] = 0
    if leak_slice is not None:
        vol[leak_slice, 1, 1] = 0
    return vol


def serpentine():
    """4 x 96 x 160, all organ but one cavity in slices 1 and 2 that winds through every row 1 .. 93: odd rows are open from column 1 to 158,
    even rows hold the one voxel that joins them, alternately at the right and at the left end"""
    vol = np.ones((4, 96, 160), dtype=np.uint8)
    for r in range(1, 94, 2):
        vol[1:3, r, 1:159] = 0
    for r in range(2, 93, 2):
        vol[1:3, r, 158 if r % 4 == 2 else 1] = 0
    return vol


def random_volume(seed=5):
    """6 x 48 x 80: smooth noise cut into the labels 1 .. 3 at its terciles, then background voxels sprinkled over it, alone and in pairs"""
    rng = np.random.RandomState(seed)
    f = ndimage.gaussian_filter(rng.standard_normal((6, 48, 80)), (1.0, 3.0, 3.0))
    lo, hi = np.percentile(f, [33, 66])
    vol = (1 + (f > lo) + (f > hi)).astype(np.uint8)
    vol[rng.random_sample(vol.shape) < 0.03] = 0
    for d, r, c in zip(rng.randint(0, 6, 60), rng.randint(0, 47, 60), rng.randint(0, 79, 60)):
        vol[d, r: r + 2, c: c + 1 + (d % 2)] = 0
    return vol


def size_limits():
    """two slabs, organ 1 and organ 2, whose holes lie in slice 2: organ 1 holds holes of 4 and 5 voxels (limit 4), organ 2 holes of 2 and 3
    and one of 2 background voxels and 1 voxel of the unlisted value 9 (limit 2)"""
    vol = np.zeros((5, 12, 30), dtype=np.uint8)
    vol[:, :, 0:14] = 1
    vol[:, :, 15:30] = 2
    vol[2, 2, 2:6] = 0
    vol[2, 5, 2:7] = 0
    vol[2, 2, 17:19] = 0
    vol[2, 5, 17:20] = 0
    vol[2, 8, 17:19] = 0
    vol[2, 8, 19] = 9
    return vol


def fixtures():
    out = []
    add = lambda name, vol, ids=(1,), max_voxels=None, tiny=True: out.append(Fixture(name, vol, list(ids), max_voxels, tiny))   # noqa: E731
    add("shell_closed", shell())
    leak = shell()
    leak[1, 1, 3] = 0                                        # touches the cavity's (2, 2, 3) by an edge diagonal only
    add("shell_edge_leak", leak)
    leak = shell()
    leak[1, 1, 1] = 0                                        # touches the cavity's (2, 2, 2) by a corner diagonal only
    add("shell_corner_leak", leak)
    add("plane_corner_leak", ring_slices(3, leak_slice=1))
    add("z_tunnel", ring_slices(5))
    add("one_slice", ring_slices(1))
    vol = np.zeros((6, 7, 7), dtype=np.uint8)
    vol[0:5, 0:6, 0:6] = 1
    vol[0:2, 2:4, 2:4] = 0                                   # a cavity on the z face: a hole slice by slice only
    vol[3, 0:2, 4] = 0                                       # a cavity on the first row: no hole for anybody
    add("cavity_on_frame", vol)
    nested = shell(9, 5, 1, 7) + shell(9, 3, 2, 6)
    add("nested_outer_first", nested, (5, 3))
    add("nested_inner_first", nested, (3, 5))
    vol = shell()
    vol[3, 3, 2:5] = 9
    add("enclosed_value", vol, (1,), 27)
    add("size_limits", size_limits(), (1, 2), [4, 2])
    vol = np.zeros((7, 7, 14), dtype=np.uint8)
    vol[:, :, :7] = shell(value=7)
    vol[:, :, 7:] = shell(value=2)
    add("absent_and_unordered", vol, (7, 200, 2))
    vol = np.zeros((5, 6, 7), dtype=np.uint8)
    vol[0:5, 1:6, 1:6] = 4
    vol[1:4, 2:5, 3] = 0
    vol[2, 3, 2:5] = 0
    add("odd_sizes", vol, (4,))
    add("one_column", np.ones((4, 9, 1), dtype=np.uint8))
    add("one_row", np.ones((4, 1, 9), dtype=np.uint8))
    add("serpentine", serpentine(), tiny=False)
    add("random", random_volume(), (2, 1, 3), 1, tiny=False)
    return out
