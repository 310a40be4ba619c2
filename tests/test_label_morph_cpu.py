"""The restatement behind the morphology tests (tests/morph_restate.py) against scipy and against the thresholded distance transform, its
algebra, the radius / radius2 rule, the mistakes its fixtures must catch, and the argument checks of msam2_label_morph that need no GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import morph_restate as R  # noqa: E402
import surface_restate as S  # noqa: E402

FIXTURES = R.fixtures()
BY_NAME = {f.name: f for f in FIXTURES}
UNIT = (1.0, 1.0, 1.0)


def structure(r2):
    """the ball at unit spacing as a scipy structure"""
    k = int(np.floor(np.sqrt(r2)))
    z, y, x = np.mgrid[-k: k + 1, -k: k + 1, -k: k + 1]
    return (x * x + y * y) + z * z <= r2


@pytest.mark.parametrize("r2", [1.0, 2.0, 3.0, 4.0, 9.0])
@pytest.mark.parametrize("name", ["blobs_7x24x40", "six_faces", "one_slice_1x16x70", "two_rows_4x2x40", "bridge_and_speck"])
def test_the_restatement_is_scipy_at_unit_spacing(name, r2):
    fx = BY_NAME[name]
    st = structure(r2)
    for v in fx.ids:
        m = fx.vol == v
        dil = ndimage.binary_dilation(m, st, border_value=0)
        ero = ndimage.binary_erosion(m, st, border_value=1)
        assert np.array_equal(R.morph(m, "dilate", r2, UNIT), dil)
        assert np.array_equal(R.morph(m, "erode", r2, UNIT), ero)
        assert np.array_equal(R.morph(m, "open", r2, UNIT), ndimage.binary_dilation(ero, st, border_value=0))
        assert np.array_equal(R.morph(m, "close", r2, UNIT), ndimage.binary_erosion(dil, st, border_value=1))


@pytest.mark.parametrize("spacing", R.SPACINGS)
def test_the_restatement_is_the_thresholded_distance_transform(spacing):
    fx = BY_NAME["radius_below_the_spacing"]                  # 4 x 9 x 14: the brute-force field is affordable here
    for v in fx.ids:
        m = fx.vol == v
        to_organ, to_outside = S.edt(fx.vol, v, spacing, "surface"), S.edt(fx.vol, v, spacing, "outside")
        for r2 in (0.0, 0.5, 0.5776, 2.0, 3.2 * 3.2, 9.0, 30.0):
            assert np.array_equal(R.morph(m, "dilate", r2, spacing), m | (to_organ <= r2)), (v, r2)
            assert np.array_equal(R.morph(m, "erode", r2, spacing), m & ~(to_outside <= r2)), (v, r2)


@pytest.mark.parametrize("name", ["blobs_7x24x40", "six_faces", "long_row_3x5x200", "facing_plates", "one_slice_1x16x70"])
def test_open_is_inside_close_is_outside_and_both_are_idempotent(name):
    fx = BY_NAME[name]
    for spacing in R.SPACINGS:
        for kind, value in R.RADII:
            (r2,) = R.r2_of(kind, value)
            for v in fx.ids:
                m = fx.vol == v
                o, c = R.morph(m, "open", r2, spacing), R.morph(m, "close", r2, spacing)
                assert not (o & ~m).any() and not (m & ~c).any()
                assert np.array_equal(R.morph(o, "open", r2, spacing), o) and np.array_equal(R.morph(c, "close", r2, spacing), c)


def test_radius_is_squared_in_float64_and_radius2_is_taken_as_is():
    import medical_sam2_amd.ops as ops
    assert (3 ** 0.5) ** 2 == 2.9999999999999996 and (2 ** 0.5) ** 2 == 2.0000000000000004 and (5 ** 0.5) ** 2 == 5.000000000000001
    seed = np.zeros((5, 7, 7), dtype=bool)
    seed[2, 3, 3] = True
    for k, at, reached in ((2, (2, 4, 4), True), (3, (3, 4, 4), False), (5, (2, 5, 4), True)):
        (by_radius,) = R.r2_of("radius", k ** 0.5)
        (by_radius2,) = R.r2_of("radius2", float(k))
        assert ops._radius2("t", k ** 0.5, None, 1) == [by_radius] and ops._radius2("t", None, float(k), 1) == [by_radius2] == [float(k)]
        assert bool(R.morph(seed, "dilate", by_radius, UNIT)[at]) is reached
        assert bool(R.morph(seed, "dilate", by_radius2, UNIT)[at]) is True
    assert ops._radius2("t", [1.0, 2.0], None, 2) == [1.0, 4.0] and ops._radius2("t", None, [1.0, 2.0], 2) == [1.0, 2.0]
    for bad in ((None, None), (1.0, 1.0), (-1.0, None), (None, float("nan")), ([1.0], None)):
        with pytest.raises(ValueError):
            ops._radius2("t", bad[0], bad[1], 2)


def cases(fx):
    for op in R.OPS:
        for claim in (R.CLAIMS if op in ("dilate", "close") else R.CLAIMS[:1]):
            for spacing in R.SPACINGS:
                for kind, value in fx.radii:
                    yield op, claim, spacing, R.r2_of(kind, value) * (1 if np.ndim(value) else len(fx.ids))


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_every_mistake_changes_a_fixtures_result(mistake):
    first = {"r2_f32": "sqrt3"}.get(mistake)                  # (where to look first: it only saves time)
    for fx in sorted(FIXTURES, key=lambda f: f.name != first):
        for op, claim, spacing, r2 in cases(fx):
            good = R.restate(fx.vol, fx.ids, op, r2, spacing, claim)
            bad = R.restate(fx.vol, fx.ids, op, r2, spacing, claim, mistake=mistake)
            if not (np.array_equal(good[0], bad[0]) and np.array_equal(good[1], bad[1])):
                return
    pytest.fail(f"no fixture notices {mistake}")


def test_nearest_wins_differs_from_first_wins_for_close_on_the_plates():
    fx = BY_NAME["facing_plates"]
    (r2,) = R.r2_of("radius", 3.2)
    out, info = R.restate(fx.vol, fx.ids, "close", [r2, r2], UNIT)
    assert (out[:, 9, :] == 2).all() and (out[:, [7, 11], :] == 1).all()
    first, _ = R.restate(fx.vol, fx.ids, "close", [r2, r2], UNIT, mistake="first_wins")
    assert (first[:, 9, :] == 1).all()
    assert info.tolist() == [[200, 700, 400, 0], [200, 300, 300, 0]]


def test_any_takes_the_lesion_and_background_does_not():
    fx = BY_NAME["lesion_and_absent"]
    (r2,) = R.r2_of("radius", 3.2)
    bg, bg_info = R.restate(fx.vol, fx.ids, "dilate", [r2, r2], UNIT, "background")
    anyv, any_info = R.restate(fx.vol, fx.ids, "dilate", [r2, r2], UNIT, "any")
    assert (bg == 50).sum() == (fx.vol == 50).sum() and (anyv == 50).sum() < (fx.vol == 50).sum()
    assert bg_info[0].tolist() == [0, 0, 0, 0] and bg_info[1, 3] == 0 and any_info[1, 3] == (fx.vol == 50).sum() - (anyv == 50).sum()


# ---- the argument checks of the C entry: refused on the host, before the device is touched -----------------------------------------------
def call(op=3, claim=0, r2=(1.0,), n=1, ws_bytes=1 << 30, values=(1,), box=(0, 1, 0, 3, 0, 3)):
    from medical_sam2_amd import _lib
    L = _lib.lib()
    fake = 1 << 20                                          # never dereferenced: every case below is refused first
    rc = L.msam2_label_morph(fake, 4, 8, 8, (ctypes.c_uint8 * 40)(*values), (ctypes.c_int32 * 240)(*(list(box) * 40)), n, op,
                             (ctypes.c_double * 40)(*r2), 3.0, 0.76, 0.76, claim, 2 * fake, 3 * fake, 4 * fake, ws_bytes, None)
    return rc, L.msam2_last_error().decode()


@pytest.mark.parametrize("kw, text", [
    (dict(op=4), "op 4"), (dict(op=-1), "op -1"), (dict(claim=2), "claim 2"), (dict(r2=(-1.0,)), "r2[0]"), (dict(r2=(float("nan"),)), "r2[0]"), (dict(r2=(float("inf"),)), "r2[0]"),
    (dict(n=33, values=tuple(range(1, 41)), r2=(1.0,) * 40), "n = 33"), (dict(n=0), "n = 0"), (dict(values=(0,)), "values[0] is 0"),
    (dict(n=2, values=(7, 7), r2=(1.0, 1.0)), "both 7"), (dict(box=(0, 4, 0, 3, 0, 3)), "box 0"), (dict(ws_bytes=64), "workspace too small"),
])
def test_bad_arguments_are_refused_on_the_host(kw, text):
    rc, msg = call(**kw)
    assert rc < 0 and "label_morph" in msg and text in msg, msg


def test_workspace_bytes_entry():
    from medical_sam2_amd import _lib
    L = _lib.lib()
    box = (ctypes.c_int32 * 12)(1, 2, 2, 5, 2, 5, 0, 0, 0, 0, 0, 0)
    r2 = (ctypes.c_double * 2)(1.0, 1.0)

    def nb(op, n=1, in_place=0, all_at_once=0, D=4, r=r2):
        return L.msam2_label_morph_workspace_bytes(D, 8, 8, box, n, op, r, 1.0, 1.0, 1.0, in_place, all_at_once)

    r16 = lambda b: (b + 15) // 16 * 16                                                                    # noqa: E731
    # erode: the box grown by one voxel, 4 x 6 x 6 = 144 voxels of 8 + 2 + 1 bytes; dilate: by the ball's extent, the same, 8 + 8 + 2 + 1
    # bytes and 8 per voxel of the volume
    assert nb(0) == 16 + r16(144 * 11) and nb(2) == nb(0)
    assert nb(1) == 16 + 4 * 8 * 8 * 8 + r16(144 * 19)
    assert nb(3) == 16 + 4 * 8 * 8 * 8 + r16(4 * 8 * 8 * 19)                                              # by two voxels: clipped to the volume
    assert nb(0, in_place=1) == nb(0) + 256
    assert nb(0, n=2, all_at_once=1) == nb(0) + r16(2 * 2 * 2 * 11) and nb(0, n=2) == nb(0)
    assert nb(4) == 0 and nb(0, n=33) == 0 and nb(0, D=2) == 0 and nb(0, r=(ctypes.c_double * 2)(-1.0, 1.0)) == 0
