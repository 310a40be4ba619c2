"""Hole filling of label volumes, the part that needs no GPU: the restatement the GPU tests compare against (tests/holes_restate.py) is
checked against an independent flood from the frame and against the facts of the definition, the fixtures are shown to be worth running, every
simulated mistake of the list is caught by one of them, and the two C entries and the wrappers refuse bad arguments with their own texts
(host pointers that are never dereferenced, as tests/test_label_contracts_cpu.py does)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import holes_restate as R  # noqa: E402

FIXTURES = R.fixtures()
BY_NAME = {f.name: f for f in FIXTURES}
TINY = [f for f in FIXTURES if f.tiny]


def holes(name, c, **kw):
    f = BY_NAME[name]
    return R.restate(f.vol, f.ids, c, **kw)[1][:, 0].tolist()


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fx", TINY, ids=[f.name for f in TINY])
def test_restatement_equals_a_flood_from_the_frame(fx):
    for c in R.CONNECTIVITIES:
        for claim in R.CLAIMS:
            for mv in (None, fx.max_voxels):
                out, info = R.restate(fx.vol, fx.ids, c, mv, claim)
                f_out, f_info = R.flood(fx.vol, fx.ids, c, mv, claim)
                assert np.array_equal(out, f_out) and np.array_equal(info, f_info), (c, claim, mv)


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------------
def test_the_facts_of_the_definition():
    for c in R.CONNECTIVITIES:
        out, info = R.restate(BY_NAME["shell_closed"].vol, [1], c)
        k = 1 if c in (6, 18, 26) else 3                     # slice by slice the 27 voxels are three holes of 9
        assert info.tolist() == [[k, 27, k, 27]] and (out[1:6, 1:6, 1:6] == 1).all() and out.sum() == 125
    assert [holes("shell_edge_leak", c)[0] for c in (6, 18, 26)] == [1, 0, 0]
    assert [holes("shell_corner_leak", c)[0] for c in (6, 18, 26)] == [1, 1, 0]
    assert [holes("plane_corner_leak", c)[0] for c in (4, 8)] == [3, 2]          # the leak opens its slice for 8 only
    assert [holes("z_tunnel", c)[0] for c in R.CONNECTIVITIES] == [0, 0, 0, 5, 5]
    assert [holes("one_slice", c)[0] for c in R.CONNECTIVITIES] == [0, 0, 0, 1, 1]
    assert [holes("cavity_on_frame", c)[0] for c in R.CONNECTIVITIES] == [0, 0, 0, 2, 2]


def test_size_limit_claim_and_priority():
    fx = BY_NAME["size_limits"]
    out, info = R.restate(fx.vol, fx.ids, 6, fx.max_voxels, "background")
    assert info.tolist() == [[2, 9, 1, 4], [3, 8, 1, 2]]                         # sizes 4 | 5 at limit 4; 2 | 3 | 2 + 1 at limit 2
    assert (out[2, 2, 2:6] == 1).all() and (out[2, 5, 2:7] == 0).all() and (out[2, 2, 17:19] == 2).all() and out[2, 8, 19] == 9
    fx = BY_NAME["enclosed_value"]
    assert R.restate(fx.vol, fx.ids, 6, 27, "background")[1].tolist() == [[1, 27, 1, 24]]     # the three voxels of 9 count and stay
    assert R.restate(fx.vol, fx.ids, 6, 26, "background")[1].tolist() == [[1, 27, 0, 0]]
    assert R.restate(fx.vol, fx.ids, 6, 27, "any")[1].tolist() == [[1, 27, 1, 27]]
    # nested shells A (5) around B (3) around 27 background voxels: the inner background is a hole of both, the position in ids decides
    a, b = BY_NAME["nested_outer_first"], BY_NAME["nested_inner_first"]
    assert R.restate(a.vol, a.ids, 6, None, "background")[1].tolist() == [[1, 125, 1, 27], [1, 27, 1, 0]]
    assert R.restate(b.vol, b.ids, 6, None, "background")[1].tolist() == [[1, 27, 1, 27], [1, 125, 1, 0]]
    assert R.restate(a.vol, a.ids, 6, None, "any")[1].tolist() == [[1, 125, 1, 125], [1, 27, 1, 0]]
    assert R.restate(b.vol, b.ids, 6, None, "any")[1].tolist() == [[1, 27, 1, 27], [1, 125, 1, 98]]
    fx = BY_NAME["absent_and_unordered"]
    assert R.restate(fx.vol, fx.ids, 6)[1].tolist() == [[1, 27, 1, 27], [0, 0, 0, 0], [1, 27, 1, 27]]
    for name in ("one_column", "one_row"):
        fx = BY_NAME[name]
        for c in R.CONNECTIVITIES:
            out, info = R.restate(fx.vol, fx.ids, c)
            assert np.array_equal(out, fx.vol) and not info.any()


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------------
def test_the_fixtures_are_worth_running():
    fx = BY_NAME["random"]
    res = {c: R.restate(fx.vol, fx.ids, c, None, "any") for c in R.CONNECTIVITIES}
    assert res[6][1][:, 0].sum() >= 20
    assert (res[6][0] != res[26][0]).any() and (res[4][0] != res[8][0]).any()
    assert fx.max_voxels == 1
    for c in R.CONNECTIVITIES:                               # holes on both sides of the limit: some qualify, some do not
        info = R.restate(fx.vol, fx.ids, c, fx.max_voxels)[1]
        assert 0 < info[:, 2].sum() < info[:, 0].sum(), c
    fx = BY_NAME["serpentine"]
    assert fx.vol.shape == (4, 96, 160)
    assert R.restate(fx.vol, fx.ids, 6)[1].tolist() == [[1, 2 * (47 * 158 + 46), 1, 2 * (47 * 158 + 46)]]
    assert R.restate(fx.vol, fx.ids, 4)[1][0, 0] == 2


# ---- (d) ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_every_simulated_mistake_is_caught_by_a_fixture(mistake):
    caught = []
    for fx in FIXTURES:
        for c in R.CONNECTIVITIES:
            for claim in R.CLAIMS:
                out, info = R.restate(fx.vol, fx.ids, c, fx.max_voxels, claim)
                w_out, w_info = R.restate(fx.vol, fx.ids, c, fx.max_voxels, claim, mistake=mistake)
                if not (np.array_equal(out, w_out) and np.array_equal(info, w_info)):
                    caught.append((fx.name, c, claim))
    assert caught, mistake


# ---- (e) ----------------------------------------------------------------------------------------------------------------------------------
MSAM2_ERR_ARG = -1
BIG = 1 << 40


def _calls():
    from medical_sam2_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    ptr = (ctypes.addressof(buf) + 15) & ~15
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)                                                         # noqa: E731

    def fill(n=2, D=4, H=6, W=8, ids=None, box=(0, 3, 0, 5, 0, 7), connectivity=6, claim=0, out=ptr + 4096, ws_bytes=BIG, ws=ptr + 8192, labels=ptr):
        m = max(n, 1)
        ids = (ctypes.c_uint8 * m)(*(ids or range(1, m + 1)))
        return L.msam2_label_fill_holes(labels, D, H, W, ids, i32(*(list(box) * m)), n, connectivity, None, claim, out, ptr + 12288, ws, ws_bytes, None)

    def bytes_(n=1, D=4, H=6, W=8, box=(0, 3, 0, 5, 0, 7), connectivity=6, in_place=0, all_at_once=0):
        return L.msam2_label_fill_holes_workspace_bytes(D, H, W, i32(*(list(box) * max(n, 1))), n, connectivity, in_place, all_at_once)

    return L, ptr, fill, bytes_


REFUSALS = [
    (dict(n=0), "label_fill_holes: n = 0 objects (1 .. 32 per call)"),
    (dict(n=33), "label_fill_holes: n = 33 objects (1 .. 32 per call)"),
    (dict(D=0), "label_fill_holes: bad sizes (D 0 of 1 .. 65535, H x W 6x8 of 1 .. 8192, at most 2^31 - 2 voxels)"),
    (dict(D=65536), "label_fill_holes: bad sizes (D 65536 of 1 .. 65535, H x W 6x8 of 1 .. 8192, at most 2^31 - 2 voxels)"),
    (dict(H=0), "label_fill_holes: bad sizes (D 4 of 1 .. 65535, H x W 0x8 of 1 .. 8192, at most 2^31 - 2 voxels)"),
    (dict(W=8193), "label_fill_holes: bad sizes (D 4 of 1 .. 65535, H x W 6x8193 of 1 .. 8192, at most 2^31 - 2 voxels)"),
    (dict(D=33, H=8192, W=8192), "label_fill_holes: bad sizes (D 33 of 1 .. 65535, H x W 8192x8192 of 1 .. 8192, at most 2^31 - 2 voxels)"),
    (dict(connectivity=5), "label_fill_holes: connectivity 5 of the background flood (6, 18 or 26 in 3-D; 4 or 8 slice by slice)"),
    (dict(claim=2), "label_fill_holes: claim 2 (0: background voxels only, 1: any voxel of a hole)"),
    (dict(ids=[3, 0]), "label_fill_holes: ids[1] is 0, the background"),
    (dict(ids=[3, 3]), "label_fill_holes: ids[0] and ids[1] are both 3"),
    (dict(box=(0, 4, 0, 5, 0, 7)), "label_fill_holes: box 0 (0..4, 0..5, 0..7) is inverted or outside the 4 x 6 x 8 volume"),
    (dict(box=(0, 3, 2, 1, 0, 7)), "label_fill_holes: box 0 (0..3, 2..1, 0..7) is inverted or outside the 4 x 6 x 8 volume"),
    (dict(box=(0, 3, 0, 5, -1, 7)), "label_fill_holes: box 0 (0..3, 0..5, -1..7) is inverted or outside the 4 x 6 x 8 volume"),
    (dict(out="labels + 1"), "label_fill_holes: out overlaps labels without being labels"),
    (dict(ws_bytes=16 + 1728 - 1), "label_fill_holes: workspace too small (1743 of 1744 bytes)"),
    (dict(out="labels", ws_bytes=16 + 192 + 1728 - 1), "label_fill_holes: workspace too small (1935 of 1936 bytes)"),
    (dict(ws="ws + 8"), "label_fill_holes: the workspace must be 16-byte aligned, info and max_voxels 4-byte"),
]


@pytest.mark.parametrize("bad, text", REFUSALS, ids=[", ".join("%s=%s" % kv for kv in b.items()) for b, _ in REFUSALS])
def test_refusal_code_and_text(bad, text):
    L, ptr, fill, _ = _calls()
    bad = {k: {"labels": ptr, "labels + 1": ptr + 1, "ws + 8": ptr + 8200}.get(v, v) if isinstance(v, str) else v for k, v in bad.items()}
    rc = fill(**bad)
    assert rc == MSAM2_ERR_ARG, (rc, L.msam2_last_error().decode())
    assert L.msam2_last_error().decode() == text


def test_null_pointers_are_refused():
    L, ptr, fill, _ = _calls()
    for bad in (dict(labels=None), dict(out=None), dict(ws=None)):
        assert fill(**bad) == MSAM2_ERR_ARG
        assert L.msam2_last_error().decode() == "label_fill_holes: null labels / ids / boxes / out / info / workspace"


def test_workspace_bytes():
    _, _, _, nbytes = _calls()
    box = 4 * 6 * 8 * 9                                      # 9 bytes per box voxel: 1728, a multiple of 16
    assert nbytes() == 16 + box
    assert nbytes(in_place=1) == 16 + 192 + box
    assert nbytes(n=3) == 16 + box and nbytes(n=3, all_at_once=1) == 16 + 3 * box
    assert nbytes(box=(1, 3, 1, 3, 1, 3)) == 16 + 256        # 27 voxels: 243 bytes rounded to 16
    # boxes that hold no hole by construction cost nothing: 2 rows, 2 columns; 2 slices only where the flood moves along z
    assert nbytes(box=(0, 3, 0, 1, 0, 7)) == 16 and nbytes(box=(0, 3, 0, 5, 3, 4)) == 16
    assert nbytes(box=(1, 2, 0, 5, 0, 7)) == 16 and nbytes(box=(1, 2, 0, 5, 0, 7), connectivity=4) == 16 + 2 * 6 * 8 * 9
    # refused arguments
    assert nbytes(n=0) == 0 and nbytes(n=33) == 0 and nbytes(D=0) == 0 and nbytes(connectivity=7) == 0 and nbytes(box=(0, 4, 0, 5, 0, 7)) == 0


def test_wrapper_refusals():
    import medical_sam2_amd.ops as ops
    import medical_sam2_amd.volume_labels as VL
    vol = torch.zeros(2, 4, 6, dtype=torch.uint8)
    cases = [
        (lambda: ops.label_fill_holes(vol, [1]), "label_fill_holes: the label volume must be on the GPU"),
        (lambda: ops.label_fill_holes(vol.to(torch.int16), [1]), "label_fill_holes: labels must be a uint8 contiguous [D, H, W] label volume"),
        (lambda: ops.label_fill_holes(vol[0], [1]), "label_fill_holes: labels must be a uint8 contiguous [D, H, W] label volume"),
        (lambda: ops.label_fill_holes(vol, list(range(1, 34))), "label_fill_holes: ids must be 1 .. 32 uint8 label values, got 33"),
        (lambda: ops.label_fill_holes(vol, [0]), "label_slices: ids must be integers in 1 .. 255 (0 is the background)"),
        (lambda: VL.fill_holes(vol, [1]), "label_fill_holes: the label volume must be on the GPU"),
        (lambda: VL.postprocess_labels(vol, [1]), "label_components: the label volume must be on the GPU"),
    ]
    for call, text in cases:
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
    with pytest.raises(AssertionError, match="fill_holes: without obj_ids the number of objects n is needed"):
        VL.fill_holes(vol)
