"""msam2_label_fill_holes, ops.label_fill_holes and volume_labels.fill_holes / postprocess_labels on the MI355X.

Every result is an integer with one definition, so every comparison is exact equality with the scipy restatement (tests/holes_restate.py,
itself checked against a flood from the frame in tests/test_label_holes_cpu.py): out voxel for voxel, info entry for entry, nothing
excluded.  The fixtures are that file's: the shells and their diagonal leaks, tunnel, frame and one-slice cases, nested shells in both
orders, enclosed foreign values, holes on both sides of a per-organ size limit, an absent organ, odd sizes, one-row and one-column volumes,
a serpentine cavity through 93 rows of 160 voxels (rows longer than a wave, a box that is the whole volume, many workgroups) and a random
volume.  The reference of every (fixture, connectivity, limit, claim) is computed once and shared."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import holes_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 4096
FIXTURES = R.fixtures()
BY_NAME = {f.name: f for f in FIXTURES}


@pytest.fixture(autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with torch.no_grad():
        yield


@functools.lru_cache(maxsize=None)
def reference(name, c, limited, claim):
    fx = BY_NAME[name]
    out, info = R.restate(fx.vol, fx.ids, c, fx.max_voxels if limited else None, claim)
    out.setflags(write=False), info.setflags(write=False)
    return out, info


def padded(host, fill, shift=0):
    """the uint8 volume inside a canvas of `fill`: (canvas, view of its place).  shift: extra bytes in front (1 = off any alignment)."""
    canvas = torch.full((host.size + 2 * PAD + shift,), fill, dtype=torch.uint8, device=DEV)
    view = canvas[PAD + shift: PAD + shift + host.size].view(host.shape)
    return canvas, view


def intact(canvas, view, fill):
    rest = torch.ones_like(canvas, dtype=torch.bool)
    start = view.data_ptr() - canvas.data_ptr()
    rest[start: start + view.numel()] = False
    return bool((canvas[rest] == fill).all())


def fill(vol, ids, c, mv=None, claim="background", **kw):
    import medical_sam2_amd.ops as ops
    labels = vol if isinstance(vol, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(vol)).to(DEV)
    out, info = ops.label_fill_holes(labels, ids, c, max_voxels=mv, claim=claim, **kw)
    return out.cpu().numpy(), info.cpu().numpy().astype(np.int64)


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("c", R.CONNECTIVITIES)
@pytest.mark.parametrize("name", [f.name for f in FIXTURES])
def test_equals_the_restatement(name, c):
    fx = BY_NAME[name]
    labels = torch.from_numpy(fx.vol).to(DEV)
    for claim in R.CLAIMS:
        for limited in ((False, True) if fx.max_voxels is not None else (False,)):
            got = fill(labels, fx.ids, c, fx.max_voxels if limited else None, claim)
            want = reference(name, c, limited, claim)
            assert np.array_equal(got[1], want[1]), (claim, limited, got[1].tolist(), want[1].tolist())
            assert np.array_equal(got[0], want[0]), (claim, limited, int((got[0] != want[0]).sum()))
    assert torch.equal(labels.cpu(), torch.from_numpy(fx.vol))                        # the input is left as it was


@pytest.mark.parametrize("c", (6, 26, 8))
@pytest.mark.parametrize("name", ["serpentine", "random", "cavity_on_frame", "odd_sizes"])
def test_nothing_is_read_or_stored_outside_the_volumes(name, c):
    """labels is a view inside a larger buffer whose other bytes are the organ's own value in one run and 0 in another (an over-read would
    close or open a hole), one byte off any alignment in the second; out sits in a canvas of 0xEE, info in one of -7"""
    fx = BY_NAME[name]
    want = reference(name, c, fx.max_voxels is not None, "any")
    for surround, shift in ((fx.ids[0], 0), (0, 1)):
        vcan, labels = padded(fx.vol, surround, shift)
        labels.copy_(torch.from_numpy(fx.vol))
        ocan, out = padded(fx.vol, 0xEE, shift)
        got = fill(labels, fx.ids, c, fx.max_voxels, "any", out=out)
        assert same(got, want), (surround, shift)
        assert intact(ocan, out, 0xEE) and intact(vcan, labels, surround)
        assert torch.equal(labels.cpu(), torch.from_numpy(fx.vol))


def test_info_sits_in_a_sentinel_canvas_through_the_c_abi():
    import medical_sam2_amd.ops as ops
    from medical_sam2_amd import _lib
    L = _lib.lib()
    fx = BY_NAME["size_limits"]
    D, H, W = fx.vol.shape
    n = len(fx.ids)
    labels = torch.from_numpy(fx.vol).to(DEV)
    out = torch.empty_like(labels)
    canvas = torch.full((64,), -7, dtype=torch.int32, device=DEV)
    info = canvas[16: 16 + 4 * n].view(n, 4)
    boxes = (ctypes.c_int32 * (6 * n))(0, 4, 0, 11, 0, 13, 0, 4, 0, 11, 15, 29)
    nb = L.msam2_label_fill_holes_workspace_bytes(D, H, W, boxes, n, 18, 0, 1)
    wcan = torch.full((nb + 2 * PAD,), 0xEE, dtype=torch.uint8, device=DEV)             # (a torch allocation: 512-byte aligned)
    ws = wcan[PAD: PAD + nb]
    mv = torch.tensor(fx.max_voxels, dtype=torch.int32, device=DEV)
    rc = L.msam2_label_fill_holes(labels.data_ptr(), D, H, W, (ctypes.c_uint8 * n)(*fx.ids), boxes, n, 18, mv.data_ptr(), 0, out.data_ptr(),
                                  info.data_ptr(), ws.data_ptr(), nb, ops._stream())
    assert rc == 0, L.msam2_last_error().decode()
    want = reference("size_limits", 18, True, "background")
    assert same((out.cpu().numpy(), info.cpu().numpy()), want)
    assert bool((canvas[:16] == -7).all()) and bool((canvas[16 + 4 * n:] == -7).all()) and intact(wcan, ws, 0xEE)


@pytest.mark.parametrize("name", ["nested_outer_first", "nested_inner_first", "random", "serpentine"])
def test_in_place_gives_the_out_of_place_bytes(name):
    fx = BY_NAME[name]
    for c in (6, 4):
        for claim in R.CLAIMS:
            labels = torch.from_numpy(fx.vol).to(DEV)
            got = fill(labels, fx.ids, c, fx.max_voxels, claim, out=labels)
            assert same(got, reference(name, c, fx.max_voxels is not None, claim)), (c, claim)
            assert np.array_equal(labels.cpu().numpy(), got[0])


@pytest.mark.parametrize("shift", (0, 1))
def test_in_place_on_an_odd_volume_inside_a_guarded_buffer(shift):
    """5 x 6 x 7 = 210 bytes, no multiple of 16, as labels AND out: the snapshot is copied 16 bytes at a time and its last two bytes singly
    (shift 0), or byte by byte from an odd address (shift 1); the canvas around the volume keeps its 0xEE on both sides"""
    fx = BY_NAME["odd_sizes"]
    want = reference("odd_sizes", 6, fx.max_voxels is not None, "any")
    canvas, labels = padded(fx.vol, 0xEE, shift)
    labels.copy_(torch.from_numpy(fx.vol))
    got = fill(labels, fx.ids, 6, fx.max_voxels, "any", out=labels)
    assert same(got, want) and np.array_equal(labels.cpu().numpy(), want[0])
    assert intact(canvas, labels, 0xEE)


@pytest.mark.parametrize("name", ["random", "size_limits", "absent_and_unordered", "nested_inner_first"])
def test_workspace_budget(name):
    """a budget that holds one box at a time gives the same result; one below the largest box raises and names the needed size"""
    from medical_sam2_amd import _lib
    L = _lib.lib()
    fx = BY_NAME[name]
    D, H, W = fx.vol.shape
    needs = []
    for v in fx.ids:
        z, y, x = np.nonzero(fx.vol == v)
        if len(z):
            box = (ctypes.c_int32 * 6)(z.min(), z.max(), y.min(), y.max(), x.min(), x.max())
            needs.append((L.msam2_label_fill_holes_workspace_bytes(D, H, W, box, 1, 6, 0, 0), v))
    largest, v = max(needs)
    for claim in R.CLAIMS:
        assert same(fill(fx.vol, fx.ids, 6, fx.max_voxels, claim, workspace_bytes=largest), reference(name, 6, fx.max_voxels is not None, claim))
    with pytest.raises(ValueError) as e:
        fill(fx.vol, fx.ids, 6, workspace_bytes=largest - 1)
    assert f"needs a workspace of {largest} bytes" in str(e.value) and f"workspace_bytes is {largest - 1}" in str(e.value)


def test_a_call_beside_another_streams_work_gives_the_same_bits():
    import medical_sam2_amd.ops as ops
    side = torch.cuda.Stream()
    names = ["random", "serpentine"]
    vols = {k: torch.from_numpy(BY_NAME[k].vol).to(DEV) for k in names}
    big = torch.from_numpy(np.tile(BY_NAME["random"].vol, (4, 4, 4))).to(DEV)
    torch.cuda.synchronize()
    results = []
    for _ in range(2):
        for k in names:
            fx = BY_NAME[k]
            ops.label_components(big, 26)                                              # the two streams' workgroups share the device
            with torch.cuda.stream(side):
                results.append((k, ops.label_fill_holes(vols[k], fx.ids, 6, max_voxels=fx.max_voxels, claim="any")))
            ops.label_fill_holes(big, BY_NAME["random"].ids, 26)
    torch.cuda.synchronize()
    for k, (out, info) in results:
        assert same((out.cpu().numpy(), info.cpu().numpy()), reference(k, 6, BY_NAME[k].max_voxels is not None, "any")), k


def test_max_voxels_forms():
    fx = BY_NAME["size_limits"]
    want = reference("size_limits", 6, True, "background")
    assert same(fill(fx.vol, fx.ids, 6, list(fx.max_voxels)), want)
    assert same(fill(fx.vol, fx.ids, 6, torch.tensor(fx.max_voxels, dtype=torch.int32, device=DEV)), want)
    assert same(fill(fx.vol, fx.ids, 6, torch.tensor(fx.max_voxels, dtype=torch.int64)), want)
    for m in (2, 4):
        assert same(fill(fx.vol, fx.ids, 6, m), R.restate(fx.vol, fx.ids, 6, m))
    assert same(fill(fx.vol, fx.ids, 6, 0), fill(fx.vol, fx.ids, 6, None))
    ids_d = torch.tensor(fx.ids, dtype=torch.uint8, device=DEV)                       # ids as a device tensor
    assert same(fill(fx.vol, ids_d, 6, fx.max_voxels), want)


def test_fill_holes_and_postprocess_labels_are_the_composition():
    import medical_sam2_amd.ops as ops
    import medical_sam2_amd.volume_labels as VL
    fx = BY_NAME["random"]
    labels = torch.from_numpy(fx.vol).to(DEV)
    for c, claim, mv in ((6, "background", 0), (8, "any", [1, 0, 3])):
        out, info = VL.fill_holes(labels, fx.ids, c, mv, claim)
        e_out, e_info = ops.label_fill_holes(labels, fx.ids, c, max_voxels=mv or None, claim=claim)
        assert torch.equal(out, e_out) and torch.equal(info, e_info)
        assert same((out.cpu().numpy(), info.cpu().numpy()), R.restate(fx.vol, fx.ids, c, mv, claim))
    out, info = VL.fill_holes(labels, None, n=3)                                      # ids 1 .. n
    assert same((out.cpu().numpy(), info.cpu().numpy()), R.restate(fx.vol, [1, 2, 3], 6))
    # clean first, then fill what the cleaned volume encloses
    cleaned, c_info = VL.clean_labels(labels, fx.ids, 18, True, 2)
    e_out, e_info = ops.label_fill_holes(cleaned, fx.ids, 6, max_voxels=5, claim="any")
    for in_place in (False, True):
        work = labels.clone()
        out, ci, hi = VL.postprocess_labels(work, fx.ids, 18, True, 2, hole_connectivity=6, max_voxels=5, claim="any", in_place=in_place)
        assert torch.equal(out, e_out) and torch.equal(ci, c_info) and torch.equal(hi, e_info)
        assert torch.equal(work, e_out if in_place else labels)
    assert same((e_out.cpu().numpy(), e_info.cpu().numpy()), R.restate(cleaned.cpu().numpy(), fx.ids, 6, 5, "any"))
