"""msam2_label_morph, ops.label_morph and volume_labels.morph_labels on the MI355X.

Every result is an integer with one definition, so every comparison is exact equality with the restatement (tests/morph_restate.py, itself
checked against scipy and the thresholded distance transform in tests/test_label_morph_cpu.py): out voxel for voxel, info entry for entry,
nothing excluded.  The fixtures are that file's; the reference of every (fixture, op, spacing, radius, claim) is computed once and shared."""
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
import morph_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 4096
FIXTURES = R.fixtures()
BY_NAME = {f.name: f for f in FIXTURES}
CT = R.SPACINGS[1]                                           # (3, 0.76, 0.76)


@pytest.fixture(autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with torch.no_grad():
        yield


def radii(fx, ri):
    """(keyword, value as the interface takes it, one r2 per organ)"""
    kind, value = fx.radii[ri]
    r2 = R.r2_of(kind, value)
    return kind, value, r2 if np.ndim(value) else r2 * len(fx.ids)


@functools.lru_cache(maxsize=None)
def sets(name, op, si, ri):
    fx = BY_NAME[name]
    return R.result_sets(fx.vol, fx.ids, op, radii(fx, ri)[2], R.SPACINGS[si])


@functools.lru_cache(maxsize=None)
def reference(name, op, si, ri, claim):
    fx = BY_NAME[name]
    if op in ("erode", "open") and claim != R.CLAIMS[0]:
        return reference(name, op, si, ri, R.CLAIMS[0])      # claim has no say there
    out, info = R.write_back(fx.vol, fx.ids, sets(name, op, si, ri), op, R.SPACINGS[si], claim)
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


def morph(vol, fx, op, si, ri, claim="background", ids=None, **kw):
    import medical_sam2_amd.ops as ops
    labels = vol if isinstance(vol, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(vol)).to(DEV)
    kind, value, _ = radii(fx, ri)
    out, info = ops.label_morph(labels, fx.ids if ids is None else ids, op, spacing=R.SPACINGS[si], claim=claim, **{kind: value}, **kw)
    return out.cpu().numpy(), info.cpu().numpy().astype(np.int64)


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def every(fx):
    for si in range(len(R.SPACINGS)):
        for ri in range(len(fx.radii)):
            for claim in R.CLAIMS:
                yield si, ri, claim


@pytest.mark.parametrize("op", R.OPS)
@pytest.mark.parametrize("name", [f.name for f in FIXTURES])
def test_equals_the_restatement(name, op):
    fx = BY_NAME[name]
    labels = torch.from_numpy(fx.vol).to(DEV)
    for si, ri, claim in every(fx):
        got = morph(labels, fx, op, si, ri, claim)
        want = reference(name, op, si, ri, claim)
        assert np.array_equal(got[1], want[1]), (si, ri, claim, got[1].tolist(), want[1].tolist())
        assert np.array_equal(got[0], want[0]), (si, ri, claim, int((got[0] != want[0]).sum()))
    assert torch.equal(labels.cpu(), torch.from_numpy(fx.vol))                        # the input is left as it was


@pytest.mark.parametrize("op", R.OPS)
@pytest.mark.parametrize("name", ["blobs_7x24x40", "six_faces", "long_row_3x5x200", "two_columns_4x30x2", "odd_5x11x67"])
def test_nothing_is_read_or_stored_outside_the_volumes(name, op):
    """labels is a view inside a larger buffer whose other bytes are the organ's own value in one run and 0 in another (an over-read would
    feed a dilation or an erosion), one byte off any alignment in the second; out sits in a canvas of 0xEE"""
    fx = BY_NAME[name]
    ri = len(fx.radii) - 1
    for si, (surround, shift) in ((1, (fx.ids[0], 0)), (0, (0, 1))):
        want = reference(name, op, si, ri, "any")
        vcan, labels = padded(fx.vol, surround, shift)
        labels.copy_(torch.from_numpy(fx.vol))
        ocan, out = padded(fx.vol, 0xEE, shift)
        got = morph(labels, fx, op, si, ri, "any", out=out)
        assert same(got, want), (surround, shift)
        assert np.array_equal(out.cpu().numpy(), want[0])
        assert intact(ocan, out, 0xEE) and intact(vcan, labels, surround)
        assert torch.equal(labels.cpu(), torch.from_numpy(fx.vol))


def tight_boxes(fx):
    boxes = []
    for v in fx.ids:
        z, y, x = np.nonzero(fx.vol == v)
        boxes.append([z.min(), z.max(), y.min(), y.max(), x.min(), x.max()] if len(z) else [0, 0, 0, 0, 0, 0])
    return boxes


@pytest.mark.parametrize("op", R.OPS)
@pytest.mark.parametrize("name", ["blobs_7x24x40", "lesion_and_absent"])
def test_c_abi_in_sentinel_canvases_and_with_boxes_of_any_slack(name, op):
    """info in a canvas of -7, the workspace in one of 0xEE; tight boxes, boxes with slack on some sides, and the whole volume as every
    organ's box give the same bytes"""
    import medical_sam2_amd.ops as ops
    from medical_sam2_amd import _lib
    L = _lib.lib()
    fx = BY_NAME[name]
    D, H, W = fx.vol.shape
    n = len(fx.ids)
    si, ri = 1, 1
    r2 = (ctypes.c_double * n)(*radii(fx, ri)[2])
    sz, sy, sx = R.SPACINGS[si]
    labels = torch.from_numpy(fx.vol).to(DEV)
    tight = tight_boxes(fx)
    slack = [[max(b[0] - 1, 0), b[1], b[2], min(b[3] + 5, H - 1), max(b[4] - 9, 0), min(b[5] + 2, W - 1)] for b in tight]
    whole = [[0, D - 1, 0, H - 1, 0, W - 1]] * n
    for claim in (0, 1):
        want = reference(name, op, si, ri, R.CLAIMS[claim])
        for boxes in (tight, slack, whole):
            flat = (ctypes.c_int32 * (6 * n))(*[int(v) for b in boxes for v in b])
            out = torch.empty_like(labels)
            canvas = torch.full((64,), -7, dtype=torch.int32, device=DEV)
            info = canvas[16: 16 + 4 * n].view(n, 4)
            nb = L.msam2_label_morph_workspace_bytes(D, H, W, flat, n, R.OPS.index(op), r2, sz, sy, sx, 0, 1)
            assert nb > 0
            wcan = torch.full((nb + 2 * PAD,), 0xEE, dtype=torch.uint8, device=DEV)     # (a torch allocation: 512-byte aligned)
            ws = wcan[PAD: PAD + nb]
            rc = L.msam2_label_morph(labels.data_ptr(), D, H, W, (ctypes.c_uint8 * n)(*fx.ids), flat, n, R.OPS.index(op), r2, sz, sy, sx, claim,
                                     out.data_ptr(), info.data_ptr(), ws.data_ptr(), nb, ops._stream())
            assert rc == 0, L.msam2_last_error().decode()
            assert same((out.cpu().numpy(), info.cpu().numpy()), want), (claim, boxes is tight, boxes is whole)
            assert bool((canvas[:16] == -7).all()) and bool((canvas[16 + 4 * n:] == -7).all()) and intact(wcan, ws, 0xEE)


@pytest.mark.parametrize("name", ["blobs_7x24x40", "facing_plates", "bridge_and_speck", "organs32"])
def test_in_place_gives_the_out_of_place_bytes(name):
    fx = BY_NAME[name]
    for op in R.OPS:
        for claim in R.CLAIMS:
            labels = torch.from_numpy(fx.vol).to(DEV)
            got = morph(labels, fx, op, 1, 1, claim, out=labels)
            assert same(got, reference(name, op, 1, 1, claim)), (op, claim)
            assert np.array_equal(labels.cpu().numpy(), got[0])


@pytest.mark.parametrize("shift", (0, 1))
def test_in_place_on_an_odd_volume_inside_a_guarded_buffer(shift):
    """5 x 11 x 67 = 3685 bytes, no multiple of 16, as labels AND out: the snapshot is copied 16 bytes at a time and its last five bytes
    singly (shift 0), or byte by byte from an odd address (shift 1); the canvas around the volume keeps its 0xEE on both sides"""
    name = "odd_5x11x67"
    fx = BY_NAME[name]
    ri = len(fx.radii) - 1
    for op in ("erode", "close"):
        want = reference(name, op, 1, ri, "any")
        canvas, labels = padded(fx.vol, 0xEE, shift)
        labels.copy_(torch.from_numpy(fx.vol))
        got = morph(labels, fx, op, 1, ri, "any", out=labels)
        assert same(got, want) and np.array_equal(labels.cpu().numpy(), want[0]), op
        assert intact(canvas, labels, 0xEE), op


@pytest.mark.parametrize("op", R.OPS)
@pytest.mark.parametrize("name", ["blobs_7x24x40", "facing_plates", "lesion_and_absent", "organs32"])
def test_workspace_budget(name, op):
    """a budget that holds one box at a time gives the same result; one below the largest box raises and names the needed size"""
    from medical_sam2_amd import _lib
    L = _lib.lib()
    fx = BY_NAME[name]
    D, H, W = fx.vol.shape
    si, ri = 2, 1
    sz, sy, sx = R.SPACINGS[si]
    needs = [L.msam2_label_morph_workspace_bytes(D, H, W, (ctypes.c_int32 * 6)(*[int(v) for v in b]), 1, R.OPS.index(op), (ctypes.c_double * 1)(r),
                                                 sz, sy, sx, 0, 0) for b, r in zip(tight_boxes(fx), radii(fx, ri)[2])]
    largest = max(needs)
    for claim in R.CLAIMS:
        assert same(morph(fx.vol, fx, op, si, ri, claim, workspace_bytes=largest), reference(name, op, si, ri, claim)), claim
    with pytest.raises(ValueError) as e:
        morph(fx.vol, fx, op, si, ri, workspace_bytes=largest - 1)
    assert f"needs a workspace of {largest} bytes" in str(e.value) and f"workspace_bytes is {largest - 1}" in str(e.value)


def test_a_call_beside_another_streams_work_gives_the_same_bits():
    import medical_sam2_amd.ops as ops
    side = torch.cuda.Stream()
    names = ["blobs_7x24x40", "facing_plates"]
    vols = {k: torch.from_numpy(BY_NAME[k].vol).to(DEV) for k in names}
    big = torch.from_numpy(np.tile(BY_NAME["blobs_7x24x40"].vol, (4, 4, 4))).to(DEV)
    torch.cuda.synchronize()
    results = []
    for _ in range(2):
        for k in names:
            fx = BY_NAME[k]
            for op in ("close", "dilate", "open"):
                ops.label_components(big, 26)                                          # the two streams' workgroups share the device
                with torch.cuda.stream(side):
                    results.append((k, op, ops.label_morph(vols[k], fx.ids, op, radius=3.2, spacing=CT, claim="any")))
                ops.label_morph(big, BY_NAME["blobs_7x24x40"].ids, "close", radius=3.2, spacing=CT)
    torch.cuda.synchronize()
    for k, op, (out, info) in results:
        assert same((out.cpu().numpy(), info.cpu().numpy()), reference(k, op, 1, 1, "any")), (k, op)


def test_morph_labels_is_label_morph():
    import medical_sam2_amd.ops as ops
    import medical_sam2_amd.volume_labels as VL
    fx = BY_NAME["blobs_7x24x40"]
    labels = torch.from_numpy(fx.vol).to(DEV)
    for op, claim in (("close", "background"), ("dilate", "any"), ("open", "background"), ("erode", "any")):
        out, info = VL.morph_labels(labels, fx.ids, op, 3.2, CT, claim)
        e_out, e_info = ops.label_morph(labels, fx.ids, op, radius=3.2, spacing=CT, claim=claim)
        assert torch.equal(out, e_out) and torch.equal(info, e_info)
        assert same((out.cpu().numpy(), info.cpu().numpy()), reference(fx.name, op, 1, 1, claim))
    out, info = VL.morph_labels(labels, None, n=3, spacing=CT, radius=3.2)            # ids 1 .. n, the default op: close
    assert same((out.cpu().numpy(), info.cpu().numpy()), R.restate(fx.vol, [1, 2, 3], "close", R.r2_of("radius", 3.2)[0], CT))
    ids_d = torch.tensor(fx.ids, dtype=torch.uint8, device=DEV)                       # ids as a device tensor; radius2 wins over radius
    out, info = VL.morph_labels(labels, ids_d, "dilate", radius2=2.0, spacing=CT)
    assert same((out.cpu().numpy(), info.cpu().numpy()), reference(fx.name, "dilate", 1, 0, "background"))
    work = labels.clone()
    out, info = VL.morph_labels(work, fx.ids, "open", 3.2, CT, in_place=True)
    assert out.data_ptr() == work.data_ptr() and same((work.cpu().numpy(), info.cpu().numpy()), reference(fx.name, "open", 1, 1, "background"))
    with pytest.raises(ValueError):
        ops.label_morph(labels, fx.ids, "close", radius=1.0, radius2=1.0)
    with pytest.raises(ValueError):
        ops.label_morph(labels, fx.ids, "shut", radius=1.0)
