"""msam2_label_components / msam2_label_clean / msam2_label_overlap, their ops wrappers and volume_labels.clean_labels / label_scores on the
MI355X.

Every result is an integer with a canonical definition, so every comparison is exact equality with the scipy restatement
(tests/components_restate.py, itself checked against a flood fill in tests/test_label_components_cpu.py), nothing excluded.  The entries are
called through the C ABI with the volume inside a 0xAB-padded buffer (also one byte off any alignment) and comp, size, out, info and counts
inside sentinel canvases of -7 (0xEE for uint8): an over-read would join or count padding, a stray store is seen.

Borders of the kernels: a wave owns 64 consecutive voxels in raster order through the whole volume, a workgroup 4 rounds of 256, so runs are
cut and neighbour bytes change hands (shuffle -> load) at linear indices that are multiples of 64, 256 and 1024.  The cube fixtures put
their contact on index 1024 (= voxel (0, 10, 24) of a [9, 33, 100] volume) and 7168 (= voxel (2, 5, 68))."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import components_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64


@pytest.fixture(autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with torch.no_grad():
        yield


def padded(x, fill, shift=0):
    """x inside a canvas of `fill`: (canvas, view of x's place).  shift: extra elements in front (1 = an unaligned label volume)."""
    canvas = torch.full((x.numel() + 2 * PAD + shift,), fill, dtype=x.dtype, device=DEV)
    view = canvas[PAD + shift: PAD + shift + x.numel()].view(x.shape)
    return canvas, view


def intact(canvas, view, fill):
    rest = torch.ones_like(canvas, dtype=torch.bool)
    start = (view.data_ptr() - canvas.data_ptr()) // canvas.element_size()
    rest[start: start + view.numel()] = False
    return bool((canvas[rest] == fill).all())


class Abi:
    """one volume on the device, the three entries on padded buffers; everything comes back as int64 numpy"""

    def __init__(self, vol, shift=0, stream=None):
        import medical_sam2_amd.ops as ops
        from medical_sam2_amd import _lib
        self.ops, self.L = ops, _lib.lib()
        self.host = np.ascontiguousarray(vol, dtype=np.uint8)
        self.D, self.H, self.W = self.host.shape
        self.stream = stream
        self.vcan, self.vol = padded(torch.from_numpy(self.host), 0xAB, shift)
        self.vol.copy_(torch.from_numpy(self.host))
        like = torch.empty(self.host.shape, dtype=torch.int32)
        self.ccan, self.comp = padded(like, -7)
        self.scan, self.size = padded(like, -7)
        self.ocan, self.out = padded(torch.from_numpy(self.host), 0xEE, shift)
        nb = self.L.msam2_label_components_workspace_bytes(self.D, self.H, self.W)
        assert nb == 4 * self.host.size
        self.ws = torch.empty(nb // 4, dtype=torch.int32, device=DEV)
        self.cws = torch.empty(self.L.msam2_label_clean_workspace_bytes(32) // 8 + 1, dtype=torch.int64, device=DEV)
        torch.cuda.synchronize()                             # the buffers are ready whichever stream the entries run on

    def _s(self):
        return self.ops._stream() if self.stream is None else self.stream.cuda_stream

    def components(self, conn, sync=True):
        p = self.ops._p
        rc = self.L.msam2_label_components(p(self.vol), self.D, self.H, self.W, conn, p(self.comp), p(self.size), p(self.ws), self.ws.numel() * 4,
                                           self._s())
        assert rc == 0, self.L.msam2_last_error().decode()
        if sync:
            torch.cuda.synchronize()
            assert intact(self.ccan, self.comp, -7) and intact(self.scan, self.size, -7) and intact(self.vcan, self.vol, 0xAB), "stray store"
            return self.comp.cpu().numpy().astype(np.int64), self.size.cpu().numpy().astype(np.int64)

    def clean(self, ids, min_voxels=None, mask=0, in_place=False):
        """on the comp / size the last components() left; in place overwrites (and then restores) the volume"""
        p = self.ops._p
        n = len(ids)
        ids_d = torch.tensor(ids, dtype=torch.uint8, device=DEV)
        mv = None if min_voxels is None else torch.tensor(min_voxels, dtype=torch.int32, device=DEV)
        ican, info = padded(torch.empty(n, 6, dtype=torch.int32), -7)
        out = self.vol if in_place else self.out
        torch.cuda.synchronize()
        rc = self.L.msam2_label_clean(p(self.vol), p(self.comp), p(self.size), p(ids_d), n, p(mv), mask, p(out), p(info), p(self.cws),
                                      self.L.msam2_label_clean_workspace_bytes(n), self.D, self.H, self.W, self._s())
        assert rc == 0, self.L.msam2_last_error().decode()
        torch.cuda.synchronize()
        assert intact(ican, info, -7) and intact(self.vcan, self.vol, 0xAB) and intact(self.ocan, self.out, 0xEE), "stray store"
        assert intact(self.ccan, self.comp, -7) and intact(self.scan, self.size, -7)
        got = out.cpu().numpy().copy()
        if in_place:
            self.vol.copy_(torch.from_numpy(self.host))
        return got, info.cpu().numpy().astype(np.int64)

    def overlap(self, gt, ids):
        p = self.ops._p
        n = len(ids)
        ids_d = torch.tensor(ids, dtype=torch.uint8, device=DEV)
        gcan, g = padded(torch.from_numpy(gt), 0xAB, 1)
        g.copy_(torch.from_numpy(gt))
        kcan, counts = padded(torch.empty(self.D, n, 3, dtype=torch.int32), -7)
        torch.cuda.synchronize()
        rc = self.L.msam2_label_overlap(p(self.vol), p(g), p(ids_d), self.D, self.H, self.W, n, p(counts), self._s())
        assert rc == 0, self.L.msam2_last_error().decode()
        torch.cuda.synchronize()
        assert intact(kcan, counts, -7) and intact(gcan, g, 0xAB) and intact(self.vcan, self.vol, 0xAB), "stray store"
        return counts.cpu().numpy().astype(np.int64)


# ---- fixtures: name -> uint8 volume -------------------------------------------------------------------------------------------------
def two_cubes(shape, b0, shift, side=2):
    """two cubes of one value: the second starts at b0, the first is it moved back by `shift` (side in an axis = a shared face there,
    side in two = an edge, side in three = a corner)"""
    vol = np.zeros(shape, dtype=np.uint8)
    a0 = [b - s for b, s in zip(b0, shift)]
    assert min(a0) >= 0
    vol[tuple(slice(a, a + side) for a in a0)] = 5
    vol[tuple(slice(b, b + side) for b in b0)] = 5
    return vol


def interleaved(shape):
    vol = np.zeros(shape, dtype=np.uint8)
    vol[:, 0::2, :] = 3
    vol[:, 1::2, :] = 4
    return vol


def wraparound(shape):
    """last column of a row and first of the next; last row of a slice and first of the next: never adjacent"""
    D, H, W = shape
    vol = np.zeros(shape, dtype=np.uint8)
    vol[0, 0, W - 1] = vol[0, 1, 0] = 2
    vol[0, H - 1, :] = 6
    vol[1, 0, :] = 6
    vol[1, 2, W - 1] = vol[1, 3, 0] = vol[1, 3, 1] = 9
    return vol


def _cases():
    S = (9, 33, 100)
    yield "one_voxel_1x1x1", np.ones((1, 1, 1), dtype=np.uint8)
    yield "zero_1x1x1", np.zeros((1, 1, 1), dtype=np.uint8)
    yield "full_1x2x2", np.full((1, 2, 2), 255, dtype=np.uint8)
    yield "full_2x3x1024", np.full((2, 3, 1024), 1, dtype=np.uint8)
    yield "full_3x64x64", np.full((3, 64, 64), 17, dtype=np.uint8)
    yield "blobs1_3x64x64", R.ellipsoids((3, 64, 64), 1, 11)[0]
    yield "blobs4_16x128x128", R.ellipsoids((16, 128, 128), 4, 12)[0]
    yield "blobs13_4x256x256", R.ellipsoids((4, 256, 256), 13, 13)[0]
    yield "blobs32_9x33x100", R.ellipsoids(S, 32, 14)[0]
    yield "noise4_9x33x100", R.noise(S, 4, 20)
    yield "noise4_2x5x37", R.noise((2, 5, 37), 4, 21)
    yield "noise4_2x3x1024", R.noise((2, 3, 1024), 4, 22)
    yield "noise4_70x8x16", R.noise((70, 8, 16), 4, 23)
    yield "parity_4x6x8", R.parity_lattice((4, 6, 8))
    yield "parity_9x33x100", R.parity_lattice(S) * 7
    yield "diagonal_9x33x100", R.diagonal_lattice(S)
    yield "diagonal_70x8x16", R.diagonal_lattice((70, 8, 16)) * 3
    yield "interleaved_2x5x37", interleaved((2, 5, 37))
    yield "interleaved_9x33x100", interleaved(S)
    yield "wraparound_2x5x37", wraparound((2, 5, 37))
    yield "wraparound_2x5x1024", wraparound((2, 5, 1024))
    # two cubes: in plane (face, edge), across a slice border (face, edge, corner), and with the contact on a kernel border (see the module text)
    yield "cubes_plane_face", two_cubes(S, (3, 12, 50), (0, 0, 2))
    yield "cubes_plane_face_rows", two_cubes(S, (3, 12, 50), (0, 2, 0))
    yield "cubes_plane_edge", two_cubes(S, (3, 12, 50), (0, 2, 2))
    yield "cubes_plane_edge_other", two_cubes(S, (3, 12, 50), (0, 2, -2))
    yield "cubes_slice_face", two_cubes(S, (4, 12, 50), (2, 0, 0))
    yield "cubes_slice_edge_rows", two_cubes(S, (4, 12, 50), (2, 2, 0))
    yield "cubes_slice_edge_rows_other", two_cubes(S, (4, 12, 50), (2, -2, 0))
    yield "cubes_slice_edge_cols", two_cubes(S, (4, 12, 50), (2, 0, 2))
    yield "cubes_slice_edge_cols_other", two_cubes(S, (4, 12, 50), (2, 0, -2))
    for k, sh in enumerate([(2, 2, 2), (2, 2, -2), (2, -2, 2), (2, -2, -2)]):
        yield f"cubes_slice_corner{k}", two_cubes(S, (4, 12, 50), sh)
    for name, sh in [("face", (0, 0, 2)), ("face_rows", (0, 2, 0)), ("edge", (0, 2, 2)), ("edge_other", (0, 2, -2))]:
        yield f"cubes_border1024_{name}", two_cubes(S, (0, 10, 24), sh)
    for name, sh in [("face", (2, 0, 0)), ("edge_rows", (2, 2, 0)), ("edge_cols", (2, 0, 2)), ("edge_cols_other", (2, 0, -2)), ("corner", (2, 2, 2)),
                     ("corner_other", (2, 2, -2)), ("corner_up", (2, -2, 2))]:
        yield f"cubes_border7168_{name}", two_cubes(S, (2, 5, 68), sh)
    for shape in [S, (2, 3, 1024), (70, 8, 16), (3, 64, 64)]:
        snake = R.serpentine(shape)
        yield "serpentine_%dx%dx%d" % shape, snake
        yield "serpentine_flipped_%dx%dx%d" % shape, np.ascontiguousarray(snake[::-1, ::-1, ::-1])


CASES = dict(_cases())


@functools.lru_cache(maxsize=None)
def reference(name, conn):
    """computed once, shared, never written to"""
    comp, size = R.restate(CASES[name], conn)
    comp.setflags(write=False), size.setflags(write=False)
    return comp, size


def test_the_fixtures_are_what_they_claim():
    assert np.flatnonzero(CASES["cubes_border1024_face"].reshape(-1) == 5).tolist()[:4] == [1022, 1023, 1024, 1025]
    assert (2 * 33 + 5) * 100 + 68 == 7168 and CASES["cubes_border7168_corner"][2, 5, 68] == 5 and CASES["cubes_border7168_corner"][1, 4, 67] == 5
    count = lambda name, conn: R.n_components(reference(name, conn)[1])                                     # noqa: E731
    assert [count("parity_4x6x8", c) for c in (4, 8, 6, 18, 26)] == [96, 4, 96, 1, 1]
    assert count("diagonal_9x33x100", 18) == int(CASES["diagonal_9x33x100"].sum()) and count("diagonal_9x33x100", 26) == 1
    for tag in ("plane", "border1024"):
        assert [count(f"cubes_{tag}_face", c) for c in (4, 8, 6, 18, 26)] == [2, 2, 1, 1, 1]                  # 4 / 8: per slice, 2 slices
        assert [count(f"cubes_{tag}_edge", c) for c in (4, 8, 6, 18, 26)] == [4, 2, 2, 1, 1]
    for tag in ("slice", "border7168"):
        assert [count(f"cubes_{tag}_face", c) for c in (6, 18, 26)] == [1, 1, 1]
        assert [count(f"cubes_{tag}_edge_cols", c) for c in (6, 18, 26)] == [2, 1, 1]
    assert [count("cubes_slice_corner0", c) for c in (6, 18, 26)] == [2, 2, 1] and [count("cubes_border7168_corner", c) for c in (6, 18, 26)] == [2, 2, 1]
    for name in ("serpentine_9x33x100", "serpentine_flipped_9x33x100"):
        assert [count(name, c) for c in (4, 8, 6, 18, 26)] == [9, 9, 1, 1, 1]
    assert [count("interleaved_9x33x100", c) for c in (4, 8, 6, 26)] == [9 * 33, 9 * 33, 33, 33]            # a row meets only itself, through the slices
    many = [count("noise4_9x33x100", c) for c in R.CONNECTIVITIES]
    assert min(many) >= 50 and max(many) >= 5000


@pytest.mark.parametrize("name", list(CASES))
def test_components_equal_the_restatement_through_the_abi(name):
    vol = CASES[name]
    for shift in (0, 1):
        a = Abi(vol, shift)
        for conn in R.CONNECTIVITIES:
            want_comp, want_size = reference(name, conn)
            comp, size = a.components(conn)
            assert np.array_equal(comp, want_comp), (shift, conn, np.argwhere(comp != want_comp)[:4].tolist())
            assert np.array_equal(size, want_size), (shift, conn, np.argwhere(size != want_size)[:4].tolist())


def _tie_volume():
    """value 4: three components of 6 voxels (a tie: the first in raster order is the largest) and one of 5; value 2: two of 1; a 9 is nobody's"""
    vol = np.zeros((3, 9, 70), dtype=np.uint8)
    vol[0, 6, 10:16] = 4
    vol[1, 1, 60:66] = 4
    vol[1, 4:6, 62:65] = 4
    vol[2, 8, 0:5] = 4
    vol[0, 0, 0] = vol[2, 8, 69] = 2
    vol[1, 8, 30:33] = 9
    return vol


CLEAN_CASES = {
    "blobs4_16x128x128": R.ellipsoids((16, 128, 128), 4, 12),
    "blobs13_4x256x256": R.ellipsoids((4, 256, 256), 13, 13),
    "blobs32_9x33x100": R.ellipsoids((9, 33, 100), 32, 14),
    "noise4_9x33x100": (R.noise((9, 33, 100), 4, 20), [3, 1]),                # value 2 is nobody's id
    "ties_3x9x70": (_tie_volume(), [4, 2]),
}


@pytest.mark.parametrize("name", list(CLEAN_CASES))
def test_clean_equals_the_restatement_through_the_abi(name):
    vol, ids = CLEAN_CASES[name]
    n = len(ids)
    assert ids != sorted(ids) and set(np.unique(vol)) - set(ids) - {0}, "ids in non-ascending order, and a value outside them"
    conn = 26 if name != "ties_3x9x70" else 6
    comp, size = R.restate(vol, conn)
    sizes = np.sort(size[size > 0])
    mid, top = int(sizes[len(sizes) // 2]), int(sizes[-1])
    rng = np.random.RandomState(n)
    mixed = int(rng.randint(1, 2 ** n - 1)) if n > 1 else 1
    every = 2 ** n - 1
    settings = [(None, 0), (None, every), ([0] * n, mixed), ([1] * n, 0), ([mid] * n, 0), ([mid] * n, every), ([mid + 1] * n, mixed),
                ([top + 1] * n, 0), ([top + 1] * n, every), (rng.randint(0, mid + 2, n).tolist(), mixed)]
    if n == 32:
        settings.append((None, 2 ** 32 - 1))
    a = Abi(vol, shift=1)
    got_comp, got_size = a.components(conn)
    assert np.array_equal(got_comp, comp) and np.array_equal(got_size, size)
    changed = 0
    for k, (mv, mask) in enumerate(settings):
        want_out, want_info = R.clean(vol, comp, size, ids, mv, mask)
        out, info = a.clean(ids, mv, mask, in_place=bool(k % 2))
        assert np.array_equal(info, want_info), (k, mv, mask, info.tolist(), want_info.tolist())
        assert np.array_equal(out, want_out), (k, mv, mask, np.argwhere(out != want_out)[:4].tolist())
        changed += int((out != vol).any())
    assert changed >= 3
    if name == "ties_3x9x70":
        out, info = a.clean(ids, None, 0b01)
        assert info.tolist() == [[4, 23, 6, 6 * 70 + 10 + 1, 1, 6], [2, 2, 1, 1, 2, 2]] and out[0, 6, 10:16].tolist() == [4] * 6 and (out == 4).sum() == 6
    # out of place twice in a row on the same tables, then in place: the same bits
    first = a.clean(ids, [mid] * n, mixed)
    assert all(np.array_equal(x, y) for x, y in zip(first, a.clean(ids, [mid] * n, mixed))) and \
        all(np.array_equal(x, y) for x, y in zip(first, a.clean(ids, [mid] * n, mixed, in_place=True)))


def test_overlap_equals_the_restatement_and_label_slices():
    import medical_sam2_amd.ops as ops
    # D * n * 3 counters are zeroed 256 per workgroup: 156 and 864 (a remainder), 54, and 64 x 4 x 3 = 768 (three whole workgroups)
    cases = dict(CLEAN_CASES, noise4_64x2x3=(R.noise((64, 2, 3), 4, 30), [1, 2, 3, 4]))
    for name in ("blobs13_4x256x256", "blobs32_9x33x100", "noise4_9x33x100", "noise4_64x2x3"):
        vol, ids = cases[name]
        gt = np.ascontiguousarray(np.roll(vol, (1, 3, -5), axis=(0, 1, 2)))
        gt[gt == ids[0]] = ids[-1]
        for shift in (0, 1):
            counts = Abi(vol, shift).overlap(gt, ids)
            assert np.array_equal(counts, R.overlap(vol, gt, ids)), (name, shift)
    # a volume labelled from integer logits at the logits' own size: label_slices' exclusive counts at threshold 0 are the overlap counts
    T, n, H, W = 5, 6, 37, 52
    g = torch.Generator().manual_seed(3)
    logits = torch.randint(-3, 4, (T, n, H, W), generator=g).float().to(DEV)
    ids = [9, 2, 200, 17, 5, 64]
    gt = torch.tensor(ids + [0, 77], dtype=torch.uint8)[torch.randint(0, n + 2, (T, H, W), generator=g)].to(DEV)
    labels, counts = ops.label_slices(logits, ids, H, W, 0.0, gt=gt, thresholds=[0.0], exclusive=True)
    got = ops.label_overlap(labels, gt, ids)
    assert got.dtype == torch.int32 and got.shape == (T, n, 3) and torch.equal(got, counts[0])
    assert np.array_equal(got.cpu().numpy(), R.overlap(labels.cpu().numpy(), gt.cpu().numpy(), ids)) and int(got[..., 0].sum()) > 0


def test_partition_and_sizes_equal_the_2d_kernel():
    """binary volumes with even H and W at connectivity 8: the same partition as msam2_cc_label slice by slice (its names are 2x2-block
    corners, so the names differ), and the same areas"""
    import medical_sam2_amd.ops as ops
    rng = np.random.RandomState(5)
    for vol in ((rng.rand(6, 64, 96) < 0.45).astype(np.uint8), (R.ellipsoids((5, 128, 128), 3, 8)[0] > 0).astype(np.uint8),
                R.serpentine((4, 34, 100))):
        d = torch.from_numpy(vol).to(DEV)
        comp, size = ops.label_components(d, 8)
        cc, area = ops.connected_components(d[:, None])
        comp, size, cc, area = comp.cpu().numpy().astype(np.int64), size.cpu().numpy().astype(np.int64), cc[:, 0].cpu().numpy(), area[:, 0].cpu().numpy()
        assert np.array_equal(comp > 0, cc > 0)
        fg = comp > 0
        mine = size.reshape(-1)[np.maximum(comp - 1, 0)] * fg                      # every voxel's component size
        assert np.array_equal(mine, area)
        for z in range(vol.shape[0]):
            pairs = np.unique(np.stack([comp[z][fg[z]], cc[z][fg[z]]]), axis=1)
            assert pairs.shape[1] == len(np.unique(pairs[0])) == len(np.unique(pairs[1]))


def test_second_stream_gives_the_same_bits():
    vol, ids = CLEAN_CASES["blobs32_9x33x100"]
    noise = CASES["noise4_9x33x100"]
    side = torch.cuda.Stream()
    runs = [Abi(vol), Abi(vol, shift=1, stream=side), Abi(noise), Abi(noise, shift=1, stream=side)]
    for _ in range(3):                                                              # the two streams' workgroups share the device
        for x in runs:
            x.components(26, sync=False)
    torch.cuda.synchronize()
    for x, name in zip(runs, ["blobs32_9x33x100"] * 2 + ["noise4_9x33x100"] * 2):
        want_comp, want_size = reference(name, 26)
        assert np.array_equal(x.comp.cpu().numpy(), want_comp) and np.array_equal(x.size.cpu().numpy(), want_size)
        assert intact(x.ccan, x.comp, -7) and intact(x.scan, x.size, -7)


def test_graph_capture_and_replay():
    import medical_sam2_amd.ops as ops
    vol, ids = CLEAN_CASES["blobs4_16x128x128"]
    other = np.ascontiguousarray(vol[::-1, :, ::-1])
    labels = torch.from_numpy(vol).to(DEV)
    ids_d = ops.label_ids(ids, DEV)
    mv = torch.tensor([3, 0, 40, 1], dtype=torch.int32, device=DEV)
    e_comp, e_size = ops.label_components(labels, 18)
    e_out, e_info = ops.label_clean(labels, e_comp, e_size, ids_d, mv, [True, False, True, True])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        comp, size = ops.label_components(labels, 18)
        out, info = ops.label_clean(labels, comp, size, ids_d, mv, [True, False, True, True])
    for v in (other, vol):                                                          # the replay reads what the buffers hold now
        labels.copy_(torch.from_numpy(v).to(DEV))
        comp.fill_(-7), size.fill_(-7), out.fill_(0xEE), info.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        want_comp, want_size = R.restate(v, 18)
        want_out, want_info = R.clean(v, want_comp, want_size, ids, [3, 0, 40, 1], 0b1101)
        assert np.array_equal(comp.cpu().numpy(), want_comp) and np.array_equal(size.cpu().numpy(), want_size)
        assert np.array_equal(out.cpu().numpy(), want_out) and np.array_equal(info.cpu().numpy(), want_info)
    assert torch.equal(comp, e_comp) and torch.equal(size, e_size) and torch.equal(out, e_out) and torch.equal(info, e_info)


def test_wrappers_on_the_device():
    import medical_sam2_amd.ops as ops
    from medical_sam2_amd.volume_labels import clean_labels
    vol, ids = CLEAN_CASES["blobs13_4x256x256"]
    labels = torch.from_numpy(vol).to(DEV)
    comp, size = R.restate(vol, 26)
    n = len(ids)
    mv = [5 * (j % 3) for j in range(n)]
    flags = [j % 2 == 0 for j in range(n)]
    want_out, want_info = R.clean(vol, comp, size, ids, mv, ops.label_largest_mask(flags, n))
    out, info = clean_labels(labels, ids, keep_largest=flags, min_voxels=mv)
    assert out.is_cuda and out.dtype == torch.uint8 and info.dtype == torch.int32 and info.shape == (n, 6) and out.data_ptr() != labels.data_ptr()
    assert np.array_equal(out.cpu().numpy(), want_out) and np.array_equal(info.cpu().numpy(), want_info) and torch.equal(labels.cpu(), torch.from_numpy(vol))
    same, _ = clean_labels(labels.clone(), ops.label_ids(ids, DEV), keep_largest=flags, min_voxels=torch.tensor(mv), in_place=True)
    assert torch.equal(same, out)
    # obj_ids = None: 1 .. n, n from the caller; connectivity 8 = slice by slice
    small = torch.from_numpy(np.ascontiguousarray(vol % 4)).to(DEV)
    c8, s8 = R.restate(vol % 4, 8)
    want_out, want_info = R.clean(vol % 4, c8, s8, [1, 2, 3], [2] * 3, 0b111)
    out, info = clean_labels(small, n=3, connectivity=8, min_voxels=2)
    assert np.array_equal(out.cpu().numpy(), want_out) and np.array_equal(info.cpu().numpy(), want_info)
    with pytest.raises(ValueError, match="comp must be int32"):
        ops.label_clean(labels, torch.zeros_like(labels), torch.zeros_like(labels), ids)


def test_end_to_end_cleaned_volume_and_scores():
    """hiera_t at 256^2, seeded weights: segment_volume -> label_volume -> clean_labels (26, keep largest) equals the restatement applied to
    the device's own label volume, and label_scores of the cleaned volume equals volume_scores of the numpy counts"""
    import medical_sam2_amd.build_sam as bs
    import medical_sam2_amd.synthetic as syn
    import medical_sam2_amd.volume as volume_mod
    import medical_sam2_amd.weights as wts
    from medical_sam2_amd.prompts import segment_prompts
    from medical_sam2_amd.volume_labels import clean_labels, label_scores, label_volume, volume_scores
    S, T, n = 256, 4, 2
    m = bs.build_sam2("sam2_hiera_t", device="cpu", hydra_overrides_extra=[f"++model.image_size={S}"])
    m.load_state_dict(wts.init_weights("hiera_t", 0), strict=True)
    m = m.to(DEV).eval()
    volume, _ = syn.blob_volume(3, n_slices=T, size=S, n_objects=n)
    ys, xs = np.mgrid[0:S, 0:S]
    gt = np.zeros((T, S, S), dtype=np.uint8)
    for t in range(T):
        for o in range(n):
            cx, cy, rx, ry = S * (0.3 + 0.35 * o) + 3 * t, S * 0.45 - 5 * t, S * 0.11 + t, S * 0.2 - 2 * o
            gt[t][((xs - cx) / rx) ** 2 + ((ys - cy) / ry) ** 2 <= 1.0] = o + 1
    gt_d = torch.from_numpy(gt).to(DEV)
    masks = volume_mod.segment_volume(m, volume.to(DEV), segment_prompts(gt_d, [1, 2], "bbox", prompt_freq=2), fill_hole_area=8)
    labels = label_volume(masks, S, S, [1, 2])
    host = labels.cpu().numpy()
    assert host.any()
    cleaned, info = clean_labels(labels, [1, 2], connectivity=26, keep_largest=True)
    comp, size = R.restate(host, 26)
    want, want_info = R.clean(host, comp, size, [1, 2], None, 0b11)
    assert np.array_equal(cleaned.cpu().numpy(), want) and np.array_equal(info.cpu().numpy(), want_info)
    assert (want_info[:, 4] <= 1).all() and want_info[:, 0].sum() >= 1
    got = label_scores(cleaned, gt_d, [1, 2])
    ref = volume_scores(R.overlap(want, gt, [1, 2])[None])
    assert sorted(got) == sorted(ref)
    for k in ref:
        assert np.array_equal(np.asarray(got[k]), np.asarray(ref[k]), equal_nan=True), k
