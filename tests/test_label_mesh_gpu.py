"""msam2_label_mesh_count, msam2_label_mesh, ops.label_mesh and volume_labels.organ_meshes on the MI355X.

Every table equals the brute-force restatement (tests/mesh_restate.py) bit for bit: quads and counts as integers, vertices as the int32
views of their float32 values, for placement in {corner, nets} x relax in {0, 1, 3}.  The entries are called through the C ABI with the
label volume inside a buffer padded with 0xAB -- a LISTED, absent id of every case: an over-read gives it vertices -- shifted off its
alignment by 0 and 1, and vertices, quads and counts inside sentinel canvases: a stray store is seen.  The workspace starts as 0x5A bytes:
nothing may rely on zeroes."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64
ABSENT = 0xAB
SPACING, ORIGIN = (3.0, 0.76, 0.76), (-12.5, 0.25, 100.0)
COMBOS = [(p, t) for p in ("corner", "nets") for t in (0, 1, 3)]
PLACEMENT = {"corner": 0, "nets": 1}
# csrc/mesh.hip: a word is the 64 lattice points of a wave; MESH_TILE_WORDS = 256 words make a scan tile; the second level scans 256 tiles per
# trip; MESH_GRID_CAP = 2048 workgroups of 4 waves make a grid-stride trip of 2048 * 4 * 64 = 2^19 lattice points.
WORD, TILE_WORDS, TILES_PER_TRIP, GRID_TRIP = 64, 256, 256, 2048 * 4 * 64
BIG_SHAPE = (64, 256, 256)                                   # 65 x 257 x 257 lattice points > 64 * 256 * 256: a second trip of the second level


@pytest.fixture(autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with torch.no_grad():
        yield


def padded(x, fill, shift=0):
    """x inside a canvas of `fill`: (canvas, view of x's place).  shift: extra elements in front (1 = off every wider alignment)."""
    canvas = torch.full((x.numel() + 2 * PAD + shift,), fill, dtype=x.dtype, device=DEV)
    view = canvas[PAD + shift: PAD + shift + x.numel()].view(x.shape)
    return canvas, view


def intact(canvas, view, fill):
    rest = torch.ones_like(canvas, dtype=torch.bool)
    start = (view.data_ptr() - canvas.data_ptr()) // canvas.element_size()
    rest[start: start + view.numel()] = False
    return bool((canvas[rest] == fill).all())


def tight_boxes(vol, ids):
    boxes = []
    for v in ids:
        nz = np.argwhere(vol == v)
        boxes.append([0] * 6 if len(nz) == 0 else [x for a in range(3) for x in (int(nz[:, a].min()), int(nz[:, a].max()))])
    return boxes


class Abi:
    """one volume on the device in a padded buffer; the two entries on sentinel canvases"""

    def __init__(self, vol, ids, shift=0, boxes=None):
        import medical_sam2_amd.ops as ops
        from medical_sam2_amd import _lib
        self.ops, self.L = ops, _lib.lib()
        self.np_vol, self.ids, self.n = vol, list(ids), len(ids)
        self.D, self.H, self.W = vol.shape
        self.vcan, self.vol = padded(torch.from_numpy(vol), ABSENT, shift)
        self.vol.copy_(torch.from_numpy(vol))
        self.boxes = tight_boxes(vol, ids) if boxes is None else boxes    # boxes: any that hold the organs, tight or not
        torch.cuda.synchronize()

    def count(self):
        ids_d = torch.tensor(self.ids, dtype=torch.uint8, device=DEV)
        can, tab = padded(torch.empty(self.n, 2, dtype=torch.int64), -7)
        rc = self.L.msam2_label_mesh_count(self.vol.data_ptr(), ids_d.data_ptr(), self.D, self.H, self.W, self.n, tab.data_ptr(), self.ops._stream())
        assert rc == 0, self.L.msam2_last_error().decode()
        torch.cuda.synchronize()
        assert intact(can, tab, -7) and intact(self.vcan, self.vol, ABSENT)
        return tab.cpu().numpy()

    def need(self, relax):
        return [self.L.msam2_label_mesh_workspace_bytes((ctypes.c_int32 * 6)(*b), relax) for b in self.boxes]

    def mesh(self, sizes, placement, relax, caps=None, workspace_bytes=None, stream=None, sync=True):
        """sizes: int [n, 2] true (vertices, quads): the segments; caps: [n, 2] capacities (default: the sizes).  -> per organ (vertices
        float32 [cap, 3], quads int32 [cap, 4]) of the segment, and counts [n, 2]"""
        n = self.n
        caps = np.asarray(sizes if caps is None else caps, dtype=np.int64).reshape(n, 2)
        v_off = np.concatenate([[0], np.cumsum(caps[:, 0])]).astype(np.int64)
        q_off = np.concatenate([[0], np.cumsum(caps[:, 1])]).astype(np.int64)
        self.vc, self.v = padded(torch.empty(int(v_off[-1]), 3, dtype=torch.float32), -7.0)
        self.qc, self.q = padded(torch.empty(int(q_off[-1]), 4, dtype=torch.int32), -7)
        self.cc, self.c = padded(torch.empty(n, 2, dtype=torch.int32), -7)
        need = self.need(relax)
        nb = sum(need) if workspace_bytes is None else workspace_bytes
        ws = torch.full(((nb + 15) // 16 * 2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
        torch.cuda.synchronize()
        i64 = lambda rows: (ctypes.c_int64 * n)(*[int(r) for r in rows])                                   # noqa: E731
        s = self.ops._stream() if stream is None else stream.cuda_stream
        rc = self.L.msam2_label_mesh(self.vol.data_ptr(), self.D, self.H, self.W, (ctypes.c_uint8 * n)(*self.ids),
                                     (ctypes.c_int32 * (6 * n))(*[x for b in self.boxes for x in b]), i64(v_off[:-1]), i64(caps[:, 0]),
                                     i64(q_off[:-1]), i64(caps[:, 1]), n, PLACEMENT[placement], relax, (ctypes.c_double * 3)(*SPACING),
                                     (ctypes.c_double * 3)(*ORIGIN), self.v.data_ptr(), self.q.data_ptr(), self.c.data_ptr(), ws.data_ptr(), nb, s)
        assert rc == 0, self.L.msam2_last_error().decode()
        self._offs, self._ws = (v_off, q_off), ws
        if sync:
            torch.cuda.synchronize()
            return self.tables()

    def tables(self):
        assert intact(self.vc, self.v, -7.0) and intact(self.qc, self.q, -7) and intact(self.cc, self.c, -7), "stray store around a table"
        assert intact(self.vcan, self.vol, ABSENT)
        v, q, (v_off, q_off) = self.v.cpu().numpy(), self.q.cpu().numpy(), self._offs
        return [(v[v_off[j]: v_off[j + 1]], q[q_off[j]: q_off[j + 1]]) for j in range(self.n)], self.c.cpu().numpy().astype(np.int64)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
def _touch(kind):
    vol = np.zeros((3, 4, 4) if kind == "edge" else (4, 4, 4), dtype=np.uint8)
    vol[1, 1, 1] = 1
    vol[(1, 2, 2) if kind == "edge" else (2, 2, 2)] = 1
    return vol


def _dense3(shape, seed):
    """label 1 on half of the voxels (nearly every lattice point is a vertex of it), labels 2 and 3 and the background share the rest"""
    rng = np.random.default_rng(seed)
    u = rng.random(shape)
    return np.select([u < 0.5, u < 0.7, u < 0.85], [1, 2, 3], 0).astype(np.uint8)


def _big():
    """blobs of label 1 over the whole volume (its box is the volume: 65 * 257 * 257 = 4 293 185 lattice points = 67 082 words > one tile of
    256 words, > one second-level trip of 256 tiles = 65 536 words, > eight grid-stride trips of 2^19 points), two small noisy organs"""
    vol = R.blobs(BIG_SHAPE, (1, 0, 0), 21, cell=8)
    vol[2:12, 3:15, 5:40] = R.noise((10, 12, 35), (2,), 22)
    vol[50:62, 200:250, 190:256] = R.noise((12, 50, 66), (3, 1), 23)
    return vol


def _cases():
    c = {}
    c["single_1x1x1"] = (np.ones((1, 1, 1), dtype=np.uint8), [1, ABSENT])
    c["noise_1x1x5"] = (R.noise((1, 1, 5), (1, 2), 2, 0.6), [1, ABSENT, 2])
    c["noise_5x1x1"] = (R.noise((5, 1, 1), (1, 2), 3, 0.6), [1, ABSENT, 2])
    c["noise_5x7x67"] = (R.noise((5, 7, 67), (1, 2), 4), [1, ABSENT, 2])            # rows of 68 lattice points cross a wave
    c["noise_3x4x64"] = (R.noise((3, 4, 64), (1, 2), 5), [1, 2, ABSENT])
    c["noise_3x4x65"] = (R.noise((3, 4, 65), (1, 2), 6), [ABSENT, 1, 2])
    c["full_3x4x5"] = (np.full((3, 4, 5), 7, dtype=np.uint8), [7, ABSENT])         # every frame face is present
    c["absent_between_4x6x9"] = (R.noise((4, 6, 9), (4, 9), 7), [4, 5, ABSENT, 9])  # 5 and 0xAB are listed and absent
    vol = np.zeros((3, 4, 6), dtype=np.uint8)
    vol[:, :, :3], vol[:, :, 3:] = 1, 2
    c["adjacent_3x4x6"] = (vol, [1, 2, ABSENT])
    c["unordered_4x5x11"] = (R.noise((4, 5, 11), (1, 2, 3), 8, 0.7), [3, ABSENT, 1, 2])
    c["edge_touch"] = (_touch("edge"), [1, ABSENT])
    c["corner_touch"] = (_touch("corner"), [1, ABSENT])
    c["dense3_9x13x70"] = (_dense3((9, 13, 70), 9), [1, 2, ABSENT, 3])
    c["big_64x256x256"] = (_big(), [1, ABSENT, 2, 3])
    return c


CASES = _cases()
SMALL = [k for k in CASES if not k.startswith("big")]
_REF = {}


def reference(name, placement, relax):
    """per organ the restatement of a case, computed once and shared, read-only"""
    key = (name, placement, relax)
    if key not in _REF:
        vol, ids = CASES[name]
        _REF[key] = [R.organ_mesh(vol, v, SPACING, ORIGIN, placement, relax) for v in ids]
        for r in _REF[key]:
            for t in r.values():
                t.setflags(write=False)
    return _REF[key]


def ref_sizes(name):
    return np.array([[len(r["vertices"]), len(r["quads"])] for r in reference(name, "corner", 0)], dtype=np.int64)


def same_bits(got, ref, what):
    for j, ((v, q), r) in enumerate(zip(got, ref)):
        assert np.array_equal(q, r["quads"]), (what, "quads of organ", j, np.argwhere(q != r["quads"])[:4].tolist())
        gv, rv = np.ascontiguousarray(v).view(np.int32), np.ascontiguousarray(r["vertices"]).view(np.int32)
        assert gv.shape == rv.shape and np.array_equal(gv, rv), (what, "vertices of organ", j, np.argwhere(gv != rv)[:4].tolist())


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("name", SMALL)
def test_tables_equal_the_restatement(name, shift):
    vol, ids = CASES[name]
    abi = Abi(vol, ids, shift)
    sizes = ref_sizes(name)
    assert np.array_equal(abi.count(), sizes)
    for placement, relax in COMBOS:
        got, counts = abi.mesh(sizes, placement, relax)
        assert np.array_equal(counts, sizes), (placement, relax)
        same_bits(got, reference(name, placement, relax), (name, shift, placement, relax))
    for j, v in enumerate(ids):
        if not (vol == v).any():
            assert sizes[j].tolist() == [0, 0], "a listed, absent organ has an empty mesh and shifts nobody's offsets"


@pytest.mark.parametrize("placement,relax", COMBOS)
def test_big_volume_scans_span_tiles_trips_and_grid_strides(placement, relax):
    name = "big_64x256x256"
    vol, ids = CASES[name]
    lattice = np.prod([s + 1 for s in BIG_SHAPE])
    words = (lattice + WORD - 1) // WORD
    assert words > TILE_WORDS * TILES_PER_TRIP and lattice > GRID_TRIP, "organ 1's box is the volume: the scan spans every level"
    abi = Abi(vol, ids, 1)
    assert abi.boxes[0] == [0, BIG_SHAPE[0] - 1, 0, BIG_SHAPE[1] - 1, 0, BIG_SHAPE[2] - 1]
    ref = reference(name, placement, relax)
    sizes = np.array([[len(r["vertices"]), len(r["quads"])] for r in ref], dtype=np.int64)
    if (placement, relax) == COMBOS[0]:
        assert np.array_equal(abi.count(), sizes)
    got, counts = abi.mesh(sizes, placement, relax)
    assert np.array_equal(counts, sizes)
    same_bits(got, ref, (name, placement, relax))


def test_adjacent_organs_share_faces_with_opposite_winding():
    name = "adjacent_3x4x6"
    vol, ids = CASES[name]
    abi = Abi(vol, ids)
    got, _ = abi.mesh(ref_sizes(name), "corner", 0)
    ref = reference(name, "corner", 0)

    def faces(j):
        """quads of organ j as tuples of lattice points, in winding order from the lowest corner"""
        lat = ref[j]["lattice"]
        return {tuple(map(tuple, lat[q])) for q in got[j][1]}

    one, two = faces(0), faces(1)
    mirrored = {(f[0], f[3], f[2], f[1]) for f in one}
    common = mirrored & two
    assert len(common) == 3 * 4, "the 12 faces of the plane x = 3 are in both meshes, wound the other way round"
    assert all(p[2] == 3 for f in common for p in f)
    assert not (one & two)


@pytest.mark.parametrize("name", ["unordered_4x5x11", "dense3_9x13x70", "absent_between_4x6x9"])
def test_one_organ_per_group_gives_the_same_bytes(name):
    vol, ids = CASES[name]
    abi = Abi(vol, ids, 1)
    sizes = ref_sizes(name)
    for placement, relax in (("nets", 0), ("nets", 3)):
        need = abi.need(relax)
        assert sum(need) > max(need) + 16
        got, counts = abi.mesh(sizes, placement, relax, workspace_bytes=max(need) + 16)      # two organs never fit: groups of one
        assert np.array_equal(counts, sizes)
        same_bits(got, reference(name, placement, relax), (name, placement, relax, "groups of one"))


@pytest.mark.parametrize("placement,relax", [("corner", 0), ("nets", 3)])
def test_short_capacity_keeps_the_canonical_prefix(placement, relax):
    name = "dense3_9x13x70"
    vol, ids = CASES[name]
    abi = Abi(vol, ids)
    sizes = ref_sizes(name)
    caps = sizes.copy()
    caps[0] = [sizes[0, 0] // 2, sizes[0, 1] // 3]           # a prefix of both tables
    caps[1] = [0, sizes[1, 1]]                               # no vertex at all
    caps[3] = [sizes[3, 0], 1]                               # one quad
    got, counts = abi.mesh(sizes, placement, relax, caps=caps)
    assert np.array_equal(counts, sizes), "the true counts, whatever fits"
    ref = reference(name, placement, relax)
    cut = [dict(vertices=r["vertices"][:caps[j, 0]], quads=r["quads"][:caps[j, 1]]) for j, r in enumerate(ref)]
    same_bits(got, cut, (name, placement, relax, "short capacity"))


def test_relaunch_on_a_second_stream_gives_the_same_bits():
    name = "dense3_9x13x70"
    vol, ids = CASES[name]
    sizes = ref_sizes(name)
    first, second = Abi(vol, ids), Abi(vol, ids, 1)
    other, side = torch.cuda.Stream(), torch.cuda.Stream()
    busy = torch.randn(1024, 1024, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(4):
            busy = busy @ busy * 1e-3                         # another stream's work beside the relaunch
    first.mesh(sizes, "nets", 3, stream=other, sync=False)
    second.mesh(sizes, "nets", 3, sync=False)
    first.mesh(sizes, "nets", 3, stream=other, sync=False)   # again, into fresh canvases
    torch.cuda.synchronize()
    ref = reference(name, "nets", 3)
    for abi in (first, second):
        got, counts = abi.tables()
        assert np.array_equal(counts, sizes)
        same_bits(got, ref, (name, "second stream"))


@pytest.mark.parametrize("name", ["dense3_9x13x70", "unordered_4x5x11", "full_3x4x5", "noise_5x7x67"])
def test_sizes_through_ops_and_the_faces_of_label_measure(name):
    import medical_sam2_amd.ops as ops
    vol, ids = CASES[name]
    labels = torch.from_numpy(vol).to(DEV)
    sizes = ops.label_mesh_sizes(labels, ids)
    assert sizes.dtype == torch.int64 and sizes.is_cuda and tuple(sizes.shape) == (len(ids), 2)
    assert np.array_equal(sizes.cpu().numpy(), ref_sizes(name))
    faces = ops.label_measure(labels, ids, faces=True)[3]
    assert torch.equal(sizes[:, 1], faces.sum(dim=1)), "one quad per face label_measure counts"


@pytest.mark.parametrize("name", ["absent_between_4x6x9", "dense3_9x13x70"])
def test_ops_label_mesh_and_organ_meshes(name):
    import medical_sam2_amd.ops as ops
    from medical_sam2_amd import volume_labels as VL
    vol, ids = CASES[name]
    labels = torch.from_numpy(vol).to(DEV)
    for placement, relax in (("nets", 0), ("corner", 3)):
        v, q, v_offs, q_offs, counts = ops.label_mesh(labels, ids, SPACING, ORIGIN, placement, relax)
        ref = reference(name, placement, relax)
        got = [(v[v_offs[j]: v_offs[j + 1]].cpu().numpy(), q[q_offs[j]: q_offs[j + 1]].cpu().numpy()) for j in range(len(ids))]
        same_bits(got, ref, (name, placement, relax, "ops"))
        assert np.array_equal(counts.cpu().numpy(), ref_sizes(name))
        meshes = VL.organ_meshes(labels, ids, SPACING, ORIGIN, placement, relax)
        assert list(meshes) == list(ids)
        for j, i in enumerate(ids):
            m = meshes[i]
            assert m.vertices.is_cuda and m.is_closed()
            assert np.array_equal(m.quads.cpu().numpy(), ref[j]["quads"])
            assert m.euler_characteristic() == (R.euler(len(ref[j]["vertices"]), ref[j]["quads"]) if len(ref[j]["quads"]) else 0)
            assert abs(m.area() - R.area(ref[j]["vertices"], ref[j]["quads"])) <= 1e-9 * max(1.0, m.area())
        assert meshes[ABSENT].empty and meshes[ABSENT].vertices.shape == (0, 3) and meshes[ABSENT].area() == 0.0
        mm = VL.mesh_measurements(meshes)
        assert mm["quads"].tolist() == ref_sizes(name)[:, 1].tolist()


def test_corner_mesh_volume_is_the_voxel_volume():
    """The divergence-theorem volume of the "corner" mesh is (voxels) x (voxel volume) in exact arithmetic.  The stored vertices are float32:
    every coordinate is off by at most delta = max |coordinate| 2^-24.  To first order a triangle's a . (b x c) moves by at most
    delta (|b x c|_1 + |c x a|_1 + |a x b|_1); the bound is that sum over the triangles / 6, times 1.01 for the second-order terms and the
    float64 summation (both more than five orders of magnitude below the first-order term)."""
    from medical_sam2_amd import volume_labels as VL
    name = "dense3_9x13x70"
    vol, ids = CASES[name]
    labels = torch.from_numpy(vol).to(DEV)
    spacing = (3.0, 0.76, 0.76)
    meshes = VL.organ_meshes(labels, ids, spacing=spacing, placement="corner")
    voxel = 3.0 * 0.76 * 0.76
    for i in ids:
        m = meshes[i]
        exact = float((vol == i).sum()) * voxel
        if m.empty:
            assert exact == 0.0 and m.volume() == 0.0
            continue
        p = m.xyz().to(torch.float64)
        t = m.triangles().to(torch.int64)
        a, b, c = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]
        delta = float(p.abs().max()) * 2.0 ** -24
        l1 = lambda x: x.abs().sum()                                                                        # noqa: E731
        bound = 1.01 * delta * float(l1(torch.linalg.cross(b, c)) + l1(torch.linalg.cross(c, a)) + l1(torch.linalg.cross(a, b))) / 6.0
        print(i, m.volume(), exact, bound)
        assert abs(m.volume() - exact) <= bound


def test_profiler_names_the_new_kernels():
    import medical_sam2_amd.ops as ops
    from torch.profiler import ProfilerActivity, profile
    vol, ids = CASES["dense3_9x13x70"]
    labels = torch.from_numpy(vol).to(DEV)
    ops.label_mesh(labels, ids, relax=1)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        ops.label_mesh(labels, ids, relax=2)
        torch.cuda.synchronize()
    names = {e.key for e in prof.key_averages()}
    for kernel in ("mesh_count_kernel", "mesh_flag_kernel", "mesh_scan_tiles_kernel", "mesh_scan_sums_kernel", "mesh_emit_kernel",
                   "mesh_relax_kernel", "mesh_store_kernel"):
        assert any(kernel in k for k in names), (kernel, sorted(k for k in names if "kernel" in k))


def slack_boxes(vol, ids):
    """per organ a box that holds it with room to spare: grown by (1, 2, 3) on the low and (2, 0, 5) on the high side, cut at the volume;
    the organ listed last takes the whole volume, an absent one a box in the middle of it"""
    out = []
    for n, (v, b) in enumerate(zip(ids, tight_boxes(vol, ids))):
        if not (vol == v).any():
            out.append([x for s in vol.shape for x in (s // 2, s - 1)])
        elif n == len(ids) - 1:
            out.append([x for s in vol.shape for x in (0, s - 1)])
        else:
            out.append([x for a, (lo, hi) in enumerate(((1, 2), (2, 0), (3, 5))) for x in (max(b[2 * a] - lo, 0), min(b[2 * a + 1] + hi, vol.shape[a] - 1))])
    return out


def _islands():
    """two noisy organs well inside a 7 x 9 x 40 volume, touching each other: their tight boxes leave room on every side"""
    vol = np.zeros((7, 9, 40), dtype=np.uint8)
    vol[2:5, 3:6, 10:30] = R.noise((3, 3, 20), (1,), 31, 0.6)
    vol[1:4, 2:8, 28:36] = R.noise((3, 6, 8), (2, 1), 32, 0.8)
    return vol, [2, ABSENT, 1, 7]


CASES["islands_7x9x40"] = _islands()


@pytest.mark.parametrize("name", ["islands_7x9x40", "absent_between_4x6x9"])
def test_a_looser_box_gives_the_same_tables(name):
    """no byte depends on the box's slack: lattice order is kept and voxels of other values inside the box are not the organ"""
    vol, ids = CASES[name]
    boxes, tight = slack_boxes(vol, ids), tight_boxes(vol, ids)
    assert boxes != tight and (name != "islands_7x9x40" or all(b != t for b, t in zip(boxes, tight)))
    abi = Abi(vol, ids, 1, boxes=boxes)
    sizes = ref_sizes(name)
    for placement, relax in (("corner", 0), ("nets", 0), ("nets", 3)):
        got, counts = abi.mesh(sizes, placement, relax)
        assert np.array_equal(counts, sizes)
        same_bits(got, reference(name, placement, relax), (name, placement, relax, "slack boxes"))


def test_every_listed_organ_absent_gives_empty_meshes():
    """an empty prediction, or ids none of which is in the volume: empty tables and zero counts, not an error"""
    import medical_sam2_amd.ops as ops
    from medical_sam2_amd import volume_labels as VL
    present = torch.from_numpy(CASES["unordered_4x5x11"][0]).to(DEV)          # holds 1, 2, 3
    for labels, ids in ((torch.zeros(3, 4, 5, dtype=torch.uint8, device=DEV), [1, 2]), (present, [5]), (present, [9, ABSENT, 77])):
        for placement, relax in (("nets", 0), ("corner", 2)):
            v, q, v_offs, q_offs, counts = ops.label_mesh(labels, ids, SPACING, ORIGIN, placement, relax)
            assert tuple(v.shape) == (0, 3) and v.dtype == torch.float32 and tuple(q.shape) == (0, 4) and q.dtype == torch.int32
            assert v_offs == [0] * (len(ids) + 1) and q_offs == [0] * (len(ids) + 1)
            assert counts.cpu().tolist() == [[0, 0]] * len(ids)
            meshes = VL.organ_meshes(labels, ids, SPACING, ORIGIN, placement, relax)
            assert list(meshes) == ids
            assert all(m.empty and m.vertices.shape == (0, 3) and m.area() == 0.0 and m.volume() == 0.0 and m.is_closed() for m in meshes.values())
        assert ops.label_mesh_sizes(labels, ids).cpu().tolist() == [[0, 0]] * len(ids)


def test_device_ids_are_the_keys_without_a_second_copy():
    """ids given as a device tensor: the dictionary's keys are the host values that came back with the boxes"""
    import medical_sam2_amd.ops as ops
    from medical_sam2_amd import volume_labels as VL
    name = "absent_between_4x6x9"
    vol, ids = CASES[name]
    labels = torch.from_numpy(vol).to(DEV)
    ids_d = ops.label_ids(ids, DEV)
    meshes = VL.organ_meshes(labels, ids_d, SPACING, ORIGIN, "nets", 1)
    assert list(meshes) == ids and all(isinstance(k, int) for k in meshes)
    ref = reference(name, "nets", 1)
    same_bits([(meshes[i].vertices.cpu().numpy(), meshes[i].quads.cpu().numpy()) for i in ids], ref, (name, "device ids"))
    out = ops.label_mesh_with_values(labels, ids_d, SPACING, ORIGIN, "nets", 1)
    assert len(out) == 6 and out[5] == ids
