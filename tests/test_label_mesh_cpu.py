"""Surface meshes of label volumes without a GPU: the known answers and properties of the restatement (tests/mesh_restate.py),
`meshes.OrganMesh` on CPU tensors built from it, the three file formats through a minimal reader, and the argument refusals of the three
entries through the C ABI.  The bars on the ball's areas are bars on the restatement: the GPU tables equal it bit for bit
(tests/test_label_mesh_gpu.py), so there is no GPU tolerance."""
import ctypes
import math
import os
import struct
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_restate as R  # noqa: E402


def _box():
    vol = np.zeros((4, 5, 6), dtype=np.uint8)
    vol[1:3, 1:4, 1:5] = 1
    return vol


def _edge_touch():
    vol = np.zeros((3, 4, 4), dtype=np.uint8)
    vol[1, 1, 1] = vol[1, 2, 2] = 1
    return vol


def _corner_touch():
    vol = np.zeros((4, 4, 4), dtype=np.uint8)
    vol[1, 1, 1] = vol[2, 2, 2] = 1
    return vol


def _single333():
    vol = np.zeros((3, 3, 3), dtype=np.uint8)
    vol[1, 1, 1] = 1
    return vol


# name -> (volume, V - E + F of the corner mesh or None)
FIXTURES = {
    "single_1x1x1": (np.ones((1, 1, 1), dtype=np.uint8), 2),
    "single_3x3x3": (_single333(), 2),
    "box_2x3x4": (_box(), 2),
    "ring": (R.ring(), 0),
    "edge_touch": (_edge_touch(), 3),
    "corner_touch": (_corner_touch(), 3),      # two cubes sharing one vertex: 15 - 24 + 12
    "full": (np.ones((3, 4, 5), dtype=np.uint8), 2),
    "noise": (R.noise((6, 7, 9), (1,), 1), None),
}


def face_counts(vol, v=1):
    """the six columns of label_measure's faces row, summed: interior faces per axis plus the frame's"""
    m = np.pad(vol == v, 1)
    return int(sum((np.diff(m.astype(np.int8), axis=a) != 0).sum() for a in range(3)))


@pytest.mark.parametrize("name", list(FIXTURES))
@pytest.mark.parametrize("placement", ["corner", "nets"])
def test_restatement_properties(name, placement):
    vol, chi = FIXTURES[name]
    r = R.organ_mesh(vol, 1, placement=placement)
    nv, q = len(r["vertices"]), r["quads"]
    assert R.is_closed(q), "every directed edge must be matched by its reverse"
    assert q.dtype == np.int32 and r["vertices"].dtype == np.float32
    assert len(q) == face_counts(vol)
    assert (q >= 0).all() and (q < nv).all() and len(np.unique(q)) == nv, "every vertex is a corner of a quad and the other way round"
    if chi is not None:
        assert R.euler(nv, q) == chi
    lat = r["lattice"]
    idx = (lat[:, 0] * (vol.shape[1] + 1) + lat[:, 1]) * (vol.shape[2] + 1) + lat[:, 2]
    assert (np.diff(idx) > 0).all(), "vertices in ascending lattice index"
    assert (r["u"] >= lat - 1).all() and (r["u"] <= lat).all(), "a vertex lies in its cell"
    if placement == "corner":
        assert R.volume(r["vertices"], q) == float((vol == 1).sum()), "divergence theorem on the voxel-face surface (exact in these sizes)"
        assert R.area(r["vertices"], q) == float(len(q)), "unit spacing: one unit of area per face"


def test_single_voxel_known_answer():
    for vol, centre in ((FIXTURES["single_1x1x1"][0], 0.0), (FIXTURES["single_3x3x3"][0], 1.0)):
        r = R.organ_mesh(vol, 1, placement="nets")
        assert len(r["u"]) == 8 and len(r["quads"]) == 6
        expect = np.array([[centre + s * (1.0 / 6.0) for s in signs] for signs in
                           [(a, b, c) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)]])
        assert np.allclose(r["u"], expect, rtol=0, atol=1e-15), "the cube of side 1/3 around the voxel's centre"
        assert abs(R.volume(r["vertices"], r["quads"]) - 1.0 / 27.0) < 1e-6
        c = R.organ_mesh(vol, 1, placement="corner")
        assert np.array_equal(np.sort(np.unique(c["u"])), [centre - 0.5, centre + 0.5])


def test_quad_winding_and_order():
    """one voxel: six quads ordered by (q0, axis), each wound so that its normal looks out"""
    r = R.organ_mesh(FIXTURES["single_3x3x3"][0], 1, placement="corner")
    p = r["vertices"].astype(np.float64)[:, ::-1]
    for q in r["quads"]:
        n = np.cross(p[q[1]] - p[q[0]], p[q[3]] - p[q[0]])
        centre = p[q].mean(axis=0)
        assert np.dot(n, centre - 1.0) > 0
    # keys 3 index(q0) + a of the six faces of voxel (1, 1, 1) in a 4 x 4 x 4 lattice
    idx = lambda k, j, i: (k * 4 + j) * 4 + i                                                               # noqa: E731
    keys = sorted([3 * idx(1, 1, 1) + 0, 3 * idx(1, 1, 1) + 1, 3 * idx(1, 1, 1) + 2, 3 * idx(2, 1, 1) + 0, 3 * idx(1, 2, 1) + 1, 3 * idx(1, 1, 2) + 2])
    lat = r["lattice"]
    got = []
    for q in r["quads"]:
        c = lat[q]
        q0 = c.min(axis=0)
        a = int(np.flatnonzero((c.max(axis=0) - q0) == 0)[0])
        got.append(3 * idx(*q0) + a)
        assert np.array_equal(lat[q[0]], q0), "a quad starts at its lowest corner"
    assert got == keys


@pytest.mark.parametrize("name", ["box_2x3x4", "ring", "edge_touch", "noise"])
@pytest.mark.parametrize("placement", ["corner", "nets"])
def test_relaxed_vertices_stay_in_their_cells(name, placement):
    vol = FIXTURES[name][0]
    base = R.organ_mesh(vol, 1, placement=placement)
    for t in (1, 3, 64):
        r = R.organ_mesh(vol, 1, placement=placement, relax=t)
        assert np.array_equal(r["quads"], base["quads"]) and np.array_equal(r["lattice"], base["lattice"])
        assert (r["u"] >= r["lattice"] - 1).all() and (r["u"] <= r["lattice"]).all()
        assert np.isfinite(r["u"]).all()


def test_spacing_and_origin():
    vol = FIXTURES["box_2x3x4"][0]
    sp, og = (3.0, 0.76, 0.76), (-100.5, 12.25, 7.0)
    r = R.organ_mesh(vol, 1, spacing=sp, origin=og, placement="corner")
    expect = ((r["u"] * np.array(sp)) + np.array(og)).astype(np.float32)
    assert np.array_equal(r["vertices"], expect)
    vol_mm3 = R.volume((r["vertices"].astype(np.float64) - np.array(og)), r["quads"])
    assert abs(vol_mm3 - 24 * 3.0 * 0.76 * 0.76) < 1e-3


def test_ball_areas():
    """radius 6 in 16^3: relaxed < nets < corner, and the net within 5 % of 4 pi r^2 (measured: 460.6 against 452.4, 1.8 %)"""
    ball = R.ball(16, 6.0)
    area = {}
    for key, placement, relax in (("corner", "corner", 0), ("nets", "nets", 0), ("relaxed", "nets", 3)):
        r = R.organ_mesh(ball, 1, placement=placement, relax=relax)
        area[key] = R.area(r["vertices"], r["quads"])
    exact = 4.0 * math.pi * 36.0
    print(area, exact)
    assert area["relaxed"] < area["nets"] < area["corner"]
    assert abs(area["nets"] - exact) <= 0.05 * exact
    assert area["corner"] == 672.0


# ---- OrganMesh on CPU tensors ------------------------------------------------------------------------------------------------------------
def _organ_mesh(vol, **kw):
    from medical_sam2_amd.meshes import OrganMesh
    r = R.organ_mesh(vol, 1, **kw)
    return OrganMesh(torch.from_numpy(r["vertices"]), torch.from_numpy(r["quads"])), r


@pytest.mark.parametrize("name", list(FIXTURES))
def test_organ_mesh_figures(name):
    vol, _ = FIXTURES[name]
    for kw in (dict(placement="corner"), dict(placement="nets", spacing=(3.0, 0.76, 0.76), origin=(1.0, -2.0, 3.0), relax=2)):
        mesh, r = _organ_mesh(vol, **kw)
        assert abs(mesh.area() - R.area(r["vertices"], r["quads"])) <= 1e-9 * max(1.0, mesh.area())
        assert abs(mesh.volume() - R.volume(r["vertices"], r["quads"])) <= 1e-9 * max(1.0, abs(mesh.volume()))
        assert mesh.euler_characteristic() == R.euler(len(r["vertices"]), r["quads"])
        assert mesh.is_closed() and R.is_closed(r["quads"])
        assert np.array_equal(mesh.triangles().numpy(), R.triangles(r["quads"]).astype(np.int32))
        assert np.array_equal(mesh.xyz().numpy(), r["vertices"][:, ::-1])


def test_organ_mesh_open_and_empty():
    from medical_sam2_amd.meshes import OrganMesh
    mesh, r = _organ_mesh(FIXTURES["box_2x3x4"][0], placement="corner")
    assert not OrganMesh(mesh.vertices, mesh.quads[1:]).is_closed()
    empty = OrganMesh(torch.zeros(0, 3), torch.zeros(0, 4, dtype=torch.int32))
    assert empty.area() == 0.0 and empty.volume() == 0.0 and empty.is_closed() and empty.euler_characteristic() == 0
    assert empty.triangles().shape == (0, 3)


def read_stl(path):
    raw = open(path, "rb").read()
    (nt,) = struct.unpack("<I", raw[80:84])
    assert len(raw) == 84 + 50 * nt, "binary STL: 84 + 50 bytes per triangle"
    rec = np.frombuffer(raw[84:], dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("attr", "<u2")]))
    return nt, rec["n"].copy(), rec["v"].copy()


def read_obj(path):
    v, f = [], []
    for line in open(path):
        t = line.split()
        if t and t[0] == "v":
            v.append([float(x) for x in t[1:]])
        elif t and t[0] == "f":
            f.append([int(x) - 1 for x in t[1:]])
    return np.array(v, dtype=np.float32).reshape(-1, 3), np.array(f, dtype=np.int32).reshape(-1, 4)


def read_ply(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode("ascii").split("\n")
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    nv = int([h for h in head if h.startswith("element vertex")][0].split()[-1])
    nf = int([h for h in head if h.startswith("element face")][0].split()[-1])
    assert len(raw) == end + 12 * nv + 17 * nf, "PLY: 12 bytes per vertex, 17 per quad"
    v = np.frombuffer(raw[end: end + 12 * nv], dtype="<f4").reshape(nv, 3)
    faces = np.frombuffer(raw[end + 12 * nv:], dtype=np.dtype([("k", "u1"), ("v", "<i4", 4)]))
    assert (faces["k"] == 4).all()
    return v.copy(), faces["v"].copy()


@pytest.mark.parametrize("name", ["single_1x1x1", "ring", "noise"])
def test_files_round_trip(name, tmp_path):
    mesh, r = _organ_mesh(FIXTURES[name][0], placement="nets", spacing=(3.0, 0.76, 0.76), origin=(0.5, -7.0, 11.0), relax=1)
    xyz, quads = r["vertices"][:, ::-1], r["quads"]
    v, f = read_obj(mesh.save(str(tmp_path / "m.obj")))
    assert np.array_equal(v.view(np.int32), np.ascontiguousarray(xyz).view(np.int32)) and np.array_equal(f, quads)
    v, f = read_ply(mesh.save(str(tmp_path / "m.ply")))
    assert np.array_equal(v.view(np.int32), np.ascontiguousarray(xyz).view(np.int32)) and np.array_equal(f, quads)
    nt, normals, corners = read_stl(mesh.save(str(tmp_path / "m.stl")))
    tri = R.triangles(quads)
    assert nt == 2 * len(quads) == len(tri)
    assert np.array_equal(corners.view(np.int32), np.ascontiguousarray(xyz[tri]).view(np.int32))
    p = xyz[tri].astype(np.float64)
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    length = np.linalg.norm(n, axis=1)
    ok = length > 0
    assert np.allclose(normals[ok], n[ok] / length[ok, None], atol=1e-6) and np.allclose(np.linalg.norm(normals[ok], axis=1), 1.0, atol=1e-6)
    with pytest.raises(AssertionError):
        mesh.save(str(tmp_path / "m.off"))


def test_empty_mesh_files(tmp_path):
    from medical_sam2_amd.meshes import OrganMesh
    empty = OrganMesh(torch.zeros(0, 3), torch.zeros(0, 4, dtype=torch.int32))
    assert read_stl(empty.save(str(tmp_path / "e.stl")))[0] == 0
    assert read_ply(empty.save(str(tmp_path / "e.ply")))[1].shape == (0, 4)
    assert read_obj(empty.save(str(tmp_path / "e.obj")))[0].shape == (0, 3)


def test_mesh_measurements_on_cpu_meshes():
    from medical_sam2_amd.volume_labels import mesh_measurements
    from medical_sam2_amd.meshes import OrganMesh
    mesh, r = _organ_mesh(FIXTURES["box_2x3x4"][0], placement="corner", spacing=(2.0, 1.0, 0.5))
    empty = OrganMesh(torch.zeros(0, 3), torch.zeros(0, 4, dtype=torch.int32))
    m = mesh_measurements({3: mesh, 9: empty})
    assert m["ids"] == [3, 9] and m["volume_mm3"][1] == 0.0 and m["area_mm2"][1] == 0.0
    assert abs(m["volume_mm3"][0] - 24.0) < 1e-9 and abs(m["volume_ml"][0] - 0.024) < 1e-12
    # faces of the 2 x 3 x 4 box: 2 (3 x 4) of 1 x 0.5, 2 (2 x 4) of 2 x 0.5, 2 (2 x 3) of 2 x 1
    assert abs(m["area_mm2"][0] - (24 * 0.5 + 16 * 1.0 + 12 * 2.0)) < 1e-9
    assert m["vertices"].tolist() == [len(r["vertices"]), 0] and m["quads"].tolist() == [52, 0]


# ---- the refusals of the three entries, through the C ABI, without a GPU -----------------------------------------------------------------------
def test_mesh_argument_errors_cross_the_abi_as_codes():
    from medical_sam2_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)                  # a valid, 16-byte alignable host address: never dereferenced by the checks
    ptr = (ctypes.addressof(buf) + 15) & ~15
    u8 = lambda *v: (ctypes.c_uint8 * len(v))(*v)                                                           # noqa: E731
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)                                                          # noqa: E731
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)                                                          # noqa: E731
    f64 = lambda *v: (ctypes.c_double * len(v))(*v)                                                         # noqa: E731
    box, one, zero = i32(0, 3, 0, 3, 0, 3), i64(1), i64(0)
    big = 1 << 30
    need0, need1 = L.msam2_label_mesh_workspace_bytes(box, 0), L.msam2_label_mesh_workspace_bytes(box, 1)

    def mesh(D=4, H=4, W=4, ids=u8(1), boxes=box, v_off=zero, v_cap=one, q_off=zero, q_cap=one, k=1, placement=1, relax=0, spacing=f64(1, 1, 1),
             origin=f64(0, 0, 0), ws=ptr, ws_bytes=big, vertices=ptr):
        return L.msam2_label_mesh(ptr, D, H, W, ids, boxes, v_off, v_cap, q_off, q_cap, k, placement, relax, spacing, origin, vertices, ptr, ptr, ws,
                                  ws_bytes, None)

    # (call, a fragment only that refusal's message holds)
    cases = {
        "count: objects": (lambda: L.msam2_label_mesh_count(ptr, ptr, 4, 4, 4, 33, ptr, None), "label_mesh_count: n = 33 objects"),
        "count: sizes": (lambda: L.msam2_label_mesh_count(ptr, ptr, 0, 4, 4, 1, ptr, None), "label_mesh_count: bad sizes (D 0 of"),
        "count: null": (lambda: L.msam2_label_mesh_count(ptr, None, 4, 4, 4, 1, ptr, None), "label_mesh_count: null labels / ids / counts"),
        "count: voxels": (lambda: L.msam2_label_mesh_count(ptr, ptr, 65535, 8192, 8192, 1, ptr, None), "label_mesh_count: bad sizes (D 65535 of"),
        "count: alignment": (lambda: L.msam2_label_mesh_count(ptr, ptr, 4, 4, 4, 1, ptr + 4, None), "counts must be 8-byte aligned"),
        "placement": (lambda: mesh(placement=2), "label_mesh: placement 2 (0: corner, 1: nets)"),
        "relax above": (lambda: mesh(relax=65), "label_mesh: relax = 65 sweeps (0 .. 64)"),
        "relax below": (lambda: mesh(relax=-1), "label_mesh: relax = -1 sweeps"),
        "spacing zero": (lambda: mesh(spacing=f64(1, 0, 1)), "label_mesh: spacing (1, 0, 1)"),
        "spacing nan": (lambda: mesh(spacing=f64(1, float("nan"), 1)), "label_mesh: spacing (1, nan, 1)"),
        "origin inf": (lambda: mesh(origin=f64(0, float("inf"), 0)), "label_mesh: origin (0, inf, 0) must be finite"),
        "origin nan": (lambda: mesh(origin=f64(0, 0, float("nan"))), "label_mesh: origin (0, 0, nan) must be finite"),
        "box outside": (lambda: mesh(boxes=i32(0, 4, 0, 3, 0, 3)), "label_mesh: box 0 (0..4, 0..3, 0..3) is inverted or outside the 4 x 4 x 4 volume"),
        "box inverted": (lambda: mesh(boxes=i32(2, 1, 0, 3, 0, 3)), "label_mesh: box 0 (2..1, 0..3, 0..3) is inverted"),
        "id zero": (lambda: mesh(ids=u8(0)), "label_mesh: ids[0] is 0, the background"),
        "id twice": (lambda: mesh(ids=u8(5, 5), boxes=i32(*([0, 3] * 6)), v_off=i64(0, 0), v_cap=i64(1, 1), q_off=i64(0, 0), q_cap=i64(1, 1), k=2),
                     "label_mesh: ids[0] and ids[1] are both 5"),
        "capacity": (lambda: mesh(v_cap=i64(-1)), "label_mesh: organ 0: negative offset or capacity (vertices 0 + -1, quads 0 + 1)"),
        "offset": (lambda: mesh(q_off=i64(-4)), "label_mesh: organ 0: negative offset or capacity (vertices 0 + 1, quads -4 + 1)"),
        "sizes": (lambda: mesh(D=65536), "label_mesh: bad sizes (D 65536 of"),
        "voxels": (lambda: mesh(D=65535, H=8192, W=8192), "at most 2^31 - 2 voxels"),
        "objects": (lambda: mesh(k=33), "label_mesh: n = 33 objects"),
        "workspace": (lambda: mesh(ws_bytes=need0 - 1), f"label_mesh: workspace too small ({need0 - 1} of {need0} bytes)"),
        "workspace relax": (lambda: mesh(relax=1, ws_bytes=need0), f"label_mesh: workspace too small ({need0} of {need1} bytes)"),
        "alignment": (lambda: mesh(ws=ptr + 8), "label_mesh: the workspace must be 16-byte aligned"),
        "null": (lambda: mesh(vertices=None), "label_mesh: null labels / ids / boxes"),
        "lattice": (lambda: mesh(D=8, H=8192, W=8192, boxes=i32(0, 7, 0, 8191, 0, 8191)),      # 9 x 8193^2 > 2^29
                    f"label_mesh: box 0 has {9 * 8193 * 8193} lattice points (at most 2^29)"),
    }
    for what, (call, fragment) in cases.items():
        rc = call()
        msg = L.msam2_last_error().decode()
        assert rc < 0, (what, rc)
        assert fragment in msg, (what, fragment, msg)


def test_mesh_workspace_bytes_formula():
    from medical_sam2_amd import _lib
    L = _lib.lib()
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)                                                          # noqa: E731
    r16 = lambda b: (b + 15) // 16 * 16                                                                     # noqa: E731
    TILE_WORDS = 256                                         # csrc/mesh.hip MESH_TILE_WORDS
    for box in ((0, 0, 0, 0, 0, 0), (2, 5, 0, 6, 3, 69), (0, 63, 0, 255, 0, 255)):
        lattice = (box[1] - box[0] + 2) * (box[3] - box[2] + 2) * (box[5] - box[4] + 2)
        words = (lattice + 63) // 64
        tiles = (words + TILE_WORDS - 1) // TILE_WORDS
        base = r16(lattice) + r16(8 * words) + 2 * r16(4 * words) + 2 * r16(4 * tiles)
        assert L.msam2_label_mesh_workspace_bytes(i32(*box), 0) == base
        assert L.msam2_label_mesh_workspace_bytes(i32(*box), 3) == base + 2 * r16(24 * lattice)
    assert L.msam2_label_mesh_workspace_bytes(i32(1, 0, 0, 0, 0, 0), 0) == 0
    assert L.msam2_label_mesh_workspace_bytes(i32(0, 0, 0, 0, 0, 0), 65) == 0
    assert L.msam2_label_mesh_workspace_bytes(i32(0, 1023, 0, 1023, 0, 1023), 0) == 0        # 1025^3 > 2^29 lattice points
    assert L.msam2_label_mesh_workspace_bytes(None, 0) == 0
