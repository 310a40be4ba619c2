"""Surface meshes of organs: what `volume_labels.organ_meshes` returns, its figures and its files.

An `OrganMesh` holds two views of the tables `ops.label_mesh` filled (csrc/mesh.hip): vertices float32 [nv, 3] with rows
(z, y, x) in physical units like every table of the label-volume chain, and quads int32 [nq, 4] of the organ's own vertex numbers, wound so
that the normals look out of the organ.  The mesh is closed and consistently oriented whatever the organ looks like (every directed edge
is matched by its reverse, also where surfaces touch along an edge), so area and enclosed volume are plain sums over its triangles, the two
(0, 1, 2), (0, 2, 3) of every quad.  The figures run in torch float64 / int64 on the device the tables live on; `save` copies the mesh to
the host once and writes binary STL, OBJ or binary little-endian PLY with vertices in (x, y, z)."""
from __future__ import annotations

import os
import struct

import numpy as np
import torch


class OrganMesh:
    def __init__(self, vertices: torch.Tensor, quads: torch.Tensor):
        assert vertices.dim() == 2 and vertices.shape[1] == 3 and vertices.dtype == torch.float32, "OrganMesh: vertices must be float32 [nv, 3]"
        assert quads.dim() == 2 and quads.shape[1] == 4 and quads.dtype == torch.int32, "OrganMesh: quads must be int32 [nq, 4]"
        self.vertices, self.quads = vertices, quads

    def __repr__(self) -> str:
        return f"OrganMesh({self.vertices.shape[0]} vertices, {self.quads.shape[0]} quads, {self.vertices.device})"

    @property
    def empty(self) -> bool:
        return self.quads.shape[0] == 0

    def triangles(self) -> torch.Tensor:
        """int32 [2 nq, 3]: (0, 1, 2) and (0, 2, 3) of every quad, quad by quad"""
        return self.quads[:, [0, 1, 2, 0, 2, 3]].reshape(-1, 3)

    def xyz(self) -> torch.Tensor:
        """float32 [nv, 3] with the columns reordered to (x, y, z), the frame the windings are right-handed in"""
        return self.vertices.flip(1)

    def _corners(self):
        p, t = self.xyz().to(torch.float64), self.triangles().to(torch.int64)
        return p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]

    def area(self) -> float:
        """surface area in the squared unit of the spacing: half the norms of the triangles' cross products"""
        if self.empty:
            return 0.0
        a, b, c = self._corners()
        return float(0.5 * torch.linalg.cross(b - a, c - a).norm(dim=1).sum())

    def volume(self) -> float:
        """enclosed volume in the cubed unit of the spacing by the divergence theorem: sum of a . (b x c) / 6 over the triangles"""
        if self.empty:
            return 0.0
        a, b, c = self._corners()
        return float((a * torch.linalg.cross(b, c)).sum() / 6.0)

    def _directed_edges(self) -> torch.Tensor:
        q = self.quads.to(torch.int64)
        return torch.cat([torch.stack([q[:, e], q[:, (e + 1) % 4]], dim=1) for e in range(4)])

    def is_closed(self) -> bool:
        """every directed edge (s -> t) occurs as often as (t -> s): closed and consistently oriented, non-manifold edges included"""
        if self.empty:
            return True
        e, n = self._directed_edges(), self.vertices.shape[0]
        forward, backward = (e[:, 0] * n + e[:, 1]).sort().values, (e[:, 1] * n + e[:, 0]).sort().values
        return bool(torch.equal(forward, backward))

    def euler_characteristic(self) -> int:
        """V - E + F with E the distinct undirected edges and F the quads"""
        if self.empty:
            return int(self.vertices.shape[0])
        e, n = self._directed_edges(), self.vertices.shape[0]
        keys = torch.minimum(e[:, 0], e[:, 1]) * n + torch.maximum(e[:, 0], e[:, 1])
        return int(self.vertices.shape[0]) - int(torch.unique(keys).numel()) + int(self.quads.shape[0])

    def save(self, path: str) -> str:
        """binary STL (.stl, triangles with their own normals), Wavefront OBJ (.obj, quads) or binary little-endian PLY (.ply, quads)"""
        ext = os.path.splitext(path)[1].lower()
        assert ext in WRITERS, f"OrganMesh.save: {path!r}: the extension must be one of {tuple(WRITERS)}"
        xyz = self.xyz().cpu().numpy().astype(np.float32)
        WRITERS[ext](path, np.ascontiguousarray(xyz), self.quads.cpu().numpy().astype(np.int32))
        return path


# ---- writers: pure numpy, vertices float32 [nv, 3] in (x, y, z), quads int32 [nq, 4] --------------------------------------------------------
def _triangles(quads: np.ndarray) -> np.ndarray:
    return quads[:, [0, 1, 2, 0, 2, 3]].reshape(-1, 3)


def write_stl(path: str, xyz: np.ndarray, quads: np.ndarray) -> None:
    """80-byte header, uint32 triangle count, then per triangle 12 float32 (normal, three corners) and a uint16 0: 84 + 50 nt bytes"""
    t = _triangles(quads)
    rec = np.zeros(len(t), dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("attr", "<u2")]))
    if len(t):
        p = xyz[t].astype(np.float64)
        nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        length = np.linalg.norm(nrm, axis=1, keepdims=True)
        rec["n"] = np.where(length > 0.0, nrm / np.where(length > 0.0, length, 1.0), 0.0)
        rec["v"] = xyz[t]
    with open(path, "wb") as f:
        f.write(b"binary STL, surface nets of a label volume".ljust(80, b" "))
        f.write(struct.pack("<I", len(t)))
        f.write(rec.tobytes())


def write_obj(path: str, xyz: np.ndarray, quads: np.ndarray) -> None:
    """`v x y z` with 9 significant digits (float32 round trips), `f a b c d` with 1-based indices"""
    with open(path, "w") as f:
        f.write(f"# {len(xyz)} vertices, {len(quads)} quads\n")
        f.write("".join(f"v {float(x):.9g} {float(y):.9g} {float(z):.9g}\n" for x, y, z in xyz))
        f.write("".join(f"f {a + 1} {b + 1} {c + 1} {d + 1}\n" for a, b, c, d in quads.tolist()))


def write_ply(path: str, xyz: np.ndarray, quads: np.ndarray) -> None:
    """binary_little_endian 1.0: float32 x y z per vertex, then (uint8 4, four int32) per face"""
    header = ("ply\nformat binary_little_endian 1.0\ncomment surface nets of a label volume\n"
              f"element vertex {len(xyz)}\nproperty float x\nproperty float y\nproperty float z\n"
              f"element face {len(quads)}\nproperty list uchar int vertex_indices\nend_header\n")
    faces = np.zeros(len(quads), dtype=np.dtype([("k", "u1"), ("v", "<i4", 4)]))
    faces["k"], faces["v"] = 4, quads
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(xyz.astype("<f4").tobytes())
        f.write(faces.tobytes())


WRITERS = {".stl": write_stl, ".obj": write_obj, ".ply": write_ply}
