"""msam2_label_error_clicks, ops.label_error_clicks and prompts.corrective_clicks / worst_slices on the MI355X.

Every result is an integer, so every comparison is exact equality with the brute-force restatement (tests/clicks_restate.py) on every entry
of the table, nothing excluded.  The entry is called through the C ABI with both volumes inside 0xAB-padded buffers (one of them one byte off
any alignment: an over-read would see a value that is nobody's id where the frame should be) and the table and the workspace inside sentinel
canvases: a stray store is seen."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clicks_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64
MODES = {"center": 0, "uniform": 1}


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


def device_table(kind, table):
    """a k or u table [D, n] of integers as the int32 device tensor the entry reads (u: the same 32 bits)"""
    t = np.ascontiguousarray(table, dtype=np.int64)
    t = t if kind == "k" else t - (t >= 2 ** 31) * 2 ** 32
    t = torch.from_numpy(t.astype(np.int32)).to(DEV)
    torch.cuda.synchronize()
    return t


class Abi:
    """two volumes on the device, the entry on padded buffers; the table comes back as int64 numpy"""

    def __init__(self, pred, gt, ids, shift=(0, 1), stream=None):
        import medical_sam2_amd.ops as ops
        from medical_sam2_amd import _lib
        self.ops, self.L = ops, _lib.lib()
        self.D, self.H, self.W = pred.shape
        self.n = len(ids)
        self.stream = stream
        self.pcan, self.pred = padded(torch.from_numpy(pred), 0xAB, shift[0])
        self.gcan, self.gt = padded(torch.from_numpy(gt), 0xAB, shift[1])
        self.pred.copy_(torch.from_numpy(pred))
        self.gt.copy_(torch.from_numpy(gt))
        self.ids = torch.tensor(ids, dtype=torch.uint8, device=DEV)
        self.tcan, self.table = padded(torch.empty(self.D, self.n, 8, dtype=torch.int32), -7)
        self.ws = {}
        for mode, m in MODES.items():
            nb = self.L.msam2_label_error_clicks_workspace_bytes(self.D, self.H, self.W, self.n, m)
            assert nb > 0 and nb % 4 == 0
            self.ws[mode] = padded(torch.empty(nb // 8 + 1, dtype=torch.int64), -7) + (nb,)   # PAD int64 in front: 8-byte aligned
        torch.cuda.synchronize()                             # the buffers are ready whichever stream the entry runs on

    def run(self, mode="center", kind=None, table=None, sync=True):
        p = self.ops._p
        t = None if kind is None else (table if isinstance(table, torch.Tensor) else device_table(kind, table))
        wcan, ws, nb = self.ws[mode]
        s = self.ops._stream() if self.stream is None else self.stream.cuda_stream
        rc = self.L.msam2_label_error_clicks(p(self.pred), p(self.gt), p(self.ids), p(t) if kind == "k" else None, p(t) if kind == "u" else None,
                                             self.D, self.H, self.W, self.n, MODES[mode], p(self.table), p(ws), nb, s)
        assert rc == 0, self.L.msam2_last_error().decode()
        if sync:
            return self.result(mode)

    def result(self, mode):
        torch.cuda.synchronize()
        wcan, ws, _ = self.ws[mode]
        assert intact(self.tcan, self.table, -7) and intact(wcan, ws, -7), "stray store"
        assert intact(self.pcan, self.pred, 0xAB) and intact(self.gcan, self.gt, 0xAB)
        return self.table.cpu().numpy().astype(np.int64)


CASES = list(R.cases())


def _where(got, ref):
    return np.argwhere(got != ref)[:4].tolist()


@pytest.mark.parametrize("name,pred,gt,ids", CASES, ids=[c[0] for c in CASES])
def test_equal_to_the_restatement_through_the_abi(name, pred, gt, ids):
    ref = R.reference(name, pred, gt, ids)
    counts = ref[..., 3:5].sum(-1)
    choices = R.k_choices(counts, seed=len(name))
    ref_u = {c: R.table(pred, gt, ids, "uniform", **{kind: t}) for c, (kind, t) in choices.items()}
    assert np.array_equal(ref_u["u_zero"], ref_u["first"]) and np.array_equal(ref_u["u_max"], ref_u["last"])
    for shift in ((0, 1), (1, 0)):
        a = Abi(pred, gt, ids, shift)
        got = a.run()
        assert np.array_equal(got, ref), (shift, _where(got, ref))
        assert (got[counts == 0] == [-1, -1, -1, 0, 0, 0, 0, 0]).all()
        for c, (kind, t) in choices.items():
            got = a.run("uniform", kind, t)
            assert np.array_equal(got, ref_u[c]), (shift, c, _where(got, ref_u[c]))
            assert (got[counts == 0] == [-1, -1, -1, 0, 0, -1, -1, 0]).all()
    if name.startswith("equal"):
        assert (ref[..., 2] == -1).all()


def test_chunking_does_not_change_the_tables():
    from medical_sam2_amd.prompts import corrective_clicks, worst_slices
    name, pred, gt, ids = next(c for c in CASES if c[0] == "blobs_5x37x65")
    ref = R.reference(name, pred, gt, ids)
    counts = ref[..., 3:5].sum(-1)
    u = R.k_choices(counts, 5)["u_random"][1]
    ref_u = R.table(pred, gt, ids, "uniform", u=u)
    p, g = torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV)
    for step in (1, 2, 5, 8):
        points, labels, errors = corrective_clicks(p, g, ids, slices_per_call=step)
        assert points.is_cuda and points.dtype == torch.float32 and points.shape == (5, 3, 1, 2)
        assert labels.dtype == torch.int32 and labels.shape == (5, 3, 1) and errors.dtype == torch.int32 and errors.shape == (5, 3, 2)
        assert np.array_equal(points.cpu().numpy()[:, :, 0], ref[..., :2].astype(np.float32)), step
        assert np.array_equal(labels.cpu().numpy()[..., 0], ref[..., 2]) and np.array_equal(errors.cpu().numpy(), ref[..., 3:5]), step
        pu, lu, eu = corrective_clicks(p, g, ids, "uniform", u=torch.from_numpy(u).to(torch.uint32), slices_per_call=step)
        assert np.array_equal(pu.cpu().numpy()[:, :, 0], ref_u[..., :2].astype(np.float32)) and np.array_equal(lu.cpu().numpy()[..., 0], ref_u[..., 2])
        assert torch.equal(eu, errors)
    # the generator's stream: the same seed gives the same voxels, every drawn voxel is an error voxel of its object with the region's label
    draw = [corrective_clicks(p, g, ids, "uniform", generator=torch.Generator(device=DEV).manual_seed(s)) for s in (1, 1, 2)]
    assert torch.equal(draw[0][0], draw[1][0]) and not torch.equal(draw[0][0], draw[2][0])
    with pytest.raises(AssertionError, match="generator on cpu"):
        corrective_clicks(p, g, ids, "uniform", generator=torch.Generator())
    xy, lab = draw[0][0].cpu().numpy()[:, :, 0].astype(np.int64), draw[0][1].cpu().numpy()[..., 0]
    for d, j in np.ndindex(*counts.shape):
        fn, fp = R.regions(pred[d], gt[d], ids[j])
        if counts[d, j]:
            assert (fn | fp)[xy[d, j, 1], xy[d, j, 0]] and lab[d, j] == int(fn[xy[d, j, 1], xy[d, j, 0]])
        else:
            assert xy[d, j].tolist() == [-1, -1] and lab[d, j] == -1
    # worst_slices on the device is its CPU rule
    w = worst_slices(errors, 2)
    assert w.is_cuda and torch.equal(w.cpu(), worst_slices(errors.cpu(), 2))
    # the 2-D use: a batch of binary masks, one object
    one = corrective_clicks((p == ids[0]).to(torch.uint8), (g == ids[0]).to(torch.uint8), [1])
    assert torch.equal(one[0][:, 0], points[:, 0]) and torch.equal(one[1][:, 0], labels[:, 0]) and torch.equal(one[2][:, 0], errors[:, 0])


def test_second_stream_gives_the_same_bits():
    name, pred, gt, ids = next(c for c in CASES if c[0] == "blobs32_5x37x64")
    ref = R.reference(name, pred, gt, ids)
    u = R.k_choices(ref[..., 3:5].sum(-1), 1)["u_random"][1]
    ref_u = R.table(pred, gt, ids, "uniform", u=u)
    side = torch.cuda.Stream()
    u_d = device_table("u", u)
    for mode, want in (("center", ref), ("uniform", ref_u)):
        a, b = Abi(pred, gt, ids), Abi(pred, gt, ids, shift=(1, 0), stream=side)
        for _ in range(3):                                                             # the two streams' workgroups share the device
            for x in (a, b):
                x.run(mode, "u" if mode == "uniform" else None, u_d if mode == "uniform" else None, sync=False)
        for x in (a, b):
            assert np.array_equal(x.result(mode), want), mode


def test_graph_capture_and_replay():
    import medical_sam2_amd.ops as ops
    name, pred, gt, ids = next(c for c in CASES if c[0] == "blobs_5x37x65")
    _, other, _, _ = next(c for c in CASES if c[0] == "ties_5x37x65")
    p, g = torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV)
    ids_d = ops.label_ids(ids, DEV)
    ws = ops._workspace8(ops.label_error_clicks_workspace_bytes(5, 37, 65, len(ids)), DEV)
    eager = ops.label_error_clicks(p, g, ids_d, workspace=ws).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.label_error_clicks(p, g, ids_d, workspace=ws)
    for v in (other, pred, other, pred):                                               # the replay reads what the buffers hold now
        p.copy_(torch.from_numpy(v).to(DEV))
        out.fill_(-7), ws.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), R.table(v, gt, ids))
    assert torch.equal(out, eager)
