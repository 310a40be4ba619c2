"""msam2_label_confidence / ops.label_confidence / volume_labels.volume_confidence / interactive.review_queue on the MI355X.

The entry is called through the C ABI with the logits inside a NaN-padded buffer, the volumes inside 0xAB canvases and the counts inside a
canvas of -7: an over-read poisons a result, a stray store is seen.  shift=1 moves every volume by one byte (the one-voxel path also where
W % 4 == 0).

1. bit equality with the composition: ops.bilinear_upsample's output moved to numpy, the definitions applied there
   (tests/confidence_restate.py) -- labels, core, envelope, conf and every count equal, integer for integer, nothing excluded; labels also
   equal msam2_label_slices' own output (the equality is with the VALUES ops.bilinear_upsample writes only as far as csrc/volume_labels.hip's
   resize_value states that kernel's roundings; DESIGN 7.20 records what the benchmark's sizes show about that);
2. exact against the float64 restatement on the dyadic fixtures (ties: margin 0; values exactly at the threshold);
3. the invariants on every case (confidence_restate.check_invariants);  4. every subset of outputs gives the same bits;
5. a second stream;  6. graph capture and replay;  7. the wrapper;  8. chunking and slice consistency;  9. review_queue."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import confidence_restate as C  # noqa: E402
import volume_labels_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64                       # elements of padding either side of every buffer (a multiple of 4: the canvases keep the 4-voxel path)
VOLUMES = ("labels", "core", "envelope", "conf")
ALL = VOLUMES + ("counts",)
MARGIN_SETS = (tuple(C.logit_margins(C.PROBABILITIES)), C.EIGHT_MARGINS)


@pytest.fixture(autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with torch.no_grad():
        yield


def padded(x, fill, shift=0):
    """x inside a canvas of `fill`: (canvas, view of x's place).  shift: extra elements in front (1 = an unaligned volume)."""
    canvas = torch.full((x.numel() + 2 * PAD + shift,), fill, dtype=x.dtype, device=DEV)
    view = canvas[PAD + shift: PAD + shift + x.numel()].view(x.shape)
    return canvas, view


def intact(canvas, view, fill):
    rest = torch.ones_like(canvas, dtype=torch.bool)
    start = (view.data_ptr() - canvas.data_ptr()) // canvas.element_size()
    rest[start: start + view.numel()] = False
    return bool((canvas[rest] == fill).all())


class Abi:
    """one msam2_label_confidence call on padded buffers; run() may be repeated, results() reads and checks the canvases"""

    def __init__(self, logits, ids, H, W, label_thr, margins, select, want=ALL, shift=0, stream=None):
        self.T, self.n, self.lh, self.lw = logits.shape
        self.H, self.W, self.thr, self.select, self.want, self.stream = H, W, float(np.float32(label_thr)), select, tuple(want), stream
        self.lcan, self.lview = padded(logits.float(), float("nan"))
        self.lview.copy_(logits)
        self.ids = torch.tensor(ids, dtype=torch.uint8, device=DEV)
        self.margins = C.f32_margins(margins)
        K = len(self.margins)
        self.bufs = {}
        for name in VOLUMES:
            if name in self.want:
                self.bufs[name] = padded(torch.empty(self.T, H, W, dtype=torch.uint8), 0xAB, shift) + (0xAB,)
        if "counts" in self.want:
            self.bufs["counts"] = padded(torch.empty(self.T, self.n, 2 + 2 * K, dtype=torch.int32), -7) + (-7,)

    def run(self, sync=True):
        import ctypes

        import medical_sam2_amd.ops as ops
        from medical_sam2_amd import _lib
        m = (ctypes.c_float * len(self.margins))(*self.margins)
        ptr = lambda name: ops._p(self.bufs[name][1]) if name in self.bufs else None                       # noqa: E731
        stream = ops._stream() if self.stream is None else self.stream.cuda_stream
        rc = _lib.lib().msam2_label_confidence(ops._p(self.lview), ops._p(self.ids), self.T, self.n, self.lh, self.lw, self.H, self.W, self.thr, m,
                                               len(self.margins), self.select, *[ptr(name) for name in ALL], stream)
        if sync:
            torch.cuda.synchronize()
        assert rc == 0, _lib.lib().msam2_last_error().decode()
        return self

    def results(self):
        out = {}
        for name, (canvas, view, fill) in self.bufs.items():
            assert intact(canvas, view, fill), f"stray {name} store"
            out[name] = view.cpu().numpy().astype(np.int64) if name == "counts" else view.cpu().numpy()
        return out


def call_abi(*args, **kw):
    return Abi(*args, **kw).run().results()


def same(out, ref, what=None):
    for name, got in out.items():
        assert got.dtype == ref[name].dtype and np.array_equal(got, ref[name]), (what, name, int((got != ref[name]).sum()))


_COMPOSITION = {}


def composition(shape, seed):
    """(logits on the device, ops.bilinear_upsample's output as numpy [T, n, H, W], ids): computed once per case"""
    import medical_sam2_amd.ops as ops
    key = (tuple(shape[:2]) + shape[2] + shape[3], seed)
    if key not in _COMPOSITION:
        T, n, (lh, lw), (H, W) = shape
        x = R.random_logits(T, n, lh, lw, seed).to(DEV)
        up = ops.bilinear_upsample(x.view(T * n, lh, lw), H, W).view(T, n, H, W).cpu().numpy()
        _COMPOSITION[key] = (x, up, R.random_ids(n, seed))
    return _COMPOSITION[key]


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d_%dx%d_to_%dx%d" % (s[0], s[1], *s[2], *s[3]))
@pytest.mark.parametrize("seed", R.SEEDS)
def test_bit_equal_to_upsample_then_rule(shape, seed):
    import medical_sam2_amd.ops as ops
    x, up, ids = composition(shape, seed)
    H, W = shape[3]
    assert up.dtype == np.float32
    for thr in (0.0, 1.5):
        own, _ = ops.label_slices(x, ids, H, W, thr)                                        # msam2_label_slices' own bytes
        own = own.cpu().numpy()
        for margins in MARGIN_SETS:
            for select in range(len(margins)):
                ref = C.restate(up, ids, thr, margins, select)
                out = call_abi(x, ids, H, W, thr, margins, select)
                same(out, ref, (thr, len(margins), select))
                assert np.array_equal(out["labels"], own)
                C.check_invariants(out, ids, margins, select, ref)
            # volumes that are not 4-byte aligned: the one-voxel path also where W % 4 == 0
            out = call_abi(x, ids, H, W, thr, margins, len(margins) - 1, shift=1)
            same(out, ref, (thr, len(margins), "shifted"))
        # not vacuous: every object has a non-zero sum in every column (tests/test_label_confidence_cpu.py: at least 47 and 374)
        if shape in (R.SHAPES[0], R.SHAPES[6]):
            ref = C.restate(up, ids, thr, MARGIN_SETS[0], 1)
            assert (ref["counts"].sum(axis=0) > 0).all(), ref["counts"].sum(axis=0)
            assert (ref["core"] != ref["labels"]).any() and (ref["envelope"] != ref["labels"]).any() and len(np.unique(ref["conf"])) == 4


@pytest.mark.parametrize("low,out_size", R.DYADIC_CASES)
def test_exact_against_float64_on_dyadic_fixtures(low, out_size):
    T, (lh, lw), (H, W) = 2, low, out_size
    x = R.dyadic_logits(T, lh, lw, seed=H)
    ids = R.random_ids(6, seed=H)
    v = R.resize64(x.numpy(), H, W)
    for thr in (0.0, 1.25):
        for select in range(3):
            ref = C.restate(v, ids, thr, C.DYADIC_MARGINS, select)
            for shift in (0, 1):
                out = call_abi(x.to(DEV), ids, H, W, thr, C.DYADIC_MARGINS, select, shift=shift)
                same(out, ref, (thr, select, shift))
                C.check_invariants(out, ids, C.DYADIC_MARGINS, select, ref)
        assert ((ref["m"] == 0) & ref["lab"]).any() and ((ref["m"] == 0) & ref["near"]).any()     # ties, and values exactly at the threshold


def test_every_subset_of_outputs_gives_the_same_bits():
    from medical_sam2_amd import _lib
    shape = R.SHAPES[4]                                                                     # 3 x 13, 16^2 -> 64^2
    x, up, ids = composition(shape, 1)
    H, W = shape[3]
    ref = C.restate(up, ids, 0.0, MARGIN_SETS[0], 1)
    subsets = [c for r in range(1, len(ALL) + 1) for c in itertools.combinations(ALL, r)]
    assert len(subsets) == 31
    for i, want in enumerate(subsets):
        out = call_abi(x, ids, H, W, 0.0, MARGIN_SETS[0], 1, want=want, shift=i & 1)
        assert set(out) == set(want)
        same(out, ref, want)
    a = Abi(x, ids, H, W, 0.0, MARGIN_SETS[0], 1, want=())
    with pytest.raises(AssertionError, match="no output requested"):
        a.run()
    assert _lib.lib().msam2_last_error().decode() == "label_confidence: no output requested (labels, core, envelope, conf, counts)"


def test_second_stream_gives_the_same_bits():
    shape = R.SHAPES[6]                                                                     # 1 x 4, 64^2 -> 256^2: 16 workgroups a call
    x, up, ids = composition(shape, 2)
    H, W = shape[3]
    ref = C.restate(up, ids, 0.0, C.EIGHT_MARGINS, 3)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    a, b = Abi(x, ids, H, W, 0.0, C.EIGHT_MARGINS, 3), Abi(x, ids, H, W, 0.0, C.EIGHT_MARGINS, 3, shift=1, stream=side)
    torch.cuda.synchronize()
    for _ in range(3):                                                                      # the two streams' workgroups share the device
        a.run(sync=False)
        b.run(sync=False)
    torch.cuda.synchronize()
    for run in (a, b):
        same(run.results(), ref)


def test_graph_capture_and_replay_with_caller_owned_outputs():
    import medical_sam2_amd.ops as ops
    T, n, (lh, lw), (H, W) = R.SHAPES[4]
    ids = R.random_ids(n, 5)
    ids_d = ops.label_ids(ids, DEV)
    first, second = R.random_logits(T, n, lh, lw, 5), R.random_logits(T, n, lh, lw, 6)
    x = first.to(DEV)
    margins = MARGIN_SETS[0]
    out = ops.label_confidence(x, ids_d, H, W, margins, 2, 0.0)                            # eager: allocates the five outputs
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        again = ops.label_confidence(x, ids_d, H, W, margins, 2, 0.0, *out)
    assert all(a is b for a, b in zip(again, out))
    for logits in (second, first, second, first):                                           # the replay reads what the buffer holds now
        x.copy_(logits.to(DEV))
        for t in out:
            t.fill_(77)
        g.replay()
        torch.cuda.synchronize()
        up = ops.bilinear_upsample(x.view(T * n, lh, lw), H, W).view(T, n, H, W).cpu().numpy()
        ref = C.restate(up, ids, 0.0, margins, 2)
        for name, t in zip(ALL, out):
            assert np.array_equal(t.cpu().numpy(), ref[name]), name


def test_wrapper_outputs_and_refusals():
    import medical_sam2_amd.ops as ops
    from medical_sam2_amd import _lib
    shape = R.SHAPES[0]
    x, up, ids = composition(shape, 0)
    (T, n), (H, W) = shape[:2], shape[3]
    margins = MARGIN_SETS[0]
    ref = C.restate(up, ids, 1.5, margins, 0)
    out = ops.label_confidence(x, ids, H, W, margins, 0, 1.5)
    assert [t.dtype for t in out] == [torch.uint8] * 4 + [torch.int32] and all(t.is_cuda for t in out)
    assert [tuple(t.shape) for t in out] == [(T, H, W)] * 4 + [(T, n, 8)]
    for name, t in zip(ALL, out):
        assert np.array_equal(t.cpu().numpy(), ref[name]), name
    # False skips an output, a tensor is filled in place; margins given as float64 are rounded to fp32 on the way
    core = torch.full((T, H, W), 0xAB, dtype=torch.uint8, device=DEV)
    labels, c, envelope, conf, counts = ops.label_confidence(x, ops.label_ids(ids, DEV), H, W, np.float64(margins), 0, 1.5, labels=False, core=core,
                                                             envelope=False, conf=False, counts=False)
    assert labels is None and envelope is None and conf is None and counts is None and c is core
    assert np.array_equal(core.cpu().numpy(), ref["core"])
    cases = [
        (lambda: ops.label_confidence(x.double(), ids, H, W, margins), "label_confidence: fp32 contiguous [T, n, lh, lw]"),
        (lambda: ops.label_confidence(x, ids[:-1], H, W, margins), f"label_confidence: {n} objects need {n} uint8 ids"),
        (lambda: ops.label_confidence(x, ids, H, W, margins, labels=torch.zeros(T, H, W, dtype=torch.uint8)),
         f"label_confidence: labels must be uint8 contiguous [{T}, {H}, {W}] on the logits' device"),
        (lambda: ops.label_confidence(x, ids, H, W, margins, envelope=torch.zeros(T, H, W + 1, dtype=torch.uint8, device=DEV)),
         f"label_confidence: envelope must be uint8 contiguous [{T}, {H}, {W}] on the logits' device"),
        (lambda: ops.label_confidence(x, ids, H, W, margins, counts=torch.zeros(T, n, 8, dtype=torch.int64, device=DEV)),
         f"label_confidence: counts must be int32 contiguous [{T}, {n}, 8] on the logits' device"),
        (lambda: ops.label_confidence(x, ids, H, W, torch.tensor(margins, device=DEV)), "label_confidence: margins are host numbers (the call reads them)"),
    ]
    for call, text in cases:
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
    for kw, text in ((dict(margins=(1.0, 0.5)), "label_confidence: margins[1] = 0.5 (finite, positive and strictly ascending)"),
                     (dict(margins=margins, select=3), "label_confidence: select = 3 (0 .. 2)"),
                     (dict(margins=()), "label_confidence: K = 0 margins (1 .. 8 per call)")):
        with pytest.raises(_lib.Msam2Error) as e:
            ops.label_confidence(x, ids, H, W, **kw)
        assert text in str(e.value)
    with pytest.raises(_lib.Msam2Error, match="no output requested"):
        ops.label_confidence(x, ids, H, W, margins, labels=False, core=False, envelope=False, conf=False, counts=False)
    torch.cuda.synchronize()


def test_volume_confidence_chunking_and_slice_consistency():
    import medical_sam2_amd.ops as ops
    from medical_sam2_amd.volume_labels import confidence_report, margins_from_probabilities, slice_consistency, volume_confidence
    T, n, (lh, lw), (H, W) = 5, 3, (16, 16), (64, 48)
    x = R.random_logits(T, n, lh, lw, 7).to(DEV)
    ids = [9, 2, 200]
    up = ops.bilinear_upsample(x.view(T * n, lh, lw), H, W).view(T, n, H, W).cpu().numpy()
    assert list(margins_from_probabilities(C.PROBABILITIES)) == list(MARGIN_SETS[0])
    ref = C.restate(up, ids, 0.0, MARGIN_SETS[0], 1)
    as_dict = {10 * t: x[t][:, None] for t in reversed(range(T))}                          # keys in ascending order are the slices
    for masks, step in ((x, 8), (x, 1), (x, 2), (x, T), (as_dict, 2), (as_dict, T)):
        got = volume_confidence(masks, H, W, ids, slices_per_call=step)
        assert set(got) == set(ALL) | {"margins"} and got["margins"] == MARGIN_SETS[0]
        for name in ALL:
            assert got[name].is_cuda and np.array_equal(got[name].cpu().numpy(), ref[name]), (step, name)
    # other margins, another band and threshold, a subset of the maps, default ids
    ref8 = C.restate(up, [1, 2, 3], 1.5, C.EIGHT_MARGINS, 6)
    got = volume_confidence(as_dict, H, W, margins=C.EIGHT_MARGINS, select=6, label_thr=1.5, slices_per_call=3, maps=("core", "conf"))
    assert set(got) == {"core", "conf", "counts", "margins"}
    for name in ("core", "conf", "counts"):
        assert np.array_equal(got[name].cpu().numpy(), ref8[name]), name
    # adjacent slices: (|A & B|, |A|, |B|) per object, against numpy
    labels = torch.from_numpy(ref["labels"]).to(DEV)
    cons = slice_consistency(labels, ids)
    assert cons.dtype == torch.int32 and cons.is_cuda and tuple(cons.shape) == (T - 1, n, 3)
    want = np.zeros((T - 1, n, 3), dtype=np.int64)
    for j, i in enumerate(ids):
        a, b = ref["labels"][:-1] == i, ref["labels"][1:] == i
        want[:, j] = np.stack([(a & b).sum(axis=(1, 2)), a.sum(axis=(1, 2)), b.sum(axis=(1, 2))], axis=-1)
    assert np.array_equal(cons.cpu().numpy(), want) and want[..., 0].sum() > 0
    rep = confidence_report(volume_confidence(x, H, W, ids, maps=())["counts"], cons, spacing=(2.0, 0.5, 0.5))
    hand = C.report_by_hand(ref["counts"], (2.0, 0.5, 0.5))
    for key, value in hand.items():
        assert np.array_equal(rep[key], value, equal_nan=True), key
    assert np.array_equal(rep["slice_dice"], 2.0 * want[..., 0] / (want[..., 1] + want[..., 2]))


def test_review_queue_on_a_hand_built_state():
    import medical_sam2_amd.ops as ops
    from medical_sam2_amd.interactive import review_queue
    from medical_sam2_amd.prompts import corrective_clicks
    T, n, (lh, lw), (H, W) = 4, 3, (16, 16), (64, 64)
    x = R.random_logits(T, n, lh, lw, 11).to(DEV)
    ids = [5, 17, 3]
    frames = {t: {"pred_masks": x[t][:, None].clone()} for t in range(T)}
    state = {"num_frames": T, "video_height": H, "video_width": W, "device": torch.device(DEV), "obj_ids": list(ids),
             "output_dict": {"cond_frame_outputs": {1: frames[1]}, "non_cond_frame_outputs": {t: frames[t] for t in (0, 2, 3)}}}
    up = ops.bilinear_upsample(x.view(T * n, lh, lw), H, W).view(T, n, H, W).cpu().numpy()
    for select, per in ((1, 1), (0, 2), (2, T + 1)):
        ref = C.restate(up, ids, 0.0, MARGIN_SETS[0], select)
        points, point_labels, errors = corrective_clicks(torch.from_numpy(ref["core"]).to(DEV), torch.from_numpy(ref["envelope"]).to(DEV), ids, "center")
        points, errors = points.cpu().numpy(), errors.cpu().numpy()
        uncertain = ref["counts"][..., 2 + select] + ref["counts"][..., 2 + 3 + select]       # [T, n]
        assert np.array_equal(errors[..., 0], uncertain) and (errors[..., 1] == 0).all()     # the envelope's voxels that the core misses ARE the band
        want = []
        for j, i in enumerate(ids):
            order = sorted((t for t in range(T) if uncertain[t, j] > 0), key=lambda t: (-uncertain[t, j], t))[:per]
            want += [(i, t, int(points[t, j, 0, 0]), int(points[t, j, 0, 1]), int(uncertain[t, j])) for t in order]
        report, queue = review_queue(state, ids, select=select, per_object=per)
        assert queue == want and len(want) == n * min(per, T), (select, per)
        for _, t, px, py, _ in queue:
            assert ref["envelope"][t, py, px] != ref["core"][t, py, px]                      # the point lies in the uncertain band
        hand = C.report_by_hand(ref["counts"])
        for key, value in hand.items():
            assert np.array_equal(report[key], value, equal_nan=True), key
        assert report["slice_dice"].shape == (T - 1, n) and report["margins"] == MARGIN_SETS[0]
