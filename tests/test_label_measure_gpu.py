"""msam2_label_measure, ops.label_measure and volume_labels.organ_measurements on the MI355X.

Every table is an integer, so every comparison is exact equality with the brute-force restatement (tests/measure_restate.py), nothing
excluded.  The entry is called through the C ABI with the label volume inside a 0xAB-padded buffer (0xAB is a listed, absent id of the blob
fixtures: an over-read gives it voxels, faces and intensities), the image inside a buffer padded with a value no fixture holds, and the
five tables inside sentinel canvases of -7: a stray store is seen.  Labels and image are shifted off their alignment independently."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import measure_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64
NAMES = ("moments", "extent", "vrange", "faces", "hist")


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


class Abi:
    """one volume (and image) on the device in padded buffers, the entry on sentinel canvases; tables come back as int64 numpy"""

    def __init__(self, vol, ids, image=None, lo=0, bins=0, faces=True, hist=True, shift=(0, 0), stream=None):
        import medical_sam2_amd.ops as ops
        from medical_sam2_amd import _lib
        self.ops, self.L = ops, _lib.lib()
        self.D, self.H, self.W = vol.shape
        self.n, self.lo, self.bins, self.stream = len(ids), lo, bins, stream
        self.vcan, self.vol = padded(torch.from_numpy(vol), 0xAB, shift[0])
        self.vol.copy_(torch.from_numpy(vol))
        self.ids = torch.tensor(ids, dtype=torch.uint8, device=DEV)
        self.img = self.itype = None
        if image is not None:
            self.ifill = R.IMAGE_PAD[image.dtype]
            assert not (image == self.ifill).any()
            self.ican, self.img = padded(torch.from_numpy(image), self.ifill, shift[1])
            self.img.copy_(torch.from_numpy(image))
            self.itype = {np.dtype(np.uint8): 0, np.dtype(np.int16): 1}[image.dtype]
        n = self.n
        shapes = dict(moments=(torch.int64, (n, 14)), extent=(torch.int32, (n, 6)), vrange=(torch.int32, (n, 2)),
                      faces=(torch.int64, (n, 6)) if faces else None, hist=(torch.int32, (n, bins)) if hist and image is not None and bins else None)
        self.can, self.tab = {}, {}
        for k, s in shapes.items():
            self.can[k], self.tab[k] = padded(torch.empty(s[1], dtype=s[0]), -7) if s else (None, None)
        torch.cuda.synchronize()                             # the buffers are ready whichever stream the entry runs on

    def run(self, sync=True):
        p, t = self.ops._p, self.tab
        s = self.ops._stream() if self.stream is None else self.stream.cuda_stream
        rc = self.L.msam2_label_measure(p(self.vol), p(self.ids), p(self.img), self.itype or 0, self.D, self.H, self.W, self.n, self.lo, self.bins,
                                        p(t["moments"]), p(t["extent"]), p(t["vrange"]), p(t["faces"]), p(t["hist"]), s)
        assert rc == 0, self.L.msam2_last_error().decode()
        if sync:
            torch.cuda.synchronize()
            return self.tables()

    def tables(self):
        for k in NAMES:
            assert self.tab[k] is None or intact(self.can[k], self.tab[k], -7), f"stray store around {k}"
        assert intact(self.vcan, self.vol, 0xAB) and (self.img is None or intact(self.ican, self.img, self.ifill))
        return {k: None if self.tab[k] is None else self.tab[k].cpu().numpy().astype(np.int64) for k in NAMES}


def check(got, ref, image, faces=True, hist=True, what=""):
    """every table the call was asked for equals the restatement's; without an image columns 10 - 13 are 0 and the range table is pre-set"""
    for k in NAMES:
        if (k == "faces" and not faces) or (k == "hist" and (not hist or image is None or ref["hist"].shape[1] == 0)):
            assert got[k] is None
            continue
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), (what, k, np.argwhere(got[k] != ref[k])[:6].tolist())
    absent = ref["moments"][:, 0] == 0
    assert (got["extent"][absent] == -1).all() and (got["moments"][absent] == 0).all()
    assert (got["vrange"][absent] == [R.INT32_MAX, R.INT32_MIN]).all()
    if image is None:
        assert (got["moments"][:, 10:] == 0).all() and (got["vrange"] == [R.INT32_MAX, R.INT32_MIN]).all()


def _filled(shape, v):
    return np.full(shape, v, dtype=np.uint8), [v]


def _cases():
    """name -> (vol, ids, image, hist_lo, bins): the smallest shapes at which each mechanism can go wrong"""
    c = {}
    vol, ids = R.blobs((3, 70, 37), 13, 1)                                # W no multiple of 16: runs straddle rows; 13 organs, a stray value,
    c["blobs13_3x70x37_i16_256"] = (vol, ids, R.hu_image(vol.shape, 2, -200, 256), -200, 256)       # id 255, an absent organ, every frame
    c["blobs13_3x70x37_u8_256"] = (vol, ids, R.grey_image(vol.shape, 3), 0, 256)
    c["blobs13_3x70x37_u8_clipped"] = (vol, ids, R.grey_image(vol.shape, 4), 17, 100)
    c["blobs13_3x70x37_i16_1bin"] = (vol, ids, R.hu_image(vol.shape, 5, 40, 1), 40, 1)
    vol, ids = R.blobs((3, 70, 37), 32, 6)
    c["blobs32_3x70x37_i16_256"] = (vol, ids, R.hu_image(vol.shape, 7, -128, 256), -128, 256)       # n = 32: two passes of 16 organs
    c["blobs32_3x70x37_i16_4096"] = (vol, ids, R.hu_image(vol.shape, 8, -1024, 4096), -1024, 4096)  # the LDS histogram's last size: an organ per pass
    c["blobs32_3x70x37_i16_4097"] = (vol, ids, R.hu_image(vol.shape, 8, -1024, 4097), -1024, 4097)  # ... and the first with global adds
    c["blobs32_3x70x37_i16_1366"] = (vol, ids, R.hu_image(vol.shape, 8, -300, 1366), -300, 1366)    # 2 organs per pass where 3 would not fit
    vol, ids = R.blobs((1, 5, 16), 3, 9)                                  # D = 1: no z neighbour, every voxel on both z frames
    c["blobs3_1x5x16_i16_256"] = (vol, ids, R.hu_image(vol.shape, 10, 0, 256), 0, 256)
    vol = np.array([[[7]], [[9]]], dtype=np.uint8)                        # H = W = 1
    c["two_2x1x1_i16_256"] = (vol, [7, 9, 11], R.hu_image(vol.shape, 11, 0, 256), 0, 256)
    vol, ids = R.blobs((2, 9, 7), 4, 12)                                  # W < 16: every lane is a non-plain lane
    c["blobs4_2x9x7_i16_65536"] = (vol, ids, R.hu_image(vol.shape, 13, -32768, 65536), -32768, 65536)   # more bins than LDS: global adds
    vol, ids = R.blobs((4, 300, 257), 13, 14)                             # several bands per slice: +y faces cross a band boundary
    c["blobs13_4x300x257_i16_4096"] = (vol, ids, R.hu_image(vol.shape, 15, -1024, 4096), -1024, 4096)
    vol, ids = _filled((2, 8, 2048), 200)                                 # one band's Sxx = 8 * 2.86e9 > 2^32
    c["filled_2x8x2048_u8_256"] = (vol, ids, R.grey_image(vol.shape, 16), 0, 256)
    vol, ids = _filled((2, 64, 256), 3)                                   # one band's Svv = 2^14 * 2^30 > 2^32
    c["filled_2x64x256_min_i16_4"] = (vol, ids, np.full(vol.shape, -32768, dtype=np.int16), -32768, 4)
    return c


CASES = _cases()
_REF = {}


def reference(name):
    """the restatement of a case, computed once and shared"""
    if name not in _REF:
        vol, ids, image, lo, bins = CASES[name]
        _REF[name] = R.tables(vol, ids, image, lo, bins)
        for k in _REF[name].values():
            k.setflags(write=False)
    return _REF[name]


def test_the_fixtures_hold_what_they_are_for():
    vol, ids, image, lo, bins = CASES["blobs13_3x70x37_i16_256"]
    ref = reference("blobs13_3x70x37_i16_256")
    assert len(ids) == 13 and 255 in ids and 1 not in ids and (vol == 1).any() and (ref["moments"][:, 0] == 0).sum() == 1
    assert (ref["faces"][:, 3:] > 0).any(axis=0).all() and image.min() == -32768 and image.max() == 32767
    assert all((image == v).any() for v in (lo, lo + bins - 1, lo - 1, lo + bins))
    assert ref["moments"][:, 12].max() > 0 and ref["moments"][:, 13].max() > 0 and (ref["faces"][:, :3] > 0).all(axis=1).sum() >= 8
    big = reference("filled_2x8x2048_u8_256")["moments"][0]
    assert big[6] // 2 > 2 ** 32 and reference("filled_2x64x256_min_i16_4")["moments"][0, 11] // 2 > 2 ** 32
    assert len(CASES["blobs32_3x70x37_i16_256"][1]) == 32


@pytest.mark.parametrize("name", list(CASES))
def test_equal_to_the_restatement_through_the_abi(name):
    vol, ids, image, lo, bins = CASES[name]
    ref = reference(name)
    shifts = [(0, 0), (1, 0), (0, 1), (1, 1)] if name.startswith("blobs13_3x70x37") else [(0, 0), (1, 1)]
    for shift in shifts:
        check(Abi(vol, ids, image, lo, bins, shift=shift).run(), ref, image, what=shift)


@pytest.mark.parametrize("name", ["blobs13_3x70x37_i16_256", "blobs13_4x300x257_i16_4096", "blobs4_2x9x7_i16_65536", "two_2x1x1_i16_256"])
def test_skipped_tables(name):
    vol, ids, image, lo, bins = CASES[name]
    ref = reference(name)
    for shift in ((0, 0), (1, 1)):
        check(Abi(vol, ids, image, lo, bins, faces=False, shift=shift).run(), ref, image, faces=False, what=("no faces", shift))
        check(Abi(vol, ids, image, lo, bins, hist=False, shift=shift).run(), ref, image, hist=False, what=("no hist", shift))
        check(Abi(vol, ids, image, lo, bins, faces=False, hist=False, shift=shift).run(), ref, image, faces=False, hist=False, what=("neither", shift))
        geometry = dict(ref, moments=ref["moments"].copy(), vrange=np.tile(np.array([R.INT32_MAX, R.INT32_MIN]), (len(ids), 1)))
        geometry["moments"][:, 10:] = 0
        check(Abi(vol, ids, None, shift=shift).run(), geometry, None, what=("no image", shift))
        check(Abi(vol, ids, None, faces=False, shift=shift).run(), geometry, None, faces=False, what=("no image, no faces", shift))


def test_second_stream_gives_the_same_bits():
    name = "blobs13_4x300x257_i16_4096"
    vol, ids, image, lo, bins = CASES[name]
    ref = reference(name)
    side = torch.cuda.Stream()
    a, b = Abi(vol, ids, image, lo, bins), Abi(vol, ids, image, lo, bins, shift=(1, 1), stream=side)
    for _ in range(3):                                                    # the two streams' workgroups share the device
        a.run(sync=False)
        b.run(sync=False)
    torch.cuda.synchronize()
    for x in (a, b):
        check(x.tables(), ref, image)


def test_graph_capture_and_replay_with_caller_owned_tables():
    import medical_sam2_amd.ops as ops
    vol, ids, image, lo, bins = CASES["blobs13_3x70x37_i16_256"]
    other, other_image = vol[::-1, ::-1].copy(), R.hu_image(vol.shape, 21, lo, bins)               # another volume on the same ids
    labels, img = torch.from_numpy(vol).to(DEV), torch.from_numpy(image).to(DEV)
    ids_d = ops.label_ids(ids, DEV)
    out = ops.label_measure(labels, ids_d, img, lo, bins)                 # eager: allocates the five tables
    torch.cuda.synchronize()
    eager = [t.clone() for t in out]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        same = ops.label_measure(labels, ids_d, img, lo, bins, out=out)
    assert all(a is b for a, b in zip(same, out))
    for v, im in ((other, other_image), (vol, image)) * 2:                # the replay reads what the buffers hold now; four replays
        labels.copy_(torch.from_numpy(np.ascontiguousarray(v)).to(DEV))
        img.copy_(torch.from_numpy(im).to(DEV))
        for t in out:
            t.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        ref = R.tables(np.ascontiguousarray(v), ids, im, lo, bins)
        for k, t in zip(NAMES, out):
            assert np.array_equal(t.cpu().numpy().astype(np.int64), ref[k]), k
    assert all(torch.equal(a, b) for a, b in zip(out, eager))


def test_wrapper_tables_and_refusals():
    import medical_sam2_amd.ops as ops
    vol, ids, image, lo, bins = CASES["blobs13_3x70x37_u8_clipped"]
    ref = reference("blobs13_3x70x37_u8_clipped")
    labels, img = torch.from_numpy(vol).to(DEV), torch.from_numpy(image).to(DEV)
    m, e, v, f, h = ops.label_measure(labels, ids, img, lo, bins)
    assert (m.dtype, e.dtype, v.dtype, f.dtype, h.dtype) == (torch.int64, torch.int32, torch.int32, torch.int64, torch.int32)
    for k, t in zip(NAMES, (m, e, v, f, h)):
        assert t.is_cuda and np.array_equal(t.cpu().numpy().astype(np.int64), ref[k]), k
    m2, e2, v2, f2, h2 = ops.label_measure(labels, ids, faces=False)
    assert f2 is None and h2 is None and torch.equal(m2[:, :10], m[:, :10]) and torch.equal(e2, e) and bool((m2[:, 10:] == 0).all())
    cases = [
        (lambda: ops.label_measure(labels, ids, img, bins=65537), "label_measure: bins = 65537 (0 = no histogram, else 1 .. 65536)"),
        (lambda: ops.label_measure(labels, ids, bins=4), "label_measure: a histogram needs an image"),
        (lambda: ops.label_measure(labels, ids, img.to(torch.int32)),
         "label_measure: image must be int16 or uint8 contiguous [3, 70, 37] on the labels' device"),
        (lambda: ops.label_measure(labels, ids, img[:, :, :36].contiguous()),
         "label_measure: image must be int16 or uint8 contiguous [3, 70, 37] on the labels' device"),
        (lambda: ops.label_measure(labels, ids, img.cpu()), "label_measure: image must be int16 or uint8 contiguous [3, 70, 37] on the labels' device"),
        (lambda: ops.label_measure(labels, ids, img, lo, bins, out=(m, e, v, f, None)),
         "label_measure: out's hist must be int32 contiguous [13, 100] on the labels' device"),
        (lambda: ops.label_measure(labels, ids, out=(m, e, v, f, h)), "label_measure: out's hist must be None (the table is not asked for)"),
    ]
    for call, text in cases:
        with pytest.raises(ValueError) as err:
            call()
        assert str(err.value) == text


def _same_reports(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), k


def test_organ_measurements_equal_the_host_half_on_the_restatement():
    from medical_sam2_amd.volume_labels import measurement_errors, measurements_from_tables, organ_measurements
    vol, ids, image, _, _ = CASES["blobs13_3x70x37_i16_256"]
    labels, img = torch.from_numpy(vol).to(DEV), torch.from_numpy(image).to(DEV)
    sp, qs = (2.5, 0.75, 0.7), (1, 50, 99.5)
    for rng, (lo, bins) in ((None, (-1024, 4096)), ((-100, 57), (-100, 157))):
        ref = R.tables(vol, ids, image, lo, bins)
        want = measurements_from_tables(ref["moments"], ref["extent"], ref["vrange"], ref["faces"], ref["hist"], lo, sp, qs)
        _same_reports(organ_measurements(labels, img, ids, sp, qs, rng), want)
    grey = R.grey_image(vol.shape, 3)
    ref = R.tables(vol, ids, grey, 0, 256)
    want = measurements_from_tables(ref["moments"], ref["extent"], ref["vrange"], ref["faces"], ref["hist"], 0)
    _same_reports(organ_measurements(labels, torch.from_numpy(grey).to(DEV), ids), want)
    ref = R.tables(vol, ids)
    geometry = measurements_from_tables(ref["moments"], ref["extent"], None, ref["faces"], None, 0, sp)
    got = organ_measurements(labels, None, ids, sp)
    _same_reports(got, geometry)
    vol2, ids2 = R.blobs((3, 70, 37), 3, 30, absent=False)                # obj_ids None: 1 .. n
    relabel = np.zeros(256, dtype=np.uint8)
    relabel[ids2] = [1, 2, 3]
    ref = R.tables(relabel[vol2], [1, 2, 3])
    _same_reports(organ_measurements(torch.from_numpy(relabel[vol2]).to(DEV), n=3),
                  measurements_from_tables(ref["moments"], ref["extent"], None, ref["faces"]))
    e = measurement_errors(got, got)
    present = got["voxels"] > 0
    assert (e["volume_rel_diff"][present] == 0).all() and (e["centroid_distance_mm"][present] == 0).all() and np.isnan(e["volume_rel_diff"][~present]).all()
