"""msam2_volume_prep / msam2_label_resize, ops.volume_prep / ops.label_resize and volume_prep.py on the MI355X.

Every result is an integer or a function of one, so every comparison is exact equality (bytes of the greys, bits of the fp32 frames) with
the numpy restatement (tests/volume_prep_restate.py), which tests/test_volume_prep_cpu.py ties to Pillow and to the loader.  The entries
are called through the C ABI: inputs sit in poisoned buffers (int16 padded with 32767, float32 with NaN, uint8 with 0xFF: an over-read
windows to a visible 255 or 0), outputs in sentinel canvases (0xAB bytes, NaN floats) whose rest must stay intact.  The tables are the
restatement's own.  The kernels have no grid-stride loop (one workgroup per tile, group and slice), so no case wraps one.

Shapes (T = 3): 37x53->64 non-dyadic upscale, taps truncated at all four borders; 64x64->64 both passes skipped; 33x64->64 and 64x17->32
one pass / two passes with full tiles only (the tile is 64 x 32); 100x130->96 downscale with a partial tile across; 100x130->90 partial
tiles both ways and S % 4 != 0 (the one-pixel stores); 700x300->16 too large for the fused form's LDS: two launches on its own."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import volume_prep_restate as R  # noqa: E402
from helpers import kernels_launched  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64
T = 3
SWITCH = "MSAM2_VOLUME_PREP_FUSED"
SHAPES = [(37, 53, 64), (64, 64, 64), (33, 64, 64), (64, 17, 32), (100, 130, 96), (100, 130, 90), (700, 300, 16)]
TORCH = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int16): torch.int16, np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32,
         np.dtype(np.int64): torch.int64}
SRC_TYPE = {np.dtype(np.uint8): 0, np.dtype(np.int16): 1, np.dtype(np.float32): 2}
TYPE_NAME = {np.dtype(np.uint8): "unsignedchar", np.dtype(np.int16): "short", np.dtype(np.float32): "float", np.dtype(np.int32): "int",
             np.dtype(np.int64): "long"}
POISON = {np.dtype(np.uint8): 0xFF, np.dtype(np.int16): 32767, np.dtype(np.float32): float("nan"), np.dtype(np.int32): 77, np.dtype(np.int64): 77}
CT, LUNG, FULL = (-160.0, 240.0), (-1000.0, 400.0), (-32768.0, 32767.0)


@pytest.fixture(autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    before = os.environ.pop(SWITCH, None)
    with torch.no_grad():
        yield
    os.environ.pop(SWITCH, None)
    if before is not None:
        os.environ[SWITCH] = before


def lib():
    from medical_sam2_amd import _lib
    return _lib.lib()


def padded(shape, dtype, fill, shift=0):
    """a contiguous view of `shape` inside a 1-D canvas of `fill`, `shift` elements off the canvas' alignment: (canvas, view)"""
    n = int(np.prod(shape))
    canvas = torch.full((n + 2 * PAD + shift,), fill, dtype=dtype, device=DEV)
    return canvas, canvas[PAD + shift: PAD + shift + n].view(*shape)


def intact(canvas, view):
    """everything of the canvas outside the view still holds the fill (0xAB bytes / NaN)"""
    start = (view.data_ptr() - canvas.data_ptr()) // canvas.element_size()
    rest = torch.cat([canvas[:start], canvas[start + view.numel():]])
    return bool(torch.isnan(rest).all()) if canvas.dtype.is_floating_point else bool((rest == 0xAB).all())


def poisoned(x: np.ndarray):
    canvas, view = padded(x.shape, TORCH[x.dtype], POISON[x.dtype])
    view.copy_(torch.from_numpy(x))
    return canvas, view


def dev_tables(n, S):
    return (None, None, 0) if n == S else tuple(torch.from_numpy(t).to(DEV) for t in R.resample_tables(n, S)) + (R.resample_tables(n, S)[0].shape[1],)


def raw_volume(dtype, Cin, H0, W0, seed):
    img = np.stack([R.sample_image(H0, W0, seed + 7 * i) for i in range(T * Cin)]).reshape(T, Cin, H0, W0)
    if dtype == np.uint8:
        return img
    v = (img.astype(np.int32) - 110) * 7 + (img.astype(np.int32) % 5)          # about -770 .. 1020: both windows clamp at both ends
    if dtype == np.int16:
        return v.astype(np.int16)
    f = (v.astype(np.float32) + np.float32(0.37)) * np.float32(1.013)
    flat = f.reshape(-1)
    flat[3::97], flat[11::193], flat[17::211] = np.nan, np.inf, -np.inf
    flat[5::101], flat[6::103] = np.float32(CT[0]), np.float32(CT[1])
    return f


def configs(dtype):
    """(name, Cin, windows): one window, three windows (channels 0 and 2 share one: a group of non-adjacent channels), three planes"""
    if dtype == np.uint8:
        return [("cin1", 1, None), ("cin1_windows_ignored", 1, [CT, LUNG, FULL]), ("cin3", 3, None)]
    w3 = [CT, LUNG, FULL] if dtype == np.int16 else [(-160.5, 240.25), LUNG, (0.0, 1e-3)]
    return [("cin1_one_window", 1, [w3[0]] * 3), ("cin1_three_windows", 1, [w3[0], w3[1], w3[0]]), ("cin3_three_windows", 3, w3)]


class Call:
    """one msam2_volume_prep call on poisoned input and sentinel outputs"""

    def __init__(self, raw, windows, S, stream=None, shift=0):
        import ctypes
        self.L, self.S, self.stream = lib(), S, stream
        self.T, self.Cin, self.H0, self.W0 = raw.shape
        self.typ = SRC_TYPE[raw.dtype]
        self.scan, self.src = poisoned(raw)
        self.gcan, self.grey = padded((self.T, 3, S, S), torch.uint8, 0xAB, shift=4 * shift)
        self.ocan, self.out = padded((self.T, 3, S, S), torch.float32, float("nan"), shift=4 * shift)
        self.tx, self.ty = dev_tables(self.W0, S), dev_tables(self.H0, S)
        self.win = None if windows is None else (ctypes.c_double * 6)(*[v for p in windows for v in p])
        self.mean, self.std = (ctypes.c_float * 3)(*R.MEAN), (ctypes.c_float * 3)(*R.STD)
        nb = 3 * self.T * self.H0 * S
        self.wcan, self.ws = padded((nb,), torch.uint8, 0xAB)
        g = R.greys(raw, windows, S)
        self.ref_grey, self.ref_out = torch.from_numpy(g), torch.from_numpy(R.normalise(g))
        torch.cuda.synchronize()

    def launch(self, grey=True, out=True, workspace=True):
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        s = torch.cuda.current_stream().cuda_stream if self.stream is None else self.stream.cuda_stream
        rc = self.L.msam2_volume_prep(p(self.src), self.typ, self.T, self.Cin, self.H0, self.W0, self.S, self.win, p(self.tx[0]), p(self.tx[1]),
                                      self.tx[2], p(self.ty[0]), p(self.ty[1]), self.ty[2], self.mean, self.std, p(self.grey) if grey else None,
                                      p(self.out) if out else None, p(self.ws) if workspace else None, self.ws.numel() if workspace else 0, s)
        assert rc == 0, self.L.msam2_last_error().decode()

    def check(self, what, grey=True, out=True):
        torch.cuda.synchronize()
        if grey:
            got = self.grey.cpu()
            assert torch.equal(got, self.ref_grey), f"{what}: {int((got != self.ref_grey).sum())} of {got.numel()} grey bytes differ"
        if out:
            got, ref = self.out.cpu().view(torch.int32), self.ref_out.view(torch.int32)
            assert torch.equal(got, ref), f"{what}: {int((got != ref).sum())} of {got.numel()} fp32 values differ in their bits"
        assert intact(self.gcan, self.grey) and intact(self.ocan, self.out) and intact(self.wcan, self.ws), f"{what}: stray store"
        if not grey:
            assert bool((self.grey == 0xAB).all()), f"{what}: grey_out written although NULL was passed"
        if not out:
            assert bool(torch.isnan(self.out).all()), f"{what}: out written although NULL was passed"

    def reset(self):
        self.grey.fill_(0xAB), self.out.fill_(float("nan")), self.ws.fill_(0xAB)


def fused_applies(H0, W0, S):
    os.environ.pop(SWITCH, None)
    return lib().msam2_volume_prep_workspace_bytes(T, H0, W0, S) == 0


def expected_kernels(dtype, fused):
    t = TYPE_NAME[np.dtype(dtype)]
    return {f"volume_prep_fused_kernel<{t}>"} if fused else {f"volume_prep_hpass_kernel<{t}>", "volume_prep_vpass_kernel"}


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32], ids=["uint8", "int16", "float32"])
@pytest.mark.parametrize("H0,W0,S", SHAPES, ids=[f"{h}x{w}to{s}" for h, w, s in SHAPES])
def test_equal_to_the_restatement_through_the_abi(H0, W0, S, dtype):
    L = lib()
    fits = fused_applies(H0, W0, S)
    assert fits == ((H0, W0, S) != (700, 300, 16)), "only 700x300->16 is beyond the fused form's LDS budget"
    calls = [(name, Call(raw_volume(dtype, Cin, H0, W0, seed=H0 + len(name)), win, S)) for name, Cin, win in configs(dtype)]
    results = {}
    for form in (["default", "1", "0"] if fits else ["default", "0"]):
        os.environ.pop(SWITCH, None)
        if form != "default":
            os.environ[SWITCH] = form
        for _, c in calls:
            c.reset()
        ran = kernels_launched(lambda: [c.launch(workspace=form != "1") for _, c in calls], "volume_prep_")
        assert ran == expected_kernels(dtype, fused=fits and form != "0"), (form, ran)
        for name, c in calls:
            c.check(f"{name}, form {form}")
            results[(name, form)] = (c.grey.clone(), c.out.clone())
    for name, _ in calls:                                              # the two forms against each other, bit for bit
        a, b = results[(name, "default")], results[(name, "0")]
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), name
    if not fits:                                                       # forcing the fused form where it does not fit is an error, not a fallback
        os.environ[SWITCH] = "1"
        c = calls[0][1]
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        rc = L.msam2_volume_prep(p(c.src), c.typ, c.T, c.Cin, c.H0, c.W0, c.S, c.win, p(c.tx[0]), p(c.tx[1]), c.tx[2], p(c.ty[0]), p(c.ty[1]),
                                 c.ty[2], c.mean, c.std, p(c.grey), p(c.out), p(c.ws), c.ws.numel(), None)
        assert rc < 0 and "LDS" in L.msam2_last_error().decode()
    # one output only, and outputs four bytes / four floats further on (still aligned for the four-pixel stores)
    os.environ.pop(SWITCH, None)
    name, Cin, win = configs(dtype)[2]
    c = Call(raw_volume(dtype, Cin, H0, W0, seed=5), win, S, shift=1)
    for grey, out in ((True, False), (False, True)):
        c.reset()
        c.launch(grey=grey, out=out)
        c.check(f"{name}, grey {grey}, out {out}", grey=grey, out=out)


def test_unaligned_outputs_take_the_one_pixel_stores():
    raw = raw_volume(np.int16, 1, 37, 53, seed=2)
    c = Call(raw, [CT] * 3, 64)
    c.gcan, c.grey = padded((T, 3, 64, 64), torch.uint8, 0xAB, shift=1)
    c.ocan, c.out = padded((T, 3, 64, 64), torch.float32, float("nan"), shift=1)
    assert c.grey.data_ptr() % 4 == 1 and c.out.data_ptr() % 16 == 4
    for form in ("1", "0"):
        os.environ[SWITCH] = form
        c.reset()
        c.launch()
        c.check(f"unaligned, form {form}")


@pytest.mark.parametrize("form", ["1", "0"])
def test_int16_window_on_every_value(form):
    os.environ[SWITCH] = form
    raw = np.arange(-32768, 32768, dtype=np.int64).astype(np.int16).reshape(1, 1, 256, 256)
    for windows in ([CT, LUNG, FULL], [(0.0, 1.0), (-1.0, 0.0), (32766.0, 32767.0)]):
        c = Call(raw, windows, 256)
        assert all(np.array_equal(c.ref_grey[0, k].numpy(), R.window_i16(raw[0, 0], int(w[0]), int(w[1]))) for k, w in enumerate(windows))
        c.launch()
        c.check(f"int16 windows {windows}")


@pytest.mark.parametrize("form", ["1", "0"])
def test_float32_window_specials(form):
    os.environ[SWITCH] = form
    lo, hi = 0.0, 510.0                                                # every odd value is an exact half-way point
    v = np.array([np.nan, np.inf, -np.inf, lo, hi, -1.0, 511.0, 1.0, 3.0, 255.0, 509.0, 0.99999994, 1.0000001, 2.0, 508.9999, -0.0], dtype=np.float32)
    raw = np.resize(np.concatenate([v, np.arange(0, 511, dtype=np.float32), np.linspace(-3, 513, 3001, dtype=np.float32)]), (1, 1, 64, 64)).copy()
    c = Call(raw, [(lo, hi), (-160.5, 240.25), (1e-30, 2e-30)], 64)
    assert c.ref_grey[0, 0].flatten()[:16].tolist() == [0, 255, 0, 0, 255, 0, 255, 1, 2, 128, 255, 0, 1, 1, 254, 0]
    c.launch()
    c.check("float32 specials")


def test_second_stream_gives_the_same_bits():
    side = torch.cuda.Stream()
    a = Call(raw_volume(np.int16, 1, 100, 130, seed=1), [CT] * 3, 96)
    b = Call(raw_volume(np.float32, 3, 37, 53, seed=2), [CT, LUNG, (0.0, 1.0)], 64, stream=side)
    c = Call(raw_volume(np.uint8, 3, 700, 300, seed=3), None, 16, stream=side)
    for form in (None, "0"):
        os.environ.pop(SWITCH, None)
        if form:
            os.environ[SWITCH] = form
        for x in (a, b, c):
            x.reset()
        torch.cuda.synchronize()
        for _ in range(3):                                             # the two streams' workgroups share the device
            a.launch(), b.launch(), c.launch()
        for x in (a, b, c):
            x.check(f"two streams, form {form}")


# ---- label maps -------------------------------------------------------------------------------------------------------------------------
def label_map(dtype, H0, W0, seed):
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:H0, 0:W0]
    lab = np.stack([((xs + 3 * t) // 7 + (ys // 5)) % 6 for t in range(T)]).astype(np.int64)
    special = [0, 1, 255] + {np.uint8: [], np.int16: [256, -1], np.int32: [256, -1, 70000], np.int64: [256, -1, 70000, 2 ** 40 + 3]}[dtype]
    idx = rng.randint(0, lab.size, 40 * len(special))
    lab.reshape(-1)[idx] = np.resize(np.array(special, dtype=np.int64), idx.size)
    lab[:, 0, 0], lab[:, -1, -1] = 255, 1
    return lab.astype(dtype)


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.int32, np.int64], ids=["uint8", "int16", "int32", "int64"])
def test_label_resize_equals_the_restatement(dtype):
    import ctypes
    L = lib()
    for (H0, W0, S), shift in (((37, 53, 64), 0), ((37, 53, 64), 1), ((100, 130, 90), 0), ((64, 64, 64), 0), ((700, 300, 16), 0)):
        raw = label_map(dtype, H0, W0, seed=S + shift)
        scan, src = poisoned(raw)
        ymap, xmap = (torch.from_numpy(R.nearest_map(n, S)).to(DEV) for n in (H0, W0))
        for keep in (None, [1, 3, 255]):
            k8 = None
            if keep is not None:
                k8 = (ctypes.c_uint32 * 8)()
                for v in keep:
                    k8[v >> 5] |= 1 << (v & 31)
            ocan, out = padded((T, S, S), torch.uint8, 0xAB, shift=shift)
            assert out.data_ptr() % 16 == shift
            torch.cuda.synchronize()

            def go():
                rc = L.msam2_label_resize(src.data_ptr(), {1: 0, 2: 1, 4: 2, 8: 3}[raw.itemsize], T, H0, W0, S, ymap.data_ptr(), xmap.data_ptr(), k8,
                                          out.data_ptr(), torch.cuda.current_stream().cuda_stream)
                assert rc == 0, L.msam2_last_error().decode()
            assert kernels_launched(go, "label_resize_") == {f"label_resize_kernel<{TYPE_NAME[np.dtype(dtype)]}>"}
            ref = R.labels(raw, S, keep)
            assert np.array_equal(out.cpu().numpy(), ref), (H0, W0, S, shift, keep, int((out.cpu().numpy() != ref).sum()))
            assert intact(ocan, out)
            if dtype != np.uint8:
                assert set(np.unique(ref)) <= ({0, 1, 2, 3, 4, 5, 255} if keep is None else {0, 1, 3, 255})


# ---- Python layer -----------------------------------------------------------------------------------------------------------------------
def _same_dicts(got, want):
    assert sorted(got) == sorted(want)
    for f in want:
        assert sorted(int(o) for o in got[f]) == sorted(int(o) for o in want[f]), f
        for o in want[f]:
            assert got[f][o].dtype == want[f][o].dtype and got[f][o].shape == want[f][o].shape and torch.equal(got[f][o], want[f][o]), (f, o)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """a synthetic case in the dataset's layout and its decoded raw arrays, cropped to the labelled slices as the loader does"""
    from PIL import Image
    import medical_sam2_amd.data as data
    root = str(tmp_path_factory.mktemp("btcv"))
    data.write_synthetic_case(root, "case0", n_slices=8, size=48, n_objects=3, seed=0)
    idir, mdir = (os.path.join(root, "Test", k, "case0") for k in ("image", "mask"))
    seg = np.stack([np.load(os.path.join(mdir, f"{i}.npy")) for i in range(8)])
    labelled = [i for i in range(8) if seg[i].sum() > 0]
    first, last = labelled[0], labelled[-1]
    rgb = np.stack([np.array(Image.open(os.path.join(idir, f"{i}.jpg")).convert("RGB")).transpose(2, 0, 1) for i in range(first, last + 1)])
    return root, np.ascontiguousarray(rgb), np.ascontiguousarray(seg[first: last + 1])


@pytest.mark.parametrize("S", [32, 64])
def test_prepare_case_equals_the_dataset_pack(case, S):
    import medical_sam2_amd.data as data
    import medical_sam2_amd.volume_prep as vp
    from medical_sam2_amd.video_predictor import load_video_frames_from_data
    from medical_sam2_amd.volume_labels import labels_from_pack
    root, rgb, seg = case
    pack = data.BTCVVolumes(root, image_size=S, mode="Test", video_length=len(rgb), prompt="bbox")[0]
    obj_list = sorted({int(o) for f in pack["label"] for o in pack["label"][f]})
    host_frames = load_video_frames_from_data(pack["image"], offload_video_to_cpu=True)
    frames, labels, bbox = vp.prepare_case(rgb, seg, size=S, obj_ids=obj_list, prompt="bbox", prompt_freq=1, pack=True)
    assert frames.dtype == torch.float32 and torch.equal(frames.cpu().view(torch.int32), host_frames.view(torch.int32))
    assert labels.dtype == torch.uint8 and torch.equal(labels.cpu(), labels_from_pack(pack["label"], obj_list))
    assert any(pack["bbox"][f] for f in pack["bbox"])
    _same_dicts(bbox, pack["bbox"])
    pack_c = data.BTCVVolumes(root, image_size=S, mode="Test", video_length=len(rgb), prompt="click", seed=11)[0]
    frames_c, labels_c, (pt, p_label) = vp.prepare_case(rgb, seg, size=S, prompt="click", prompt_freq=1, pack=True, seed=11)   # ids from the volume
    assert torch.equal(frames_c, frames) and torch.equal(labels_c, labels)
    _same_dicts(pt, pack_c["pt"])
    _same_dicts(p_label, pack_c["p_label"])
    # the device form of the prompts: what segment_volume / train_step_3d take
    t0 = next(f for f in sorted(pack["bbox"]) if len(pack["bbox"][f]) == len(obj_list))
    _, _, prompts = vp.prepare_case(rgb[t0: t0 + 1], seg[t0: t0 + 1], size=S, obj_ids=obj_list, prompt="bbox", prompt_freq=1)
    assert torch.equal(prompts[0]["boxes"].cpu(), torch.stack([pack["bbox"][t0][o] for o in obj_list]))
    # the greys, and an int16 volume with one window: the three channels are one resampling
    g = vp.prepare_volume(rgb, size=S, grey=True)[1]
    assert torch.equal(g.cpu(), torch.from_numpy(R.greys(rgb, None, S)))
    hu = ((rgb[:, :1].astype(np.int32) - 100) * 9).astype(np.int16)[:, 0]
    os.environ[SWITCH] = "0"                                           # the form that goes through the slices in chunks: 2, then 1
    f16, g16 = vp.prepare_volume(hu, window=CT, size=S, grey=True, slices_per_call=2)
    ref = R.greys(hu[:, None], [CT] * 3, S)
    assert torch.equal(g16.cpu(), torch.from_numpy(ref)) and torch.equal(f16.cpu().view(torch.int32), torch.from_numpy(R.normalise(ref)).view(torch.int32))


@pytest.mark.parametrize("H0,W0,S", [(37, 53, 64), (700, 300, 16)], ids=["fused", "two_launches"])
def test_second_prepare_volume_allocates_nothing_and_is_capturable(H0, W0, S):
    import medical_sam2_amd.volume_prep as vp
    raws = [torch.from_numpy(raw_volume(np.int16, 1, H0, W0, seed=s)[:, 0]).to(DEV) for s in (1, 2)]
    refs = [torch.from_numpy(R.normalise(R.greys(r.cpu().numpy()[:, None], [CT] * 3, S))) for r in raws]
    raw = raws[0].clone()
    out = torch.empty(T, 3, S, S, dtype=torch.float32, device=DEV)
    vp.prepare_volume(raw, window=CT, size=S, out=out)                  # warms the tables (and the two-launch form's workspace)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()
    got = vp.prepare_volume(raw, window=CT, size=S, out=out)
    torch.cuda.synchronize()
    after = torch.cuda.memory_stats()
    assert got is out
    for key in ("allocation.all.allocated", "segment.all.allocated", "allocated_bytes.all.allocated"):
        assert after[key] == before[key], key
    assert torch.equal(out.cpu().view(torch.int32), refs[0].view(torch.int32))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        vp.prepare_volume(raw, window=CT, size=S, out=out)
    for k in (1, 0):                                                    # the replay reads what the raw buffer holds now
        raw.copy_(raws[k])
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu().view(torch.int32), refs[k].view(torch.int32)), k


def test_init_state_from_volume_holds_the_prepared_frames():
    import medical_sam2_amd.build_sam as bs
    import medical_sam2_amd.volume_prep as vp
    import medical_sam2_amd.weights as wts
    S = 256
    m = bs.build_sam2_video_predictor("sam2_hiera_t", device="cpu", hydra_overrides_extra=[f"++model.image_size={S}"])
    m.load_state_dict(wts.init_weights("hiera_t", 0), strict=True)
    m = m.to(DEV).eval()
    greys = np.stack([R.sample_image(100, 130, seed) for seed in (1, 2)])
    st = m.init_state_from_volume(greys)
    frames = vp.prepare_volume(greys, size=S)
    assert st["num_frames"] == 2 and st["video_height"] == S and st["video_width"] == S and st["images"].is_cuda
    assert torch.equal(st["images"].view(torch.int32), frames.view(torch.int32))
    assert torch.equal(frames.cpu().view(torch.int32), torch.from_numpy(R.normalise(R.greys(greys[:, None], None, S))).view(torch.int32))
    hu = ((greys.astype(np.int32) - 100) * 9).astype(np.int16)
    st = m.init_state_from_volume(hu, window=CT, video_height=100, video_width=130)
    assert st["video_height"] == 100 and st["video_width"] == 130
    assert torch.equal(st["images"].view(torch.int32), vp.prepare_volume(hu, window=CT, size=S).view(torch.int32))
