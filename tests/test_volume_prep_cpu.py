"""Volume intake without a GPU: the numpy restatement (tests/volume_prep_restate.py) that arbitrates the GPU tests is tied to Pillow itself,
to committed Pillow outputs, and to the loader it replaces (`data.BTCVVolumes` + `load_video_frames_from_data` + `labels_from_pack`); the
product's host tables are tied to the restatement; the window rules to exact rational arithmetic; the entries' argument checks are run
through the C ABI on host pointers that are never dereferenced.  Every comparison is exact equality."""
import ctypes
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import volume_prep_restate as R  # noqa: E402

PAIR_IDS = [f"{h}x{w}->{s}" for h, w, s in R.PAIRS]


@pytest.mark.parametrize("H0,W0,S", R.PAIRS, ids=PAIR_IDS)
def test_restatement_equals_pillow(H0, W0, S):
    Image = pytest.importorskip("PIL.Image")
    x = R.sample_image(H0, W0, H0 + W0)
    rgb = np.array(Image.fromarray(x).convert("RGB").resize((S, S)))
    mine = R.resize_bicubic(x, S)
    for c in range(3):
        assert np.array_equal(rgb[..., c], mine), (c, int((rgb[..., c] != mine).sum()))
    for m in (x > 128, x == 255, np.ones_like(x, dtype=bool)):
        assert np.array_equal(np.array(Image.fromarray(m).resize((S, S))), R.resize_nearest(m, S))


def test_restatement_equals_the_committed_pillow_outputs():
    g = np.load(os.path.join(ROOT, "tests", "golden", "volume_prep_pillow.npz"))
    pairs = [tuple(int(v) for v in p) for p in g["pairs"]]
    assert pairs == [p for p in R.PAIRS if p[2] <= 128] and len(pairs) == 9
    for i, (H0, W0, S) in enumerate(pairs):
        x = g[f"x_{i}"]
        assert x.shape == (H0, W0) and x.dtype == np.uint8
        assert np.array_equal(R.resize_bicubic(x, S), g[f"bic_{i}"]), (H0, W0, S)
        m = np.unpackbits(g[f"m_{i}"])[: H0 * W0].reshape(H0, W0).astype(bool)
        near = np.unpackbits(g[f"near_{i}"])[: S * S].reshape(S, S).astype(bool)
        assert np.array_equal(R.resize_nearest(m, S), near), (H0, W0, S)


def test_product_tables_equal_the_restatement():
    import medical_sam2_amd.volume_prep as vp
    sizes = sorted({(n, s) for h, w, s in R.PAIRS for n in (h, w)} | {(1024, 1024), (2048, 1024), (5, 8192)})
    for n, s in sizes:
        kk, bounds = vp.resample_tables(n, s)
        rk, rb = R.resample_tables(n, s)
        assert kk.dtype == np.int32 and bounds.dtype == np.int32 and kk.shape == rk.shape and bounds.shape == (s, 2)
        assert np.array_equal(kk, rk) and np.array_equal(bounds, rb), (n, s)
        nm = vp.nearest_map(n, s)
        assert nm.dtype == np.int32 and np.array_equal(nm, R.nearest_map(n, s)), (n, s)


@pytest.mark.parametrize("lo,hi", [(-160, 240), (-1000, 400), (-32768, 32767), (0, 1)])
def test_int16_window_is_round_half_up_exactly(lo, hi):
    v = np.arange(-32768, 32768, dtype=np.int64)
    got = R.window_i16(v.astype(np.int16), lo, hi)
    w = hi - lo
    half_up = [math.floor(Fraction(255 * (min(max(int(x), lo), hi) - lo), w) + Fraction(1, 2)) for x in v]
    assert got.dtype == np.uint8 and np.array_equal(got.astype(np.int64), np.array(half_up))
    assert got[0] == 0 and got[-1] == 255 and R.window_i16_exact(lo, lo, hi) == 0 and R.window_i16_exact(hi, lo, hi) == 255


def test_float32_window_specials():
    lo, hi = 0.0, 510.0                                       # 255 (t - lo) / (hi - lo) = t / 2: every odd t is an exact half-way point
    v = np.array([np.nan, np.inf, -np.inf, lo, hi, -1.0, 511.0, 1.0, 3.0, 255.0, 509.0, 0.99999994, 1.0000001, 2.0, 508.9999], dtype=np.float32)
    want = [0, 255, 0, 0, 255, 0, 255, 1, 2, 128, 255, 0, 1, 1, 254]
    got = R.window_f32(v, lo, hi)
    assert got.dtype == np.uint8 and got.tolist() == want
    # against exact rational arithmetic on the float32 values themselves, for windows whose float64 steps are not all exact
    rng = np.random.RandomState(3)
    for lo, hi in ((-160.0, 240.0), (-1000.5, 399.25), (0.0, 1.0)):
        w = hi - lo
        pts = np.concatenate([lo + (np.arange(0, 256) + 0.5) * w / 255.0, rng.uniform(lo - 10, hi + 10, 2000), [lo, hi]]).astype(np.float32)
        exact = [math.floor(Fraction(min(max(Fraction(float(x)), Fraction(lo)), Fraction(hi)) - Fraction(lo)) * 255 / Fraction(w) + Fraction(1, 2)) for x in pts]
        got = R.window_f32(pts, lo, hi).astype(np.int64)
        # float64 rounds three times before the floor: it may differ from the exact value only where the exact quotient is within
        # rounding of a half-way point; everywhere else the rule IS round half up
        frac = [abs((Fraction(min(max(Fraction(float(x)), Fraction(lo)), Fraction(hi)) - Fraction(lo)) * 255 / Fraction(w)) % 1 - Fraction(1, 2)) for x in pts]
        for a, b, f in zip(got, exact, frac):
            assert a == b or (abs(a - b) == 1 and f < Fraction(1, 10 ** 9)), (lo, hi, a, b, float(f))


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """a synthetic case in the dataset's layout (48^2, 3 objects) and its decoded raw arrays, cropped to the labelled slices as the loader does"""
    Image = pytest.importorskip("PIL.Image")
    import medical_sam2_amd.data as data
    root = str(tmp_path_factory.mktemp("btcv"))
    data.write_synthetic_case(root, "case0", n_slices=8, size=48, n_objects=3, seed=0)
    idir, mdir = (os.path.join(root, "Test", k, "case0") for k in ("image", "mask"))
    seg = np.stack([np.load(os.path.join(mdir, f"{i}.npy")) for i in range(8)])
    labelled = [i for i in range(8) if seg[i].sum() > 0]
    first, last = labelled[0], labelled[-1]
    rgb = np.stack([np.array(Image.open(os.path.join(idir, f"{i}.jpg")).convert("RGB")).transpose(2, 0, 1) for i in range(first, last + 1)])
    return root, np.ascontiguousarray(rgb), np.ascontiguousarray(seg[first: last + 1])


@pytest.mark.parametrize("S", [32, 48, 64])
def test_restated_pipeline_equals_the_loader(case, S):
    import medical_sam2_amd.data as data
    from medical_sam2_amd.video_predictor import load_video_frames_from_data
    from medical_sam2_amd.volume_labels import labels_from_pack
    root, rgb, seg = case
    pack = data.BTCVVolumes(root, image_size=S, mode="Test", video_length=len(rgb))[0]
    assert pack["image"].shape == (len(rgb), 3, S, S) and len(rgb) >= 3
    g = R.greys(rgb, None, S)
    assert np.array_equal(g.astype(np.float32), pack["image"].numpy())
    frames = load_video_frames_from_data(pack["image"], offload_video_to_cpu=True)
    mine = R.normalise(g)
    assert mine.dtype == np.float32 and np.array_equal(mine.view(np.int32), frames.numpy().view(np.int32))
    obj_list = sorted({int(o) for f in pack["label"] for o in pack["label"][f]})
    assert len(obj_list) == 3
    vol = labels_from_pack(pack["label"], obj_list).numpy()
    assert np.array_equal(R.labels(seg, S), vol) and np.array_equal(R.labels(seg, S, keep=obj_list), vol)
    assert np.array_equal(R.labels(seg, S, keep=obj_list[:1]), np.where(vol == obj_list[0], vol, 0))


def test_argument_errors_cross_the_abi_as_codes_naming_the_entry():
    from medical_sam2_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)                   # a valid host address: the checks never dereference it
    ptr = (ctypes.addressof(buf) + 15) & ~15
    m, s = (ctypes.c_float * 3)(*R.MEAN), (ctypes.c_float * 3)(*R.STD)

    def win(*pairs):
        return (ctypes.c_double * 6)(*[v for p in pairs for v in p])

    ct = (-160.0, 240.0)

    def prep(src=ptr, typ=1, T=2, Cin=1, H0=37, W0=53, S=64, w=win(ct, ct, ct), kx=ptr, bx=ptr, ksx=5, ky=ptr, by=ptr, ksy=5, mean=m, std=s,
             grey=ptr, out=ptr, ws=None, nws=0):
        return L.msam2_volume_prep(src, typ, T, Cin, H0, W0, S, w, kx, bx, ksx, ky, by, ksy, mean, std, grey, out, ws, nws, None)

    cases = {
        "null src": lambda: prep(src=None),
        "no output": lambda: prep(grey=None, out=None),
        "src_type": lambda: prep(typ=3),
        "Cin": lambda: prep(Cin=2),
        "T": lambda: prep(T=0),
        "T large": lambda: prep(T=65536),
        "H0": lambda: prep(H0=8193),
        "S": lambda: prep(S=8193, ksx=5, ksy=5),
        "no windows": lambda: prep(w=None),
        "lo >= hi": lambda: prep(w=win(ct, (5.0, 5.0), ct)),
        "nan window": lambda: prep(typ=2, w=win(ct, (float("nan"), 1.0), ct)),
        "infinite width": lambda: prep(typ=2, w=win(ct, (-1e308, 1e308), ct)),
        "int16 range": lambda: prep(w=win(ct, ct, (-32769.0, 0.0))),
        "int16 fraction": lambda: prep(w=win((0.5, 9.0), ct, ct)),
        "ksize_x": lambda: prep(ksx=7),
        "ksize_y of a skipped pass": lambda: prep(H0=64, ksy=5),
        "null table": lambda: prep(ky=None),
        "workspace": lambda: prep(H0=700, W0=300, S=16, ksx=77, ksy=177),              # too large for the fused form, no workspace given
        "workspace size": lambda: prep(H0=700, W0=300, S=16, ksx=77, ksy=177, ws=ptr, nws=2 * 3 * 700 * 16 - 1),
    }
    for what, call in cases.items():
        rc = call()
        msg = L.msam2_last_error().decode()
        assert rc < 0, (what, rc)
        assert msg.startswith("volume_prep:"), (what, msg)
    assert L.msam2_volume_prep_workspace_bytes(2, 700, 300, 16) == 2 * 3 * 700 * 16
    assert L.msam2_volume_prep_workspace_bytes(64, 512, 512, 1024) == 0 and L.msam2_volume_prep_workspace_bytes(0, 512, 512, 1024) == 0

    def lab(src=ptr, typ=3, T=2, H0=37, W0=53, S=64, ym=ptr, xm=ptr, out=ptr):
        return L.msam2_label_resize(src, typ, T, H0, W0, S, ym, xm, None, out, None)

    for what, call in {"null": lambda: lab(out=None), "maps": lambda: lab(xm=None), "type": lambda: lab(typ=4), "T": lambda: lab(T=0),
                       "W0": lambda: lab(W0=0), "S": lambda: lab(S=8193)}.items():
        rc = call()
        msg = L.msam2_last_error().decode()
        assert rc < 0 and msg.startswith("label_resize:"), (what, rc, msg)
