"""Argument contracts of the label-volume entries without a GPU: every refusal that depends on the shared limits (objects per call, slices,
rows and columns, voxels) with its return code AND its full text, through the C ABI (fake pointers: a refused call launches nothing).  The
texts differ per source file on purpose -- "of 2 .. 8192" where a voxel needs an in-plane neighbour, no voxel clause where the entry has no
voxel cap, the "T ... H0 x W0 ... S" form of the intake -- and a caller may match on them: they are pinned byte for byte.  No row passes
every check (it would reach a launch: MSAM2_ERR_LAUNCH on a machine without a GPU, which the code comparison refuses)."""
import ctypes

import pytest

MSAM2_ERR_ARG = -1
BIG = 1 << 40


def _calls():
    from medical_sam2_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    ptr = (ctypes.addressof(buf) + 15) & ~15
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)                                                         # noqa: E731

    def slices(n=2, T=2, lh=4, lw=4, H=8, W=8):
        return L.msam2_label_slices(ptr, ptr, T, n, lh, lw, H, W, 0.0, None, 0, None, 0, ptr, None, None)

    def stats(n=2, D=2, H=4, W=4):
        return L.msam2_label_stats(ptr, ptr, D, H, W, n, ptr, ptr, None)

    def pick(n=2, D=2, H=4, W=4):
        return L.msam2_label_pick(ptr, ptr, ptr, ptr, ptr, None, D, H, W, n, ptr, None)

    def components(D=2, H=4, W=4):
        return L.msam2_label_components(ptr, D, H, W, 26, ptr, ptr, ptr, BIG, None)

    def clean(n=2, D=2, H=4, W=4):
        return L.msam2_label_clean(ptr, ptr, ptr, ptr, n, None, 0, ptr, ptr, ptr, BIG, D, H, W, None)

    def overlap(n=2, D=2, H=4, W=4):
        return L.msam2_label_overlap(ptr, ptr, ptr, D, H, W, n, ptr, None)

    def edt(D=2, H=4, W=4):
        return L.msam2_label_edt(ptr, D, H, W, 1, 0, None, 1.0, 1.0, 1.0, ptr, ptr, BIG, None)

    def surface(n=2, D=2, H=4, W=4):
        m = max(n, 1)
        ids = (ctypes.c_uint8 * m)(*range(1, m + 1))
        return L.msam2_label_surface_distances(ptr, ptr, D, H, W, ids, i32(*([0, 0, 0, 1, 0, 1] * m)), (ctypes.c_int64 * (2 * m))(), i32(*([0] * (2 * m))),
                                               n, 1.0, 1.0, 1.0, ptr, 1000, ptr, ptr, BIG, None)

    def prep(T=2, H0=4, W0=4, S=4):
        return L.msam2_volume_prep(ptr, 0, T, 1, H0, W0, S, None, None, None, 0, None, None, 0, f3, f3, ptr, ptr, None, 0, None)

    def resize(T=2, H0=4, W0=4, S=4):
        return L.msam2_label_resize(ptr, 0, T, H0, W0, S, ptr, ptr, None, ptr, None)

    return L, dict(slices=slices, stats=stats, pick=pick, components=components, clean=clean, overlap=overlap, edt=edt, surface=surface, prep=prep,
                   resize=resize)


# (call, expected msam2_last_error()): the texts are what the library printed before the limits and refusals moved to common.h
CASES = [
    ("slices", dict(n=0),
     'label_slices: n = 0 objects (1 .. 32 per call)'),
    ("slices", dict(n=33),
     'label_slices: n = 33 objects (1 .. 32 per call)'),
    ("stats", dict(n=0),
     'label_stats: n = 0 objects (1 .. 32 per call)'),
    ("stats", dict(n=33),
     'label_stats: n = 33 objects (1 .. 32 per call)'),
    ("pick", dict(n=0),
     'label_pick: n = 0 objects (1 .. 32 per call)'),
    ("pick", dict(n=33),
     'label_pick: n = 33 objects (1 .. 32 per call)'),
    ("clean", dict(n=0),
     'label_clean: n = 0 objects (1 .. 32 per call)'),
    ("clean", dict(n=33),
     'label_clean: n = 33 objects (1 .. 32 per call)'),
    ("overlap", dict(n=0),
     'label_overlap: n = 0 objects (1 .. 32 per call)'),
    ("overlap", dict(n=33),
     'label_overlap: n = 33 objects (1 .. 32 per call)'),
    ("surface", dict(n=0),
     'label_surface_distances: n = 0 objects (1 .. 32 per call)'),
    ("surface", dict(n=33),
     'label_surface_distances: n = 33 objects (1 .. 32 per call)'),
    ("slices", dict(T=0),
     'label_slices: bad sizes (T 0, low-res 4x4, output 8x8)'),
    ("slices", dict(T=65536),
     'label_slices: bad sizes (T 65536, low-res 4x4, output 8x8)'),
    ("slices", dict(H=0),
     'label_slices: bad sizes (T 2, low-res 4x4, output 0x8)'),
    ("slices", dict(W=0),
     'label_slices: bad sizes (T 2, low-res 4x4, output 8x0)'),
    ("slices", dict(lh=0),
     'label_slices: bad sizes (T 2, low-res 0x4, output 8x8)'),
    ("slices", dict(lw=0),
     'label_slices: bad sizes (T 2, low-res 4x0, output 8x8)'),
    ("slices", dict(H=65536, W=32768),
     'label_slices: bad sizes (T 2, low-res 4x4, output 65536x32768)'),
    ("slices", dict(lh=65536, lw=32768),
     'label_slices: bad sizes (T 2, low-res 65536x32768, output 8x8)'),
    ("stats", dict(D=0),
     'label_stats: bad sizes (D 0 of 1 .. 65535, H x W 4x4 of 1 .. 8192)'),
    ("stats", dict(D=65536),
     'label_stats: bad sizes (D 65536 of 1 .. 65535, H x W 4x4 of 1 .. 8192)'),
    ("stats", dict(H=0),
     'label_stats: bad sizes (D 2 of 1 .. 65535, H x W 0x4 of 1 .. 8192)'),
    ("stats", dict(H=8193),
     'label_stats: bad sizes (D 2 of 1 .. 65535, H x W 8193x4 of 1 .. 8192)'),
    ("stats", dict(W=0),
     'label_stats: bad sizes (D 2 of 1 .. 65535, H x W 4x0 of 1 .. 8192)'),
    ("stats", dict(W=8193),
     'label_stats: bad sizes (D 2 of 1 .. 65535, H x W 4x8193 of 1 .. 8192)'),
    ("pick", dict(D=0),
     'label_pick: bad sizes (D 0 of 1 .. 65535, H x W 4x4 of 1 .. 8192)'),
    ("pick", dict(D=65536),
     'label_pick: bad sizes (D 65536 of 1 .. 65535, H x W 4x4 of 1 .. 8192)'),
    ("pick", dict(H=0),
     'label_pick: bad sizes (D 2 of 1 .. 65535, H x W 0x4 of 1 .. 8192)'),
    ("pick", dict(H=8193),
     'label_pick: bad sizes (D 2 of 1 .. 65535, H x W 8193x4 of 1 .. 8192)'),
    ("pick", dict(W=0),
     'label_pick: bad sizes (D 2 of 1 .. 65535, H x W 4x0 of 1 .. 8192)'),
    ("pick", dict(W=8193),
     'label_pick: bad sizes (D 2 of 1 .. 65535, H x W 4x8193 of 1 .. 8192)'),
    ("components", dict(D=0),
     'label_components: bad sizes (D 0 of 1 .. 65535, H x W 4x4 of 1 .. 8192, at most 2^31 - 2 voxels)'),
    ("components", dict(D=65536),
     'label_components: bad sizes (D 65536 of 1 .. 65535, H x W 4x4 of 1 .. 8192, at most 2^31 - 2 voxels)'),
    ("components", dict(H=0),
     'label_components: bad sizes (D 2 of 1 .. 65535, H x W 0x4 of 1 .. 8192, at most 2^31 - 2 voxels)'),
    ("components", dict(H=8193),
     'label_components: bad sizes (D 2 of 1 .. 65535, H x W 8193x4 of 1 .. 8192, at most 2^31 - 2 voxels)'),
    ("components", dict(W=0),
     'label_components: bad sizes (D 2 of 1 .. 65535, H x W 4x0 of 1 .. 8192, at most 2^31 - 2 voxels)'),
    ("components", dict(W=8193),
     'label_components: bad sizes (D 2 of 1 .. 65535, H x W 4x8193 of 1 .. 8192, at most 2^31 - 2 voxels)'),
    ("components", dict(D=33, H=8192, W=8192),
     'label_components: bad sizes (D 33 of 1 .. 65535, H x W 8192x8192 of 1 .. 8192, at most 2^31 - 2 voxels)'),
    ("clean", dict(D=0),
     'label_clean: bad sizes (D 0 of 1 .. 65535, H x W 4x4 of 1 .. 8192, at most 2^31 - 2 voxels)'),
    ("clean", dict(D=65536),
     'label_clean: bad sizes (D 65536 of 1 .. 65535, H x W 4x4 of 1 .. 8192, at most 2^31 - 2 voxels)'),
    ("clean", dict(H=0),
     'label_clean: bad sizes (D 2 of 1 .. 65535, H x W 0x4 of 1 .. 8192, at most 2^31 - 2 voxels)'),
    ("clean", dict(H=8193),
     'label_clean: bad sizes (D 2 of 1 .. 65535, H x W 8193x4 of 1 .. 8192, at most 2^31 - 2 voxels)'),
    ("clean", dict(W=0),
     'label_clean: bad sizes (D 2 of 1 .. 65535, H x W 4x0 of 1 .. 8192, at most 2^31 - 2 voxels)'),
    ("clean", dict(W=8193),
     'label_clean: bad sizes (D 2 of 1 .. 65535, H x W 4x8193 of 1 .. 8192, at most 2^31 - 2 voxels)'),
    ("clean", dict(D=33, H=8192, W=8192),
     'label_clean: bad sizes (D 33 of 1 .. 65535, H x W 8192x8192 of 1 .. 8192, at most 2^31 - 2 voxels)'),
    ("overlap", dict(D=0),
     'label_overlap: bad sizes (D 0 of 1 .. 65535, H x W 4x4 of 1 .. 8192, at most 2^31 - 2 voxels)'),
    ("overlap", dict(D=65536),
     'label_overlap: bad sizes (D 65536 of 1 .. 65535, H x W 4x4 of 1 .. 8192, at most 2^31 - 2 voxels)'),
    ("overlap", dict(H=0),
     'label_overlap: bad sizes (D 2 of 1 .. 65535, H x W 0x4 of 1 .. 8192, at most 2^31 - 2 voxels)'),
    ("overlap", dict(H=8193),
     'label_overlap: bad sizes (D 2 of 1 .. 65535, H x W 8193x4 of 1 .. 8192, at most 2^31 - 2 voxels)'),
    ("overlap", dict(W=0),
     'label_overlap: bad sizes (D 2 of 1 .. 65535, H x W 4x0 of 1 .. 8192, at most 2^31 - 2 voxels)'),
    ("overlap", dict(W=8193),
     'label_overlap: bad sizes (D 2 of 1 .. 65535, H x W 4x8193 of 1 .. 8192, at most 2^31 - 2 voxels)'),
    ("overlap", dict(D=33, H=8192, W=8192),
     'label_overlap: bad sizes (D 33 of 1 .. 65535, H x W 8192x8192 of 1 .. 8192, at most 2^31 - 2 voxels)'),
    ("edt", dict(D=0),
     'label_edt: bad sizes (D 0 of 1 .. 65535, H x W 4x4 of 2 .. 8192, at most 2^31 - 2 voxels)'),
    ("edt", dict(D=65536),
     'label_edt: bad sizes (D 65536 of 1 .. 65535, H x W 4x4 of 2 .. 8192, at most 2^31 - 2 voxels)'),
    ("edt", dict(H=0),
     'label_edt: bad sizes (D 2 of 1 .. 65535, H x W 0x4 of 2 .. 8192, at most 2^31 - 2 voxels)'),
    ("edt", dict(H=8193),
     'label_edt: bad sizes (D 2 of 1 .. 65535, H x W 8193x4 of 2 .. 8192, at most 2^31 - 2 voxels)'),
    ("edt", dict(W=0),
     'label_edt: bad sizes (D 2 of 1 .. 65535, H x W 4x0 of 2 .. 8192, at most 2^31 - 2 voxels)'),
    ("edt", dict(W=8193),
     'label_edt: bad sizes (D 2 of 1 .. 65535, H x W 4x8193 of 2 .. 8192, at most 2^31 - 2 voxels)'),
    ("edt", dict(H=1),
     'label_edt: bad sizes (D 2 of 1 .. 65535, H x W 1x4 of 2 .. 8192, at most 2^31 - 2 voxels)'),
    ("edt", dict(W=1),
     'label_edt: bad sizes (D 2 of 1 .. 65535, H x W 4x1 of 2 .. 8192, at most 2^31 - 2 voxels)'),
    ("edt", dict(D=33, H=8192, W=8192),
     'label_edt: bad sizes (D 33 of 1 .. 65535, H x W 8192x8192 of 2 .. 8192, at most 2^31 - 2 voxels)'),
    ("surface", dict(D=0),
     'label_surface_distances: bad sizes (D 0 of 1 .. 65535, H x W 4x4 of 2 .. 8192, at most 2^31 - 2 voxels)'),
    ("surface", dict(D=65536),
     'label_surface_distances: bad sizes (D 65536 of 1 .. 65535, H x W 4x4 of 2 .. 8192, at most 2^31 - 2 voxels)'),
    ("surface", dict(H=0),
     'label_surface_distances: bad sizes (D 2 of 1 .. 65535, H x W 0x4 of 2 .. 8192, at most 2^31 - 2 voxels)'),
    ("surface", dict(H=8193),
     'label_surface_distances: bad sizes (D 2 of 1 .. 65535, H x W 8193x4 of 2 .. 8192, at most 2^31 - 2 voxels)'),
    ("surface", dict(W=0),
     'label_surface_distances: bad sizes (D 2 of 1 .. 65535, H x W 4x0 of 2 .. 8192, at most 2^31 - 2 voxels)'),
    ("surface", dict(W=8193),
     'label_surface_distances: bad sizes (D 2 of 1 .. 65535, H x W 4x8193 of 2 .. 8192, at most 2^31 - 2 voxels)'),
    ("surface", dict(H=1),
     'label_surface_distances: bad sizes (D 2 of 1 .. 65535, H x W 1x4 of 2 .. 8192, at most 2^31 - 2 voxels)'),
    ("surface", dict(W=1),
     'label_surface_distances: bad sizes (D 2 of 1 .. 65535, H x W 4x1 of 2 .. 8192, at most 2^31 - 2 voxels)'),
    ("surface", dict(D=33, H=8192, W=8192),
     'label_surface_distances: bad sizes (D 33 of 1 .. 65535, H x W 8192x8192 of 2 .. 8192, at most 2^31 - 2 voxels)'),
    ("prep", dict(T=0),
     'volume_prep: bad sizes (T 0 of 1 .. 65535, H0 x W0 4x4 and S 4 of 1 .. 8192)'),
    ("prep", dict(T=65536),
     'volume_prep: bad sizes (T 65536 of 1 .. 65535, H0 x W0 4x4 and S 4 of 1 .. 8192)'),
    ("prep", dict(H0=0),
     'volume_prep: bad sizes (T 2 of 1 .. 65535, H0 x W0 0x4 and S 4 of 1 .. 8192)'),
    ("prep", dict(H0=8193),
     'volume_prep: bad sizes (T 2 of 1 .. 65535, H0 x W0 8193x4 and S 4 of 1 .. 8192)'),
    ("prep", dict(W0=0),
     'volume_prep: bad sizes (T 2 of 1 .. 65535, H0 x W0 4x0 and S 4 of 1 .. 8192)'),
    ("prep", dict(W0=8193),
     'volume_prep: bad sizes (T 2 of 1 .. 65535, H0 x W0 4x8193 and S 4 of 1 .. 8192)'),
    ("prep", dict(S=0),
     'volume_prep: bad sizes (T 2 of 1 .. 65535, H0 x W0 4x4 and S 0 of 1 .. 8192)'),
    ("prep", dict(S=8193),
     'volume_prep: bad sizes (T 2 of 1 .. 65535, H0 x W0 4x4 and S 8193 of 1 .. 8192)'),
    ("resize", dict(T=0),
     'label_resize: bad sizes (T 0 of 1 .. 65535, H0 x W0 4x4 and S 4 of 1 .. 8192)'),
    ("resize", dict(T=65536),
     'label_resize: bad sizes (T 65536 of 1 .. 65535, H0 x W0 4x4 and S 4 of 1 .. 8192)'),
    ("resize", dict(H0=0),
     'label_resize: bad sizes (T 2 of 1 .. 65535, H0 x W0 0x4 and S 4 of 1 .. 8192)'),
    ("resize", dict(H0=8193),
     'label_resize: bad sizes (T 2 of 1 .. 65535, H0 x W0 8193x4 and S 4 of 1 .. 8192)'),
    ("resize", dict(W0=0),
     'label_resize: bad sizes (T 2 of 1 .. 65535, H0 x W0 4x0 and S 4 of 1 .. 8192)'),
    ("resize", dict(W0=8193),
     'label_resize: bad sizes (T 2 of 1 .. 65535, H0 x W0 4x8193 and S 4 of 1 .. 8192)'),
    ("resize", dict(S=0),
     'label_resize: bad sizes (T 2 of 1 .. 65535, H0 x W0 4x4 and S 0 of 1 .. 8192)'),
    ("resize", dict(S=8193),
     'label_resize: bad sizes (T 2 of 1 .. 65535, H0 x W0 4x4 and S 8193 of 1 .. 8192)'),
]


# ---- the entries that work per organ inside a box, and the refusals beside the limits ------------------------------------------------------
# Rows that the entries' own files check by substring or not at all (test_label_holes_cpu.py and test_label_measure_cpu.py pin most of
# theirs byte for byte already; msam2_label_measure has no row here: every one of its refusals is pinned there).  The texts and the
# workspace sizes are what the library of the commit BEFORE the box helpers moved to csrc/label_boxes.h printed and returned, taken from
# a build of that commit, not from the code under test.
def _box_calls():
    from medical_sam2_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(8192)
    ptr = (ctypes.addressof(buf) + 15) & ~15
    i32 = lambda v: (ctypes.c_int32 * len(v))(*v)                                                          # noqa: E731
    u8 = lambda v: (ctypes.c_uint8 * len(v))(*v)                                                           # noqa: E731
    f64 = lambda v: (ctypes.c_double * len(v))(*v)                                                         # noqa: E731
    at = lambda off: None if off is None else ptr + off                                                    # noqa: E731

    # labels at ptr, 4 x 6 x 8 = 192 bytes; out 2048 bytes behind it unless the row says otherwise
    def holes(n=1, c=6, claim=0, ids=(3,), boxes=(0, 3, 0, 5, 0, 7), out=2048, info=4096, ws=4112, nb=BIG):
        return L.msam2_label_fill_holes(ptr, 4, 6, 8, u8(ids), i32(boxes), n, c, None, claim, at(out), at(info), at(ws), nb, None)

    def morph(n=1, H=6, op=0, claim=0, values=(3,), boxes=(0, 3, 0, 5, 0, 7), r2=(1.0,), sp=(1.0, 1.0, 1.0), labels=0, out=2048, info=4096, ws=4112,
              nb=BIG, D=4, W=8):
        return L.msam2_label_morph(at(labels), D, H, W, u8(values), i32(boxes), n, op, f64(r2), sp[0], sp[1], sp[2], claim, at(out), at(info),
                                   at(ws), nb, None)

    def clicks(pred=0, gt=0, ids=0, k=None, u=None, D=1, H=8, W=8, n=2, mode=0, out=0, ws=0, nb=1 << 20):
        return L.msam2_label_error_clicks(at(pred), at(gt), at(ids), at(k), at(u), D, H, W, n, mode, at(out), at(ws), nb, None)

    def edt(D=4, H=8, W=16, value=1, features=0, box=None, sp=(1.0, 1.0, 1.0), labels=0, d2=0, ws=0, nb=BIG):
        return L.msam2_label_edt(at(labels), D, H, W, value, features, None if box is None else i32(box), sp[0], sp[1], sp[2], at(d2), at(ws), nb,
                                 None)

    def surface(n=2, D=4, H=8, W=16, boxes=(0, 3, 0, 7, 0, 15) * 2, offs=(0, 10, 20, 30), caps=(10, 10, 10, 10), sp=(1.0, 1.0, 1.0), length=40,
                gt=0, dist=0, counts=0, ws=0, nb=BIG):
        return L.msam2_label_surface_distances(ptr, at(gt), D, H, W, u8((1, 2)), i32(boxes), (ctypes.c_int64 * 4)(*offs), i32(caps), n, sp[0], sp[1],
                                               sp[2], at(dist), length, at(counts), at(ws), nb, None)

    return L, dict(holes=holes, morph=morph, clicks=clicks, edt=edt, surface=surface), i32, f64


NAN, INF = float("nan"), float("inf")
BOX_CASES = [
    ('holes', dict(c=0),
     'label_fill_holes: connectivity 0 of the background flood (6, 18 or 26 in 3-D; 4 or 8 slice by slice)'),
    ('holes', dict(n=2, ids=(3, 4), boxes=(0, 3, 0, 5, 0, 7, 0, 3, 0, 6, 0, 7)),
     'label_fill_holes: box 1 (0..3, 0..6, 0..7) is inverted or outside the 4 x 6 x 8 volume'),
    ('holes', dict(n=3, ids=(3, 4, 3), boxes=(0, 3, 0, 5, 0, 7, 0, 3, 0, 5, 0, 7, 0, 3, 0, 5, 0, 7)),
     'label_fill_holes: ids[0] and ids[2] are both 3'),
    ('holes', dict(out=191),
     'label_fill_holes: out overlaps labels without being labels'),
    ('holes', dict(out=-191),
     'label_fill_holes: out overlaps labels without being labels'),
    ('holes', dict(n=2, ids=(3, 4), boxes=(0, 1, 0, 5, 0, 7, 1, 3, 1, 4, 2, 6), nb=559),
     'label_fill_holes: workspace too small (559 of 560 bytes)'),
    ('holes', dict(info=4098),
     'label_fill_holes: the workspace must be 16-byte aligned, info and max_voxels 4-byte'),
    ('morph', dict(op=4),
     'label_morph: op 4 (0: erode, 1: dilate, 2: open, 3: close)'),
    ('morph', dict(op=-1),
     'label_morph: op -1 (0: erode, 1: dilate, 2: open, 3: close)'),
    ('morph', dict(claim=2),
     'label_morph: claim 2 (0: background voxels only, 1: any voxel whose value is not in values)'),
    ('morph', dict(r2=(-1.0,)),
     'label_morph: r2[0] = -1 (a squared radius: >= 0 and finite)'),
    ('morph', dict(r2=(NAN,)),
     'label_morph: r2[0] = nan (a squared radius: >= 0 and finite)'),
    ('morph', dict(r2=(INF,)),
     'label_morph: r2[0] = inf (a squared radius: >= 0 and finite)'),
    ('morph', dict(n=0),
     'label_morph: n = 0 objects (1 .. 32 per call)'),
    ('morph', dict(n=33),
     'label_morph: n = 33 objects (1 .. 32 per call)'),
    ('morph', dict(H=1),
     'label_morph: bad sizes (D 4 of 1 .. 65535, H x W 1x8 of 2 .. 8192, at most 2^31 - 2 voxels)'),
    ('morph', dict(H=8193),
     'label_morph: bad sizes (D 4 of 1 .. 65535, H x W 8193x8 of 2 .. 8192, at most 2^31 - 2 voxels)'),
    ('morph', dict(values=(0,)),
     'label_morph: values[0] is 0, the background'),
    ('morph', dict(n=2, values=(7, 7), boxes=(0, 3, 0, 5, 0, 7, 0, 3, 0, 5, 0, 7), r2=(1.0, 1.0)),
     'label_morph: values[0] and values[1] are both 7'),
    ('morph', dict(n=2, values=(7, 8), boxes=(0, 3, 0, 5, 0, 7, 0, 4, 0, 5, 0, 7), r2=(1.0, 1.0)),
     'label_morph: box 1 (0..4, 0..5, 0..7) is inverted or outside the 4 x 6 x 8 volume'),
    ('morph', dict(boxes=(2, 1, 0, 5, 0, 7)),
     'label_morph: box 0 (2..1, 0..5, 0..7) is inverted or outside the 4 x 6 x 8 volume'),
    ('morph', dict(sp=(1.0, 0.0, 1.0)),
     'label_morph: spacing (1, 0, 1): every value must be positive with a square in 2.3e-308 .. 2.6e297'),
    ('morph', dict(sp=(-1.0, 1.0, 1.0)),
     'label_morph: spacing (-1, 1, 1): every value must be positive with a square in 2.3e-308 .. 2.6e297'),
    ('morph', dict(sp=(1.0, 1.0, NAN)),
     'label_morph: spacing (1, 1, nan): every value must be positive with a square in 2.3e-308 .. 2.6e297'),
    ('morph', dict(sp=(1.0, 1e+150, 1.0)),
     'label_morph: spacing (1, 1e+150, 1): every value must be positive with a square in 2.3e-308 .. 2.6e297'),
    ('morph', dict(sp=(1e-155, 1.0, 1.0)),
     'label_morph: spacing (1e-155, 1, 1): every value must be positive with a square in 2.3e-308 .. 2.6e297'),
    ('morph', dict(D=65535, H=8192, W=2, boxes=(0, 65534, 0, 8191, 0, 1)),
     'label_morph: the grown box 0 has more than 2^25 rows (slices x rows: 536862720)'),
    ('morph', dict(out=100),
     'label_morph: out overlaps labels without being labels'),
    ('morph', dict(out=-100),
     'label_morph: out overlaps labels without being labels'),
    ('morph', dict(nb=64),
     'label_morph: workspace too small (64 of 2128 bytes)'),
    ('morph', dict(op=1, out=0, nb=5391),
     'label_morph: workspace too small (5391 of 5392 bytes)'),
    ('morph', dict(ws=4120),
     'label_morph: the workspace must be 16-byte aligned, info 4-byte'),
    ('morph', dict(info=4098),
     'label_morph: the workspace must be 16-byte aligned, info 4-byte'),
    ('morph', dict(labels=None),
     'label_morph: null labels / values / boxes / r2 / out / info / workspace'),
    ('clicks', dict(pred=None),
     'label_error_clicks: null pred / gt / ids / clicks / workspace'),
    ('clicks', dict(mode=2),
     'label_error_clicks: mode 2 (0: centre of the largest error, 1: uniform over the error)'),
    ('clicks', dict(mode=-1),
     'label_error_clicks: mode -1 (0: centre of the largest error, 1: uniform over the error)'),
    ('clicks', dict(mode=1),
     'label_error_clicks: mode 1 needs exactly one of k (indices) and u (uniform words), mode 0 neither'),
    ('clicks', dict(mode=1, k=0, u=0),
     'label_error_clicks: mode 1 needs exactly one of k (indices) and u (uniform words), mode 0 neither'),
    ('clicks', dict(k=0),
     'label_error_clicks: mode 1 needs exactly one of k (indices) and u (uniform words), mode 0 neither'),
    ('clicks', dict(n=0),
     'label_error_clicks: n = 0 objects (1 .. 32 per call)'),
    ('clicks', dict(n=33),
     'label_error_clicks: n = 33 objects (1 .. 32 per call)'),
    ('clicks', dict(D=0),
     'label_error_clicks: bad sizes (D 0 of 1 .. 65535, H x W 8x8 of 1 .. 8192, at most 2^31 - 2 voxels)'),
    ('clicks', dict(H=8193),
     'label_error_clicks: bad sizes (D 1 of 1 .. 65535, H x W 8193x8 of 1 .. 8192, at most 2^31 - 2 voxels)'),
    ('clicks', dict(W=0),
     'label_error_clicks: bad sizes (D 1 of 1 .. 65535, H x W 8x0 of 1 .. 8192, at most 2^31 - 2 voxels)'),
    ('clicks', dict(D=33, H=8192, W=8192),
     'label_error_clicks: bad sizes (D 33 of 1 .. 65535, H x W 8192x8192 of 1 .. 8192, at most 2^31 - 2 voxels)'),
    ('clicks', dict(nb=287),
     'label_error_clicks: workspace too small (287 of 288 bytes)'),
    ('clicks', dict(mode=1, k=0, nb=63),
     'label_error_clicks: workspace too small (63 of 64 bytes)'),
    ('clicks', dict(ws=4),
     'label_error_clicks: the workspace must be 8-byte aligned, clicks 4-byte'),
    ('clicks', dict(out=2),
     'label_error_clicks: the workspace must be 8-byte aligned, clicks 4-byte'),
    ('edt', dict(labels=None),
     'label_edt: null labels / d2 / workspace'),
    ('edt', dict(value=256),
     'label_edt: value 256 (0 .. 255)'),
    ('edt', dict(value=-1),
     'label_edt: value -1 (0 .. 255)'),
    ('edt', dict(features=2),
     'label_edt: features 2 (0: the surface of value, 1: the voxels != value)'),
    ('edt', dict(sp=(1.0, 0.0, 1.0)),
     'label_edt: spacing (1, 0, 1): every value must be positive with a square in 2.3e-308 .. 2.6e297'),
    ('edt', dict(sp=(-1.0, 1.0, 1.0)),
     'label_edt: spacing (-1, 1, 1): every value must be positive with a square in 2.3e-308 .. 2.6e297'),
    ('edt', dict(sp=(1.0, 1.0, NAN)),
     'label_edt: spacing (1, 1, nan): every value must be positive with a square in 2.3e-308 .. 2.6e297'),
    ('edt', dict(sp=(INF, 1.0, 1.0)),
     'label_edt: spacing (inf, 1, 1): every value must be positive with a square in 2.3e-308 .. 2.6e297'),
    ('edt', dict(sp=(1.0, 1e+150, 1.0)),
     'label_edt: spacing (1, 1e+150, 1): every value must be positive with a square in 2.3e-308 .. 2.6e297'),
    ('edt', dict(sp=(1.0, 1.0, 1e-155)),
     'label_edt: spacing (1, 1, 1e-155): every value must be positive with a square in 2.3e-308 .. 2.6e297'),
    ('edt', dict(box=(2, 1, 0, 7, 0, 15)),
     'label_edt: box (2..1, 0..7, 0..15) is inverted or outside the 4 x 8 x 16 volume'),
    ('edt', dict(box=(0, 3, 0, 8, 0, 15)),
     'label_edt: box (0..3, 0..8, 0..15) is inverted or outside the 4 x 8 x 16 volume'),
    ('edt', dict(box=(0, 3, 0, 7, -1, 15)),
     'label_edt: box (0..3, 0..7, -1..15) is inverted or outside the 4 x 8 x 16 volume'),
    ('edt', dict(D=65535, H=8192, W=2),
     'label_edt: the box has more than 2^25 rows (slices x rows: 536862720)'),
    ('edt', dict(nb=5119),
     'label_edt: workspace too small (5119 of 5136 bytes)'),
    ('edt', dict(ws=4),
     'label_edt: d2 / workspace must be 8-byte aligned'),
    ('edt', dict(d2=4),
     'label_edt: d2 / workspace must be 8-byte aligned'),
    ('surface', dict(gt=None),
     'label_surface_distances: null pred / gt / ids / boxes / seg_offsets / capacity / dist / counts / workspace'),
    ('surface', dict(sp=(0.0, 1.0, 1.0)),
     'label_surface_distances: spacing (0, 1, 1): every value must be positive with a square in 2.3e-308 .. 2.6e297'),
    ('surface', dict(sp=(1.0, 1.0, -2.0)),
     'label_surface_distances: spacing (1, 1, -2): every value must be positive with a square in 2.3e-308 .. 2.6e297'),
    ('surface', dict(sp=(1e+150, 1.0, 1.0)),
     'label_surface_distances: spacing (1e+150, 1, 1): every value must be positive with a square in 2.3e-308 .. 2.6e297'),
    ('surface', dict(length=-1),
     'label_surface_distances: dist_len -1'),
    ('surface', dict(boxes=(0, 3, 5, 4, 0, 15, 0, 3, 0, 7, 0, 15)),
     'label_surface_distances: box 0 (0..3, 5..4, 0..15) is inverted or outside the 4 x 8 x 16 volume'),
    ('surface', dict(boxes=(0, 3, 0, 7, 0, 15, 0, 4, 0, 7, 0, 15)),
     'label_surface_distances: box 1 (0..4, 0..7, 0..15) is inverted or outside the 4 x 8 x 16 volume'),
    ('surface', dict(n=1, D=65535, H=8192, W=2, boxes=(0, 65534, 0, 8191, 0, 1, 0, 65534, 0, 8191, 0, 1)),
     'label_surface_distances: box 0 has more than 2^25 rows (slices x rows: 536862720)'),
    ('surface', dict(length=39),
     'label_surface_distances: segment (1, 1) = [30, 30 + 10) leaves dist (39 elements)'),
    ('surface', dict(caps=(10, 10, -1, 10)),
     'label_surface_distances: segment (1, 0) = [20, 20 + -1) leaves dist (40 elements)'),
    ('surface', dict(offs=(0, 10, 20, -1)),
     'label_surface_distances: segment (1, 1) = [-1, -1 + 10) leaves dist (40 elements)'),
    ('surface', dict(nb=20543),
     'label_surface_distances: workspace too small (20543 of 20544 bytes)'),
    ('surface', dict(ws=4),
     'label_surface_distances: dist / workspace must be 8-byte aligned, counts 4-byte'),
    ('surface', dict(dist=4),
     'label_surface_distances: dist / workspace must be 8-byte aligned, counts 4-byte'),
    ('surface', dict(counts=2),
     'label_surface_distances: dist / workspace must be 8-byte aligned, counts 4-byte'),
]


@pytest.mark.parametrize("entry, bad, text", BOX_CASES, ids=["%s(%s)" % (e, ", ".join("%s=%r" % kv for kv in b.items())) for e, b, _ in BOX_CASES])
def test_box_entry_refusal_code_and_text(entry, bad, text):
    L, calls, _, _ = _box_calls()
    rc = calls[entry](**bad)
    assert rc == MSAM2_ERR_ARG, (rc, L.msam2_last_error().decode())
    assert L.msam2_last_error().decode() == text


def test_box_entry_workspace_bytes():
    """the sizes the queries returned before the move, byte for byte: head 16, snapshot and tables rounded to 16, 0 for every bad argument"""
    L, _, i32, f64 = _box_calls()
    two = i32((1, 3, 1, 4, 2, 6, 0, 1, 0, 5, 0, 7))              # 3 x 4 x 5 = 60 voxels; the second box is two slices thin
    holes = lambda n=2, c=6, in_place=0, all_at_once=0, D=4, boxes=two: L.msam2_label_fill_holes_workspace_bytes(D, 6, 8, boxes, n, c, in_place, all_at_once)   # noqa: E731
    morph = lambda op, n=2, in_place=0, all_at_once=0, r2=(2.0, 0.0), sp=(2.5, 1.0, 1.0): L.msam2_label_morph_workspace_bytes(                # noqa: E731
        4, 6, 8, two, n, op, f64(r2), sp[0], sp[1], sp[2], in_place, all_at_once)
    got = {
        "holes": holes(), "holes all": holes(all_at_once=1), "holes in place": holes(in_place=1), "holes in plane": holes(c=8, all_at_once=1),
        "holes one": holes(n=1), "holes c": holes(c=5), "holes n": holes(n=33), "holes D": holes(D=3), "holes null": holes(boxes=None),
        "erode": morph(0), "erode all": morph(0, all_at_once=1), "dilate": morph(1), "dilate all in place": morph(1, in_place=1, all_at_once=1),
        "open": morph(2), "close": morph(3), "close anisotropic": morph(3, sp=(1.0, 0.5, 0.5)), "morph op": morph(4), "morph r2": morph(0, r2=(2.0, -1.0)),
        "morph spacing": morph(0, sp=(1.0, 0.0, 1.0)),
        "clicks centre": L.msam2_label_error_clicks_workspace_bytes(3, 8, 5, 2, 0), "clicks uniform": L.msam2_label_error_clicks_workspace_bytes(3, 8, 5, 2, 1),
        "clicks n": L.msam2_label_error_clicks_workspace_bytes(3, 8, 5, 33, 0),
        "edt": L.msam2_label_edt_workspace_bytes(3, 4, 5), "edt thin": L.msam2_label_edt_workspace_bytes(1, 1, 7),
        "edt rows": L.msam2_label_edt_workspace_bytes(65535, 8192, 2), "edt side": L.msam2_label_edt_workspace_bytes(1, 8193, 2),
        "surface": L.msam2_label_surface_distances_workspace_bytes(two, 2), "surface one": L.msam2_label_surface_distances_workspace_bytes(two, 1),
        "surface inverted": L.msam2_label_surface_distances_workspace_bytes(i32((2, 1, 0, 3, 0, 3)), 1),
        "surface n": L.msam2_label_surface_distances_workspace_bytes(two, 33),
    }
    assert got == {
        'holes': 560, 'holes all': 560, 'holes in place': 752, 'holes in plane': 1424, 'holes one': 560, 'holes c': 0, 'holes n': 0, 'holes D': 0,
        'holes null': 0, 'erode': 1872, 'erode all': 3456, 'dilate': 3952, 'dilate all in place': 5968, 'open': 1872, 'close': 5200,
        'close anisotropic': 5200, 'morph op': 0, 'morph r2': 0, 'morph spacing': 0, 'clicks centre': 576, 'clicks uniform': 192, 'clicks n': 0,
        'edt': 616, 'edt thin': 80, 'edt rows': 0, 'edt side': 0, 'surface': 3168, 'surface one': 1232, 'surface inverted': 0, 'surface n': 0,
    }


@pytest.mark.parametrize("entry, bad, text", CASES, ids=["%s(%s)" % (e, ", ".join("%s=%d" % kv for kv in b.items())) for e, b, _ in CASES])
def test_refusal_code_and_text(entry, bad, text):
    L, calls = _calls()
    rc = calls[entry](**bad)
    assert rc == MSAM2_ERR_ARG, (rc, L.msam2_last_error().decode())
    assert L.msam2_last_error().decode() == text


def test_wrapper_refusals_keep_their_text():
    """the refusals of the ops wrappers that need no device (host tensors: nothing is launched), whole texts: the table check every label entry
    shares names the tensor, the dtype, the shape and whose device it must be on"""
    import torch

    import medical_sam2_amd.ops as ops
    logits, vol = torch.zeros(2, 2, 4, 4), torch.zeros(2, 4, 6, dtype=torch.uint8)
    tab = torch.zeros(2, 4, 6, dtype=torch.int32)
    cases = [
        (lambda: ops.label_slices(logits, [1, 2], 8, 8, gt=torch.zeros(2, 8, 8, dtype=torch.int32)),
         "label_slices: gt must be uint8 contiguous [2, 8, 8] on the logits' device"),
        (lambda: ops.label_slices(logits, [1, 2], 8, 8, labels=torch.zeros(2, 8, 9, dtype=torch.uint8)),
         "label_slices: labels must be uint8 contiguous [2, 8, 8] on the logits' device"),
        (lambda: ops.label_ids([1, 256], "cpu"), "label_slices: ids must be integers in 1 .. 255 (0 is the background)"),
        (lambda: ops.label_ids([], "cpu"), "label_slices: ids must be integers in 1 .. 255 (0 is the background)"),
        (lambda: ops.label_ids([7, 7], "cpu"), "label_slices: ids must be distinct"),
        (lambda: ops.label_stats(torch.zeros(1, 1, 8193, dtype=torch.uint8), [1]),
         "label_stats: sizes 1 x 1 x 8193 (1 .. 65535 slices of 1 .. 8192 rows and columns)"),
        (lambda: ops.label_pick(vol.to(torch.int16), [1], tab, tab, k=tab), "label_pick: labels must be a uint8 contiguous [D, H, W] label volume"),
        (lambda: ops.label_clean(vol, tab, tab, list(range(1, 34))), "label_clean: ids must be 1 .. 32 uint8 label values, got 33"),
        (lambda: ops.label_overlap(vol, vol, [1]), "label_overlap: the label volume must be on the GPU"),
        (lambda: ops.label_edt(vol[:, :1].contiguous(), 1), "label_edt: the label volume must be on the GPU"),
    ]
    for call, text in cases:
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text


def test_box_wrapper_helpers_keep_their_text(monkeypatch):
    """the three refusals that surface_segments, label_fill_holes and label_morph share through one preparation path in ops.py, whole texts
    as the wrappers raised them when each spelled them out; host tensors, and label_stats replaced by a table: nothing is launched"""
    import torch

    import medical_sam2_amd.ops as ops
    vol = torch.zeros(2, 4, 6, dtype=torch.uint8)
    stats = torch.tensor([[[0, -1, -1, -1, -1], [3, 1, 2, 0, 4]], [[0, -1, -1, -1, -1], [2, 3, 3, 5, 5]]], dtype=torch.int32)   # [D, n, 5]
    monkeypatch.setattr(ops, "label_stats", lambda labels, ids: (stats, None))
    u8 = lambda *v: torch.tensor(v, dtype=torch.uint8)                                                     # noqa: E731
    cases = [
        (lambda: ops._organ_boxes("label_fill_holes", (vol,), u8(7, 7)), "label_fill_holes: ids must be distinct values in 1 .. 255"),
        (lambda: ops._organ_boxes("label_morph", (vol,), u8(0, 3)), "label_morph: ids must be distinct values in 1 .. 255"),
        (lambda: ops._box_workspace("label_surface_distances", [5, 9], [100, 2000], 2100, 1000, "cpu"),
         "label_surface_distances: the box of id 9 alone needs a workspace of 2000 bytes, workspace_bytes is 1000"),
        (lambda: ops._box_workspace("label_fill_holes", [5], [1001], 1001, 1000, "cpu"),
         "label_fill_holes: the box of id 5 alone needs a workspace of 1001 bytes, workspace_bytes is 1000"),
        (lambda: ops._out_volume("label_fill_holes", vol, torch.zeros(2, 4, 7, dtype=torch.uint8)),
         "label_fill_holes: out must be uint8 contiguous [2, 4, 6] on the labels' device"),
        (lambda: ops._out_volume("label_morph", vol, torch.zeros(2, 4, 6, dtype=torch.int8)),
         "label_morph: out must be uint8 contiguous [2, 4, 6] on the labels' device"),
        (lambda: ops._out_volume("label_morph", vol, torch.zeros(2, 4, 12, dtype=torch.uint8)[:, :, ::2]),
         "label_morph: out must be uint8 contiguous [2, 4, 6] on the labels' device"),
    ]
    for call, text in cases:
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
    # and what they hand on when nothing is refused
    values, (extents, again) = ops._organ_boxes("label_surface_distances", (vol, vol), u8(7, 7), distinct=False)
    assert values == [7, 7] and extents == again == [(0, None), (5, (0, 1, 1, 3, 0, 5))]
    assert ops._boxes_or_empty(extents) == [[0, 0, 0, 0, 0, 0], [0, 1, 1, 3, 0, 5]]
    out, in_place = ops._out_volume("label_morph", vol, None)
    assert out.shape == vol.shape and out.dtype == torch.uint8 and in_place == 0 and ops._out_volume("label_morph", vol, vol) == (vol, 1)
    ws, nb = ops._box_workspace("label_morph", [5, 9], [100, 900], 1000, 950, "cpu")
    assert nb == 950 and ws.numel() * 8 == 960 and ops._box_workspace("label_morph", [5], [100], 100, 950, "cpu")[1] == 100
