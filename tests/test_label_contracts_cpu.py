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
