"""Variant matrix of the row-wise, elementwise and conv-tail kernels (GPU): every kernel of csrc/elementwise.hip and of csrc/conv.hip outside
the patch embedding that a forward call can pick -- the vector and the scalar fallback forms, every type instantiation -- reached on purpose
through the C entries of libmsam2_hip.so and checked at its edges, in the style of tests/test_gemm_variants_gpu.py:
  * each group of launches names the kernel instantiation it must reach; torch.profiler asserts that exactly that one ran (EXPECTED lists
    them all; test_every_listed_instantiation_has_a_case compares the tables with a literal list);
  * inputs are views inside NaN-filled buffers (strided where the entry takes a stride, NaN guards on either side otherwise);
  * every output lies inside a sentinel-filled buffer (rows before and after, columns beside it where there is an ldy): the sentinels must be
    bit-identical afterwards;
  * float64 references run on the GPU from the operand-rounded inputs; arithmetic kernels lie within the derived bounds of
    tests/pointwise_bounds.py element by element (no tolerance here is taken from a kernel's output); pure data movement is bit-exact;
  * "wrap" cases are the smallest totals that force a second trip of a kernel's grid-stride loop.
The 16-bit type is ops.OP16 throughout (T16 in the kernel keys), so the bf16 build runs the file unchanged.
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointwise_bounds as PB  # noqa: E402
from helpers import (SENT16, SENT32, Canvas, Canvas2, Flat, K, kernels_launched, nan_guarded, nan_padded, op16_is_fp16, reached, same_bits,  # noqa: E402,F401
                     strided_nan, within)

DEV = "cuda"
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import medical_sam2_amd.ops as ops_mod
    return ops_mod


@pytest.fixture(scope="module")
def L(ops):
    from medical_sam2_amd import _lib
    return _lib.lib()


# ---------------------------------------------------------------------------------------------------------------------------------
def tn(bits: int) -> str:
    return "float" if bits == 32 else "T16"


def dt(ops, bits: int):
    return F32 if bits == 32 else ops.OP16


def stream():
    return torch.cuda.current_stream().cuda_stream


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def randn(*shape, seed=0):
    return torch.randn(*shape, generator=gen(seed), device=DEV)


# =================================================================================================================================
# LayerNorm
LN_C = [4, 100, 128, 132, 256, 260, 384, 388, 768, 772, 1024]          # both ends of CHUNKS 2, 4, 6, 12, 16
LN_ROWS = [1, 17, 33]
LN_TYPES = [(32, 32), (32, 16), (16, 32), (16, 16)]
LN_CHUNKS = [2, 4, 6, 12, 16]


def ln_chunks(C):
    n = (C // 4 + 15) // 16
    return next(c for c in LN_CHUNKS if n <= c)


def ln_data(ops, rows, C, ti, seed):
    """rows of different scale and offset; row 1 has mean = 1000 std (a one-pass variance loses it), the last row is constant (var = 0:
    out = bias); rounded to the input type"""
    x = randn(rows, C, seed=seed) * (0.5 + (torch.arange(rows, device=DEV) % 4).float())[:, None]
    x += 2.0 * ((torch.arange(rows, device=DEV) % 3).float() - 1)[:, None]
    if rows > 2:
        x[1] = 1000.0 + randn(C, seed=seed + 1)
    if rows > 1:
        x[rows - 1] = 2.0
    w = 1.0 + 0.5 * randn(C, seed=seed + 2)
    b = randn(C, seed=seed + 3)
    return x.to(dt(ops, ti)), w, b


class LnJob:
    def __init__(self, ops, L, ti, to, C, rows, act, *, ldx=None, x_off=0, ycanvas=None, seed=0, w_off=0, b_off=0):
        self.ops, self.L, self.to, self.act, self.C, self.rows = ops, L, to, act, C, rows
        self.what = f"layernorm {tn(ti)}->{tn(to)} C={C} rows={rows} act={act} ldx={ldx} x_off={x_off} w_off={w_off} b_off={b_off}"
        x, self.w, self.b = ln_data(ops, rows, C, ti, seed)
        if w_off:
            self.w = nan_guarded(self.w, w_off)
        if b_off:
            self.b = nan_guarded(self.b, b_off)
        self.x = strided_nan(x, ldx if ldx is not None else C + 4, x_off)
        self.cv = ycanvas if ycanvas is not None else Canvas(rows, C, dt(ops, to), aligned=True)
        self.ti = ti

    def launch(self):
        x, y = self.x, self.cv.view
        return self.L.msam2_layernorm(x.data_ptr(), int(self.ti == 16), x.stride(0), self.w.data_ptr(), self.b.data_ptr(), y.data_ptr(),
                                      int(self.to == 16), y.stride(0), self.rows, self.C, 1e-6, self.act, stream())

    def check(self):
        ref, bound = PB.layernorm_bound(self.x.double(), self.w.double(), self.b.double(), 1e-6, self.act, self.to == 16, op16_is_fp16())
        within(self.cv.view, ref, bound, self.what)
        assert self.cv.sentinels_intact(), self.what + ": wrote outside its output view"


LN_VEC_CASES = [(ti, to, ch) for ti, to in LN_TYPES for ch in LN_CHUNKS]


@pytest.mark.parametrize("ti,to,ch", LN_VEC_CASES)
def test_layernorm_vector(ops, L, ti, to, ch):
    """ldx = C + 4 inside NaN padding, aligned canvas: the vector kernel with the CHUNKS of the width"""
    jobs = [LnJob(ops, L, ti, to, C, rows, act, seed=C + rows) for C in LN_C if ln_chunks(C) == ch for rows in LN_ROWS for act in (0, 1)]
    reached(L, f"layernorm_kernel<{tn(ti)},{tn(to)},{ch}>", "layernorm_", [j.launch for j in jobs])
    for j in jobs:
        j.check()


def test_layernorm_strided_output_stays_on_the_vector_kernel(ops, L):
    """ldx = ldy = C + 4; and a 16-bit x / y that is only 8-byte aligned (the width of a four-element 16-bit access)"""
    C, rows = 128, 17
    for ti, to in LN_TYPES:
        jobs = [LnJob(ops, L, ti, to, C, rows, 0, ycanvas=Canvas2(rows, C, dt(ops, to), C + 4, 0))]
        if ti == 16:
            jobs.append(LnJob(ops, L, ti, to, C, rows, 0, x_off=4))
        if to == 16:
            jobs.append(LnJob(ops, L, ti, to, C, rows, 1, ycanvas=Canvas2(rows, C, dt(ops, to), C + 8, 4)))
        reached(L, f"layernorm_kernel<{tn(ti)},{tn(to)},2>", "layernorm_", [j.launch for j in jobs])
        for j in jobs:
            j.check()


@pytest.mark.parametrize("ti,to", LN_TYPES)
def test_layernorm_scalar_paths(ops, L, ti, to):
    """the scalar kernel, reached four ways: C % 4 != 0; ldx = C + 1; a base one element off; an fp32 y that is only 8-byte aligned (the
    vector kernel stores 16 bytes there: the host check used to pass 8-byte alignment for every output type)"""
    rows = 17
    jobs = [LnJob(ops, L, ti, to, C, rows, act, ldx=C + 3, seed=C) for C in (1, 63, 65, 1023) for act in (0, 1)]
    jobs.append(LnJob(ops, L, ti, to, 128, rows, 0, ldx=129))
    jobs.append(LnJob(ops, L, ti, to, 128, 33, 1, x_off=1))
    if to == 32:
        jobs.append(LnJob(ops, L, ti, to, 128, rows, 0, ycanvas=Canvas2(rows, 128, F32, 136, 2)))
    reached(L, f"layernorm_scalar_kernel<{tn(ti)},{tn(to)}>", "layernorm_", [j.launch for j in jobs])
    for j in jobs:
        j.check()


@pytest.mark.parametrize("ti,to", LN_TYPES)
def test_layernorm_scalar_by_one_term_each(ops, L, ti, to):
    """C = 128, rows = 17, and ONE term of msam2_layernorm's vector test false while every other holds (the terms test_layernorm_scalar_paths
    does not flip on their own): ldy % 4 != 0 under an aligned y (the view starts 3 * 130 + 2 = 392 elements into its buffer); weight, then
    bias, one float off; a 16-bit y one element off; an fp32 x that is only 8-byte aligned (the mask goes by element size on the x side too)"""
    C, rows = 128, 17
    jobs = [LnJob(ops, L, ti, to, C, rows, 1, ycanvas=Canvas2(rows, C, dt(ops, to), 130, 2), seed=1),
            LnJob(ops, L, ti, to, C, rows, 0, w_off=1, seed=2), LnJob(ops, L, ti, to, C, rows, 1, b_off=1, seed=3)]
    if to == 16:
        jobs.append(LnJob(ops, L, ti, to, C, rows, 0, ycanvas=Canvas2(rows, C, dt(ops, to), 136, 1), seed=4))
    if ti == 32:
        jobs.append(LnJob(ops, L, ti, to, C, rows, 0, x_off=2, seed=5))
    for j in jobs[:1]:
        assert j.cv.view.data_ptr() % 16 == 0 and j.cv.view.stride(0) % 4 != 0
    for j in jobs[1:3]:
        assert (j.w.data_ptr() % 16 != 0) != (j.b.data_ptr() % 16 != 0) and j.x.data_ptr() % 16 == 0 and j.cv.view.data_ptr() % 16 == 0
    reached(L, f"layernorm_scalar_kernel<{tn(ti)},{tn(to)}>", "layernorm_", [j.launch for j in jobs])
    for j in jobs:
        j.check()


@pytest.mark.parametrize("C", [4, 128, 260, 388, 772, 1024])
def test_layernorm_dual(ops, L, C):
    """y32 bit-equal to the single-output call, y16 == y32.to(OP16)"""
    rows = 17
    x, w, b = ln_data(ops, rows, C, 32, C)
    xv = strided_nan(x, C + 4)
    y32, y16, y1 = Canvas(rows, C, F32), Canvas(rows, C, ops.OP16), Canvas(rows, C, F32)
    reached(L, f"layernorm_kernel<float,float,{ln_chunks(C)}>", "layernorm_", [
        lambda: L.msam2_layernorm_dual(xv.data_ptr(), xv.stride(0), w.data_ptr(), b.data_ptr(), y32.view.data_ptr(), y32.view.stride(0),
                                       y16.view.data_ptr(), y16.view.stride(0), rows, C, 1e-6, stream()),
        lambda: L.msam2_layernorm(xv.data_ptr(), 0, xv.stride(0), w.data_ptr(), b.data_ptr(), y1.view.data_ptr(), 0, y1.view.stride(0), rows, C,
                                  1e-6, 0, stream())])
    ref, bound = PB.layernorm_bound(xv.double(), w.double(), b.double(), 1e-6)
    within(y32.view, ref, bound, f"layernorm_dual C={C}")
    same_bits(y32.view, y1.view, "layernorm_dual fp32 rows against msam2_layernorm")
    same_bits(y16.view, y32.view.to(ops.OP16), "layernorm_dual 16-bit rows against the rounded fp32 rows")
    assert y32.sentinels_intact() and y16.sentinels_intact() and y1.sentinels_intact()


# =================================================================================================================================
# add_cast
AC_TYPES = [(a, b, o) for a in (32, 16) for b in (32, 16) for o in (32, 16)]


def ac_launch(L, a, b, alpha, out, D0, D1, C, ops):
    return L.msam2_add_cast(a.data_ptr(), int(a.dtype == ops.OP16), a.stride(0), a.stride(1), b.data_ptr() if b is not None else None,
                            int(b is not None and b.dtype == ops.OP16), b.stride(0) if b is not None else 0, b.stride(1) if b is not None else 0,
                            alpha, out.data_ptr(), int(out.dtype == ops.OP16), D0, D1, C, stream())


def ac_jobs(ops, ta, tb, to, C, *, a_layout, a_off=0, seed=0):
    """one job per b layout: full, broadcast over dim 0, over dim 1, over both, absent (only in the tb = fp32 instantiation, which a null b
    selects).  a_layout 'T': a is the transpose of a [D1, D0, Cp] buffer (Cp = 8); 'pad5': rows of stride 5 (C = 4: a_s1 % 4 != 0);
    'plain': contiguous.  a_off moves a's base by that many elements."""
    D0, D1 = 3, 5
    jobs = []
    for bl, alpha in (("full", 0.75), ("b0", -2.5), ("b1", 1.0), ("b01", 0.75), ("none", 1.0)):
        if bl == "none" and tb != 32:
            continue
        src = randn(D0, D1, C, seed=seed).to(dt(ops, ta))
        if a_layout == "T":
            buf = torch.full((a_off + D1 * D0 * 8 + 8,), float("nan"), dtype=src.dtype, device=DEV)
            a = torch.as_strided(buf, (D0, D1, C), (8, D0 * 8, 1), a_off)
        elif a_layout == "pad5":
            buf = torch.full((a_off + D0 * D1 * 5 + 8,), float("nan"), dtype=src.dtype, device=DEV)
            a = torch.as_strided(buf, (D0, D1, C), (D1 * 5, 5, 1), a_off)
        else:
            buf = torch.full((a_off + D0 * D1 * C + 8,), float("nan"), dtype=src.dtype, device=DEV)
            a = torch.as_strided(buf, (D0, D1, C), (D1 * C, C, 1), a_off)
        a.copy_(src)
        b = None
        if bl != "none":
            shape = {"full": (D0, D1, C), "b0": (1, D1, C), "b1": (D0, 1, C), "b01": (1, 1, C)}[bl]
            b = nan_guarded(randn(*shape, seed=seed + 7).to(dt(ops, tb))).expand(D0, D1, C)
        out = Flat((D0, D1, C), dt(ops, to))
        jobs.append((a, b, alpha, out, f"add_cast {tn(ta)},{tn(tb)}->{tn(to)} C={C} a={a_layout}+{a_off} b={bl}"))
    return jobs


def ac_check(ops, jobs):
    for a, b, alpha, out, what in jobs:
        ref, bound = PB.add_cast_bound(a.double(), b.double() if b is not None else None, alpha, out.view.dtype == ops.OP16, op16_is_fp16())
        within(out.view, ref, bound, what)
        if b is None:                                          # cast only: bit-exact
            same_bits(out.view, a.to(out.view.dtype), what + " (cast only)")
        assert out.sentinels_intact(), what + ": wrote outside its output"


@pytest.mark.parametrize("ta,tb,to", AC_TYPES)
def test_add_cast_vector(ops, L, ta, tb, to):
    jobs = ac_jobs(ops, ta, tb, to, 4, a_layout="T")
    reached(L, f"add_cast_vec_kernel<{tn(ta)},{tn(tb)},{tn(to)}>", "add_cast_", [lambda j=j: ac_launch(L, j[0], j[1], j[2], j[3].view, 3, 5, 4, ops) for j in jobs])
    ac_check(ops, jobs)


@pytest.mark.parametrize("ta,tb,to", AC_TYPES)
def test_add_cast_scalar(ops, L, ta, tb, to):
    """C in {1, 6}; C = 4 with a base 1..3 elements off; C = 4 with a_s1 % 4 != 0"""
    groups = [(1, ac_jobs(ops, ta, tb, to, 1, a_layout="T", seed=1)), (6, ac_jobs(ops, ta, tb, to, 6, a_layout="T", seed=2)),
              (4, ac_jobs(ops, ta, tb, to, 4, a_layout="pad5", seed=3))]
    groups += [(4, ac_jobs(ops, ta, tb, to, 4, a_layout="plain", a_off=o, seed=3 + o)) for o in (1, 2, 3)]
    launches = [lambda j=j, C=C: ac_launch(L, j[0], j[1], j[2], j[3].view, 3, 5, C, ops) for C, jobs in groups for j in jobs]
    reached(L, f"add_cast_kernel<{tn(ta)},{tn(tb)},{tn(to)}>", "add_cast_", launches)
    for _, jobs in groups:
        ac_check(ops, jobs)


def ac_strided(src, s0, s1, off):
    """src [D0, D1, C] as a view with element strides (s0, s1, 1) inside a NaN-filled buffer, `off` elements into it"""
    D0, D1, C = src.shape
    buf = torch.full((off + D0 * s0 + D1 * s1 + C + 8,), float("nan"), dtype=src.dtype, device=DEV)
    v = torch.as_strided(buf, (D0, D1, C), (s0, s1, 1), off)
    v.copy_(src)
    return v


@pytest.mark.parametrize("ta,tb,to", AC_TYPES)
def test_add_cast_scalar_by_one_term_each(ops, L, ta, tb, to):
    """a [2, 3, 8] volume with strides (24, 8), and ONE term of msam2_add_cast's vector test false while every other holds (the terms
    test_add_cast_scalar does not flip on their own: its 'pad5' layout breaks a_s0 and a_s1 together, b and out are always aligned):
    a_s0 = 26; a_s1 = 9; out one element off; b_s0 = 26; b_s1 = 9; b one element off.  (total / 4 < 2^31 needs 2^33 elements: not flipped.)"""
    D0, D1, C = 2, 3, 8
    cases = [("a_s0", (26, 8, 0), (24, 8, 0), 0), ("a_s1", (28, 9, 0), (24, 8, 0), 0), ("out", (24, 8, 0), (24, 8, 0), 1),
             ("b_s0", (24, 8, 0), (26, 8, 0), 0), ("b_s1", (24, 8, 0), (28, 9, 0), 0), ("b", (24, 8, 0), (24, 8, 1), 0)]
    jobs = []
    for i, (term, sa, sb, out_off) in enumerate(cases):
        a = ac_strided(randn(D0, D1, C, seed=20 + i).to(dt(ops, ta)), *sa)
        b = ac_strided(randn(D0, D1, C, seed=40 + i).to(dt(ops, tb)), *sb)
        jobs.append((a, b, 0.75, Flat((D0, D1, C), dt(ops, to), offset=out_off), f"add_cast {tn(ta)},{tn(tb)}->{tn(to)} only {term} off"))
    reached(L, f"add_cast_kernel<{tn(ta)},{tn(tb)},{tn(to)}>", "add_cast_", [lambda j=j: ac_launch(L, j[0], j[1], j[2], j[3].view, D0, D1, C, ops) for j in jobs])
    ac_check(ops, jobs)


@pytest.mark.parametrize("key,shape", [("add_cast_kernel<float,float,float>", (2, 1025, 1026)), ("add_cast_vec_kernel<float,float,float>", (4, 1025, 4100))])
def test_add_cast_grid_stride_wraps(ops, L, key, shape):
    """more elements (groups of four) than the capped grid has threads; alpha = 1, so a + b is one fp32 addition: bit-exact"""
    D0, D1, C = shape
    assert (D0 * D1 * C) // (4 if "vec" in key else 1) > (16384 if "vec" in key else 8192) * 256
    a, b = nan_guarded(randn(*shape, seed=1)), nan_guarded(randn(1, D1, C, seed=2)).expand(*shape)
    out = Flat(shape, F32)
    reached(L, key, "add_cast_", [lambda: ac_launch(L, a, b, 1.0, out.view, D0, D1, C, ops)])
    same_bits(out.view, a + b, "add_cast wrap")
    assert out.sentinels_intact()


# =================================================================================================================================
# maxpool2x2
def pool_ref(x, B, H, W):
    C = x.shape[1]
    return x.reshape(B, H // 2, 2, W // 2, 2, C).amax((2, 4)).reshape(-1, C)


def mp_launch(L, ops, x, y, B, H, W):
    return L.msam2_maxpool2x2(x.data_ptr(), int(x.dtype == ops.OP16), x.stride(0), y.data_ptr(), int(y.dtype == ops.OP16), y.stride(0), B, H, W,
                              x.shape[1], stream())


@pytest.mark.parametrize("ti,to", LN_TYPES)
def test_maxpool(ops, L, ti, to):
    """bit-exact; B = 3 with H != W so that a batch or row mix-up shows; strided input inside NaN padding, strided output in a canvas"""
    B, H, W, C = 3, 4, 6, 5
    x = nan_padded(B * H * W, C, C + 3, dt(ops, ti), randn(B * H * W, C, seed=3))
    cv = Canvas(B * (H // 2) * (W // 2), C, dt(ops, to), aligned=False)
    reached(L, f"maxpool2x2_kernel<{tn(ti)},{tn(to)}>", "maxpool2x2_", [lambda: mp_launch(L, ops, x, cv.view, B, H, W)])
    same_bits(cv.view, pool_ref(x, B, H, W).to(dt(ops, to)), f"maxpool {tn(ti)}->{tn(to)}")
    assert cv.sentinels_intact()


def test_maxpool_saturates(ops, L):
    """fp32 -> 16 bits with inputs beyond +-65504: the fp16 build stores +-65504, never inf (csrc/common.h; the kernel used a plain
    conversion: inf).  bf16 has nothing to saturate: the plain rounding."""
    B, H, W, C = 1, 2, 4, 3
    x = randn(B * H * W, C, seed=5) * 10
    x[0], x[2] = 1.0e5, -1.0e5
    x[3], x[6], x[7] = -2.0e5, -3.0e5, -1.5e5                  # the 2x2 window (pixels 2, 3, 6, 7) has only values below -65504
    cv = Canvas(2, C, ops.OP16, aligned=False)
    reached(L, "maxpool2x2_kernel<float,T16>", "maxpool2x2_", [lambda: mp_launch(L, ops, x, cv.view, B, H, W)])
    ref = pool_ref(x, B, H, W)
    if op16_is_fp16():
        assert bool(torch.isfinite(cv.view).all()), "maxpool2x2 stored inf in fp16"
        ref = ref.clamp(-65504.0, 65504.0)
    same_bits(cv.view, ref.to(ops.OP16), "maxpool saturation")
    assert cv.sentinels_intact()


def test_maxpool_grid_stride_wraps(ops, L):
    B, H, W, C = 1, 1024, 1026, 8
    assert B * (H // 2) * (W // 2) * C > 8192 * 256
    x = nan_guarded(randn(B * H * W, C, seed=6))
    out = Flat((B * (H // 2) * (W // 2), C), F32)
    reached(L, "maxpool2x2_kernel<float,float>", "maxpool2x2_", [lambda: mp_launch(L, ops, x, out.view, B, H, W)])
    same_bits(out.view, pool_ref(x, B, H, W), "maxpool wrap")
    assert out.sentinels_intact()


# =================================================================================================================================
# upsample2x_add_ (in place, fp32): the single fp32 addition is bit-exact
def up_ref(y, top, B, H, W):
    C = y.shape[-1]
    t = top.view(B, H // 2, W // 2, C).repeat_interleave(2, 1).repeat_interleave(2, 2)
    return y.view(B, H, W, C) + t


UP_CASES = [("upsample2x_add_kernel", 2, 4, 6, 3, 0), ("upsample2x_add4_kernel", 2, 4, 6, 4, 0), ("upsample2x_add4_kernel", 2, 4, 6, 48, 0),
            ("upsample2x_add_kernel", 2, 4, 6, 4, 1),                                    # C % 4 == 0 but y one element off its alignment
            ("upsample2x_add_kernel", 1, 838, 836, 3, 0), ("upsample2x_add4_kernel", 1, 1024, 1026, 16, 0)]      # wraps


@pytest.mark.parametrize("key,B,H,W,C,off", UP_CASES)
def test_upsample2x_add(ops, L, key, B, H, W, C, off):
    if H > 100:
        assert B * H * W * C // (4 if "4" in key else 1) > (16384 if "4" in key else 8192) * 256
    y0, top = randn(B, H, W, C, seed=1), nan_guarded(randn(B, H // 2, W // 2, C, seed=2))
    out = Flat((B, H, W, C), F32, offset=off)
    out.view.copy_(y0)
    reached(L, key, "upsample2x_add", [lambda: L.msam2_upsample2x_add(out.view.data_ptr(), top.data_ptr(), B, H, W, C, stream())])
    same_bits(out.view, up_ref(y0, top, B, H, W), f"upsample2x_add {B}x{H}x{W}x{C}")
    assert out.sentinels_intact()


def test_upsample2x_add_top_misaligned(ops, L):
    """C % 4 == 0 and an aligned y, but top one float off its alignment: the one-element kernel (UP_CASES moves only y)"""
    B, H, W, C = 2, 4, 6, 4
    y0, top = randn(B, H, W, C, seed=1), nan_guarded(randn(B, H // 2, W // 2, C, seed=2), 1)
    out = Flat((B, H, W, C), F32)
    out.view.copy_(y0)
    assert out.view.data_ptr() % 16 == 0 and top.data_ptr() % 16 == 4
    reached(L, "upsample2x_add_kernel", "upsample2x_add", [lambda: L.msam2_upsample2x_add(out.view.data_ptr(), top.data_ptr(), B, H, W, C, stream())])
    same_bits(out.view, up_ref(y0, top, B, H, W), "upsample2x_add with top off its alignment")
    assert out.sentinels_intact()


# =================================================================================================================================
# rope_
def rope_launch(L, x, n_rope, cs, sn):
    B, Lr, D = x.shape
    return L.msam2_rope_inplace(x.data_ptr(), x.stride(0), x.stride(1), B, Lr, n_rope, cs.shape[0], D, cs.data_ptr(), sn.data_ptr(), stream())


def rope_check(ops, before, after, view_of, n_rope, cs, sn, what):
    """before / after: the whole buffer; view_of(buffer) -> the [B, L, D] view that was rotated"""
    x0, x1 = view_of(before), view_of(after)
    B, Lr, D = x0.shape
    n_pos = cs.shape[0]
    if n_rope:
        pos = torch.arange(n_rope, device=DEV) % n_pos
        c, s = cs[pos].double()[None], sn[pos].double()[None]
        re, im = x0[:, :n_rope, 0::2].double(), x0[:, :n_rope, 1::2].double()
        rr, ri, br, bi = PB.rope_bound(re, im, c, s, op16_is_fp16())
        within(x1[:, :n_rope, 0::2], rr, br, what + " (re)")
        within(x1[:, :n_rope, 1::2], ri, bi, what + " (im)")
    untouched = torch.ones(before.shape, dtype=torch.bool, device=DEV)
    view_of(untouched)[:, :n_rope] = False
    same_bits(after[untouched], before[untouched], what + ": rows past n_rope and the neighbouring columns")


@pytest.mark.parametrize("n_rope", [0, 1, 10])
def test_rope_strided_view(ops, L, n_rope):
    """the middle third of a [B, L, 3 D] buffer; L = 10 > n_pos = 4: the table tiles"""
    B, Lr, D = 2, 10, 8
    cs, sn = ops.rope_table(2, D, 10000.0, DEV)
    buf = randn(B, Lr, 3 * D, seed=n_rope).to(ops.OP16)
    before = buf.clone()
    view_of = lambda t: t[:, :, D:2 * D]
    reached(L, "rope_inplace_kernel" if n_rope else None, "rope_inplace", [lambda: rope_launch(L, view_of(buf), n_rope, cs, sn)])
    rope_check(ops, before, buf, view_of, n_rope, cs, sn, f"rope n_rope={n_rope}")


def test_rope_saturates(ops, L):
    """an already saturated q / k pair (60000, 60000) rotated by 45 degrees is (0, 84853): the fp16 build stores 65504, never inf (the
    kernel used a plain conversion: inf, which reached the softmax)"""
    D = 4
    x = torch.full((1, 1, D), 60000.0, device=DEV).to(ops.OP16)
    before = x.clone()
    cs = torch.full((1, D // 2), math.sqrt(0.5), device=DEV)
    sn = cs.clone()
    reached(L, "rope_inplace_kernel", "rope_inplace", [lambda: rope_launch(L, x, 1, cs, sn)])
    if op16_is_fp16():
        assert bool(torch.isfinite(x).all()), "rope stored inf in fp16"
        re, im = before[0, 0, 0::2].double(), before[0, 0, 1::2].double()
        rr, ri, br, _ = PB.rope_bound(re, im, cs[0].double(), sn[0].double())
        assert float(ri.min()) > 65504.0
        same_bits(x[0, 0, 1::2], torch.full((D // 2,), 65504.0, device=DEV).to(ops.OP16), "rope saturation")
        within(x[0, 0, 0::2], rr, br, "rope saturation (re)")
    else:
        rope_check(ops, before, x, lambda t: t, 1, cs, sn, "rope at 60000 (bf16)")


def test_rope_grid_stride_wraps(ops, L):
    B, n_rope, D = 2, 8200, 256
    assert B * n_rope * (D // 2) > 8192 * 256
    cs, sn = ops.rope_table(64, D, 10000.0, DEV)               # 4096 positions: rows 4096.. reuse the table
    x = randn(B, n_rope + 3, D, seed=4).to(ops.OP16)
    before = x.clone()
    reached(L, "rope_inplace_kernel", "rope_inplace", [lambda: rope_launch(L, x, n_rope, cs, sn)])
    rope_check(ops, before, x, lambda t: t, n_rope, cs, sn, "rope wrap")


# =================================================================================================================================
# bilinear_upsample
def bil_launch(L, x, y, H, W):
    P, h, w = x.shape
    return L.msam2_bilinear_upsample(x.data_ptr(), y.data_ptr(), P, h, w, H, W, stream())


BIL_CASES = [("bilinear_kernel", 3, 16, 24, 50, 97), ("bilinear_kernel", 2, 7, 5, 7, 5), ("bilinear4_kernel", 2, 32, 32, 12, 20),
             ("bilinear_kernel", 2, 5, 6, 11, 18), ("bilinear4_kernel", 2, 8, 8, 16, 32), ("bilinear4_kernel", 1, 1, 1, 3, 4),
             ("bilinear_kernel", 1, 64, 64, 2049, 2050), ("bilinear4_kernel", 4, 64, 48, 2048, 2052)]            # wraps


@pytest.mark.parametrize("key,P,h,w,H,W", BIL_CASES)
def test_bilinear(ops, L, key, P, h, w, H, W):
    if H > 1000:
        assert P * H * W // (4 if "4" in key else 1) > 16384 * 256
    x = nan_guarded(randn(P, h, w, seed=h + w))
    out = Flat((P, H, W), F32)
    reached(L, key, "bilinear", [lambda: bil_launch(L, x, out.view, H, W)])
    ref, bound = PB.bilinear_bound(x.double(), H, W)
    within(out.view, ref, bound, f"bilinear {h}x{w} -> {H}x{W}")
    if (h, w) == (H, W):
        same_bits(out.view, x, "bilinear identity")
    assert out.sentinels_intact()


def test_bilinear_vector_and_scalar_forms_agree(ops, L):
    """W % 4 == 0: the four-pixel kernel, and the one-pixel kernel forced by a y one element off its alignment, give the same bits"""
    P, h, w, H, W = 2, 16, 24, 50, 96
    x = nan_guarded(randn(P, h, w, seed=9))
    a, b = Flat((P, H, W), F32), Flat((P, H, W), F32, offset=1)
    reached(L, "bilinear4_kernel", "bilinear", [lambda: bil_launch(L, x, a.view, H, W)])
    reached(L, "bilinear_kernel", "bilinear", [lambda: bil_launch(L, x, b.view, H, W)])
    same_bits(a.view, b.view, "bilinear4 against bilinear")
    assert a.sentinels_intact() and b.sentinels_intact()


# =================================================================================================================================
# aa_downsample: reference F.interpolate(x.double() * s + b, mode="bilinear", antialias=True) (evaluated on the host, where float64 is
# implemented for the anti-aliased filter everywhere; the bound's sum |w v| is evaluated on the GPU)
AA_CASES = [(2, 8, 12, 1, 1.0, 0.0), (2, 8, 12, 2, 20.0, -10.0), (3, 16, 8, 4, 20.0, -10.0), (1, 4, 4, 4, 1.0, 0.0), (2, 6, 10, 2, 1.0, 0.0),
            (1, 2900, 2900, 2, 20.0, -10.0)]                                                                    # wrap


@pytest.mark.parametrize("P,H,W,f,s,b", AA_CASES)
def test_aa_downsample(ops, L, P, H, W, f, s, b):
    if H > 1000:
        assert P * (H // f) * (W // f) > 8192 * 256
    x = nan_guarded(randn(P, H, W, seed=H + f))
    out = Flat((P, H // f, W // f), F32)
    reached(L, "aa_downsample_kernel", "aa_downsample", [lambda: L.msam2_aa_downsample(x.data_ptr(), out.view.data_ptr(), P, H, W, f, s, b, stream())])
    ref = F.interpolate((x.double().cpu() * s + b)[None], size=(H // f, W // f), mode="bilinear", antialias=True, align_corners=False)[0].to(DEV)
    ref2, bound = PB.aa_downsample_bound(x.double(), f, s, b)
    assert float((ref - ref2).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), "the restated filter differs from F.interpolate"
    within(out.view, ref, bound, f"aa_downsample {H}x{W} / {f}")
    assert out.sentinels_intact()


# =================================================================================================================================
# image_prep
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@pytest.mark.parametrize("S,H,W", [(64, 64, 64), (64, 37, 53), (64, 128, 192), (840, 840, 840), (840, 37, 53), (840, 1680, 2520)])
def test_image_prep(ops, L, S, H, W):
    """S = 840 is the wrap case.  H x W = S x S is the identity: bit-equal to (img / 255 - mean) / std in fp32 (the kernel multiplied by
    1.0f / 255.0f, which differs from the division in the last bit for 126 of the 256 pixel values)"""
    if S == 840:
        assert 3 * S * S > 8192 * 256
    img = nan_guarded(torch.randint(0, 256, (H, W, 3), generator=gen(S + H), device=DEV).to(torch.uint8))
    out = Flat((3, S, S), F32)
    m, s = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
    reached(L, "image_prep_kernel", "image_prep", [lambda: L.msam2_image_prep(img.data_ptr(), out.view.data_ptr(), H, W, S, m, s, stream())])
    m32 = torch.tensor(list(m), device=DEV).view(3, 1, 1)
    s32 = torch.tensor(list(s), device=DEV).view(3, 1, 1)
    chw = img.permute(2, 0, 1)
    if (H, W) == (S, S):
        host = (chw.cpu().float() / 255.0 - m32.cpu()) / s32.cpu()            # IEEE fp32 divisions
        same_bits(out.view, host.to(DEV), "image_prep identity")
    px = chw.double() / 255.0
    v, bv = PB.bilinear_bound(px, S, S, pixel_err=PB.U)
    ref = (v - m32.double()) / s32.double()
    within(out.view, ref, (bv + PB.U * (v - m32.double()).abs()) / s32.double() + PB.U * ref.abs(), f"image_prep {H}x{W} -> {S}")
    assert out.sentinels_intact()


# =================================================================================================================================
# space_to_depth / im2col3x3s2: bit-exact gathers with zero fill
def s2d_ref(x, B, H, W, C, k, ld, odt):
    p = x.view(B, H // k, k, W // k, k, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, k * k * C).to(odt)
    return F.pad(p, (0, ld - k * k * C))


S2D_CASES = [(ti, k, C, 8, 12) for ti in (32, 16) for k, C in ((4, 1), (2, 1), (2, 4), (2, 3))] + [(32, 4, 1, 2048, 2048)]     # the last one wraps


@pytest.mark.parametrize("ti,k,C,H,W", S2D_CASES)
def test_space_to_depth(ops, L, ti, k, C, H, W):
    """(k, C) = (2, 3): ld = 16 > 12, the zero fill"""
    B = 1 if H > 1000 else 2
    ld = (k * k * C + 7) // 8 * 8
    if H > 1000:
        assert B * (H // k) * (W // k) * ld > 8192 * 256
    x = nan_guarded(randn(B * H * W, C, seed=k + C).to(dt(ops, ti)))
    out = Flat((B * (H // k) * (W // k), ld), ops.OP16)
    reached(L, f"space_to_depth_kernel<{tn(ti)}>", "space_to_depth", [
        lambda: L.msam2_space_to_depth(x.data_ptr(), int(ti == 16), out.view.data_ptr(), B, H, W, C, k, ld, stream())])
    same_bits(out.view, s2d_ref(x, B, H, W, C, k, ld, ops.OP16), f"space_to_depth k={k} C={C}")
    assert out.sentinels_intact()


def im2col_ref(x, B, H, W, C, ld):
    p = F.pad(x.view(B, H, W, C), (0, 0, 1, 1, 1, 1))
    cols = [p[:, ky:ky + H:2, kx:kx + W:2] for ky in range(3) for kx in range(3)]
    return F.pad(torch.cat(cols, -1).reshape(-1, 9 * C), (0, ld - 9 * C))


@pytest.mark.parametrize("C,B,H,W", [(C, 2, H, W) for C in (4, 12, 64) for H, W in ((2, 2), (6, 10), (16, 16))] + [(64, 1, 512, 512)])
def test_im2col3x3s2(ops, L, C, B, H, W):
    """C = 4: ld = 40 against 9 C = 36 (the zero-fill group and the tap clamp); 512 x 512 x 64 is the wrap case"""
    ld = (9 * C + 7) // 8 * 8
    if H > 100:
        assert B * (H // 2) * (W // 2) * (ld // 4) > 16384 * 256
    x = nan_guarded(randn(B * H * W, C, seed=C + H).to(ops.OP16))
    out = Flat((B * (H // 2) * (W // 2), ld), ops.OP16)
    reached(L, "im2col3x3s2_kernel", "im2col3x3s2", [lambda: L.msam2_im2col3x3s2(x.data_ptr(), out.view.data_ptr(), B, H, W, C, ld, stream())])
    same_bits(out.view, im2col_ref(x, B, H, W, C, ld), f"im2col3x3s2 C={C} {H}x{W}")
    assert out.sentinels_intact()


# =================================================================================================================================
# gate_rows / any_positive / gather_rows / obj_ptr_mix / non_overlap: selections and fills, bit-exact
OBJ = [0.0, -0.0, float("nan"), 1e-30, 3.0]                 # only the last two are "> 0"


@pytest.mark.parametrize("row_len", [1, 257, 513 * 512])
def test_gate_rows(ops, L, row_len):
    """rows whose score is not > 0 (0.0, -0.0, NaN) are filled; 513 * 512 elements wrap the 1024-block grid"""
    if row_len > 1000:
        assert row_len > 1024 * 256
    B = len(OBJ)
    x0, score = randn(B, row_len, seed=row_len), nan_guarded(torch.tensor(OBJ, device=DEV))
    out = Flat((B, row_len), F32)
    out.view.copy_(x0)
    reached(L, "gate_rows_kernel", "gate_rows", [lambda: L.msam2_gate_rows(out.view.data_ptr(), score.data_ptr(), -1024.0, B, row_len, stream())])
    same_bits(out.view, torch.where((score > 0)[:, None], x0, torch.full_like(x0, -1024.0)), f"gate_rows row_len={row_len}")
    assert out.sentinels_intact()


@pytest.mark.parametrize("row_len", [1, 1023, 1025, 70000])
def test_any_positive(ops, L, row_len):
    """the only positive value first, last, in the middle, absent; rows of -0.0 and of NaN give 0"""
    x = -randn(7, row_len, seed=row_len).abs()
    x[0, 0], x[1, row_len - 1], x[2, row_len // 2] = 1e-30, 1e-30, 5.0
    x[4], x[5], x[6] = -0.0, float("nan"), 0.0
    x = nan_guarded(x)
    out = Flat((7,), F32)
    reached(L, "any_positive_kernel", "any_positive", [lambda: L.msam2_any_positive(x.data_ptr(), out.view.data_ptr(), 7, row_len, stream())])
    same_bits(out.view, torch.tensor([1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0], device=DEV), f"any_positive row_len={row_len}")
    assert out.sentinels_intact()


@pytest.mark.parametrize("C", [1, 257])
def test_gather_rows_and_obj_ptr_mix(ops, L, C):
    n, T = 5, 4
    x = nan_guarded(randn(n, T, C, seed=C))
    sel = nan_guarded(torch.tensor([3, 0, 2, 1, 0], dtype=torch.int32, device=DEV))
    a, b = Flat((n, C), F32), Flat((n, C), F32)
    reached(L, "gather_rows_kernel", "gather_rows", [
        lambda: L.msam2_gather_rows(x.data_ptr(), sel.data_ptr(), a.view.data_ptr(), n, T, C, 0, stream()),
        lambda: L.msam2_gather_rows(x.data_ptr(), None, b.view.data_ptr(), n, T, C, 2, stream())])
    same_bits(a.view, x[torch.arange(n, device=DEV), sel.long()], f"gather_rows C={C}")
    same_bits(b.view, x[:, 2], f"gather_rows sel=None offset=2 C={C}")
    assert a.sentinels_intact() and b.sentinels_intact()
    obj, nop = nan_guarded(torch.tensor(OBJ, device=DEV)), nan_guarded(randn(C, seed=C + 1))
    p0 = randn(n, C, seed=C + 2)
    ptr = Flat((n, C), F32)
    ptr.view.copy_(p0)
    reached(L, "obj_ptr_mix_kernel", "obj_ptr_mix", [lambda: L.msam2_obj_ptr_mix(ptr.view.data_ptr(), obj.data_ptr(), nop.data_ptr(), n, C, stream())])
    same_bits(ptr.view, torch.where((obj > 0)[:, None], p0, nop[None].expand(n, C)), f"obj_ptr_mix C={C}")
    assert ptr.sentinels_intact()


def non_overlap_ref(x):
    n = x.shape[0]
    idx = torch.arange(n, device=x.device)[:, None]
    best = torch.where(x == x.max(0, keepdim=True).values, idx, n).min(0, keepdim=True).values       # the first maximum
    return torch.where(idx == best, x, x.clamp(max=-10.0))


@pytest.mark.parametrize("n,P", [(1, 255), (2, 255), (5, 255), (2, 1450 * 1450)])
def test_non_overlap(ops, L, n, P):
    """integer-valued scores tie often (the first maximum wins); losing scores lie on both sides of -10; 1450^2 pixels wrap the grid"""
    if P > 1000:
        assert P > 8192 * 256
    x = (randn(n, P, seed=n) * 8).round()
    x[:, 1::2] += 0.25 * randn(n, P, seed=n + 1)[:, 1::2]
    x = nan_guarded(x)
    out = Flat((n, P), F32)
    reached(L, "non_overlap_kernel", "non_overlap", [lambda: L.msam2_non_overlap(x.data_ptr(), out.view.data_ptr(), n, P, stream())])
    same_bits(out.view, non_overlap_ref(x), f"non_overlap n={n} P={P}")
    assert out.sentinels_intact()


# =================================================================================================================================
# select_mask
DELTA, THRESH = float(np.float32(0.05)), float(np.float32(0.98))


def select_ref(masks, ious, obj, multimask, dynamic):
    """the rule of csrc/conv.hip restated on the host: counts are integers, the stability score is one fp32 division"""
    n, _, P = masks.shape
    m, io, ob = masks.cpu().numpy(), ious.cpu().numpy(), obj.cpu().numpy()
    low, sel, iou_sel = np.empty((n, P), np.float32), np.empty(n, np.int32), np.empty(n, np.float32)
    for b in range(n):
        best = 1 + int(np.argmax(io[b, 1:]))                  # numpy: the first maximum
        choice = best
        if not multimask:
            choice = 0
            if dynamic:
                ti, tu = int((m[b, 0] > np.float32(DELTA)).sum()), int((m[b, 0] > -np.float32(DELTA)).sum())
                stab = np.float32(ti) / np.float32(tu) if tu > 0 else np.float32(1.0)
                if not stab >= np.float32(THRESH):
                    choice = best
        sel[b], iou_sel[b] = choice, io[b, choice]
        low[b] = m[b, choice] if ob[b] > 0 else np.float32(-1024.0)
    return torch.from_numpy(low).to(DEV), torch.from_numpy(sel).to(DEV), torch.from_numpy(iou_sel).to(DEV)


@pytest.mark.parametrize("P", [4, 256, 9216])
def test_select_mask(ops, L, P):
    """P = 9216: the second trip of the stability loop, whose empty slots are -inf.  Images: 0 stable; 1 unstable (dynamic fallback to the best
    of 1..3, IoU tie: the first wins); 2 stability exactly == thresh (49 / 50, token 0 stays; P >= 256); 3 no pixel above -delta (tu == 0:
    token 0 stays); 4 values exactly +-delta (counted by neither comparison); 5-8 the object scores 0.0, -0.0, tiny, NaN"""
    n = 9
    masks = randn(n, 4, P, seed=P) * 4 + torch.sign(randn(n, 4, P, seed=P + 1))         # |v| > delta almost surely
    masks[0, 0] = masks[0, 0].abs() + 1.0
    masks[1, 0] = masks[1, 0] * 0.001
    if P >= 256:
        masks[2, 0] = -5.0
        masks[2, 0, P - 49:] = 5.0
        masks[2, 0, 0] = 0.0                                   # 49 above delta, 50 above -delta
    masks[3, 0] = -masks[3, 0].abs() - 1.0
    masks[4, 0, 0::2], masks[4, 0, 1::2] = DELTA, -DELTA        # ti = 0, tu = P / 2: stability 0
    ious = torch.rand(n, 4, generator=gen(P + 2), device=DEV)
    ious[1, 1:] = torch.tensor([0.25, 0.75, 0.75], device=DEV)
    ious[4, 1:] = torch.tensor([0.5, 0.5, 0.5], device=DEV)
    obj = torch.tensor([1.0, 2.0, 1.0, 1.0, 1.0, 0.0, -0.0, 1e-30, float("nan")], device=DEV)
    masks, ious, obj = nan_guarded(masks), nan_guarded(ious), nan_guarded(obj)
    for multimask, dynamic in ((1, 1), (0, 1), (0, 0)):
        low, sel, iou_sel = Flat((n, P), F32), Flat((n,), torch.int32), Flat((n,), F32)
        reached(L, "select_mask_kernel", "select_mask", [
            lambda: L.msam2_select_mask(masks.data_ptr(), ious.data_ptr(), obj.data_ptr(), low.view.data_ptr(), sel.view.data_ptr(),
                                        iou_sel.view.data_ptr(), n, P, multimask, dynamic, DELTA, THRESH, stream())])
        rl, rs, ri = select_ref(masks, ious, obj, multimask, dynamic)
        what = f"select_mask P={P} multimask={multimask} dynamic={dynamic}"
        same_bits(sel.view, rs, what + ": sel")
        same_bits(iou_sel.view, ri, what + ": iou_sel")
        same_bits(low.view, rl, what + ": low_res")
        if not multimask and dynamic:
            assert rs.tolist()[:5] == [0, 2, 0 if P >= 256 else int(rs[2]), 0, 1], rs.tolist()
        assert low.sentinels_intact() and sel.sentinels_intact() and iou_sel.sentinels_intact()


# =================================================================================================================================
# hyper_masks
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("K_", [1, 4, 8])
def test_hyper_masks(ops, L, K_, n):
    C = 32
    for P in (1, 255, 257, 4096):
        for exact in (True, False):
            if exact:                                          # small integers: every partial sum is an integer < 2^24, exact in any order
                hyper = torch.randint(-3, 4, (n, K_, C), generator=gen(P), device=DEV).float()
                up = torch.randint(-4, 5, (n, P, C), generator=gen(P + 1), device=DEV).to(ops.OP16)
            else:
                hyper, up = randn(n, K_, C, seed=P + 2), randn(n, P, C, seed=P + 3).to(ops.OP16)
            hyper, up = nan_guarded(hyper), nan_guarded(up)
            out = Flat((n, K_, P), F32)
            reached(L, "hyper_masks_kernel", "hyper_masks", [
                lambda: L.msam2_hyper_masks(hyper.data_ptr(), up.data_ptr(), out.view.data_ptr(), n, K_, P, C, stream())])
            ref, bound = PB.hyper_masks_bound(hyper.double(), up.double())
            if exact:
                same_bits(out.view, ref.float(), f"hyper_masks integers K={K_} P={P} n={n}")
            else:
                within(out.view, ref, bound, f"hyper_masks K={K_} P={P} n={n}")
            assert out.sentinels_intact()


# =================================================================================================================================
# prompt_points
@pytest.mark.parametrize("C", [6, 256])
@pytest.mark.parametrize("n_pad", [0, 1, 2])
def test_prompt_points(ops, L, C, n_pad):
    """labels -1 .. 3, the out-of-range labels 4 and -2 (pure positional encoding), coordinates 0, S - 1, negative and beyond S"""
    S, nf = 1024.0, C // 2
    xy = torch.tensor([[[0.0, 0.0], [S - 1, S - 1], [-7.5, 100.25], [S + 300.0, 511.0], [12.0, 900.5], [333.0, 4.0], [64.0, 64.0]],
                       [[5.0, 6.0], [700.0, 3.0], [1.0, 1000.0], [512.0, 512.0], [0.5, 0.5], [20.0, 30.0], [1023.0, 0.0]]], device=DEV)
    lab = torch.tensor([[-1, 0, 1, 2, 3, 4, -2], [3, 2, 1, 0, -1, 1, 4]], dtype=torch.int32, device=DEV)
    n, P = lab.shape
    gauss, emb, nap = randn(2, nf, seed=C), randn(4, C, seed=C + 1), randn(C, seed=C + 2)
    xy, lab, gauss, emb, nap = (nan_guarded(t) for t in (xy, lab, gauss, emb, nap))
    out = Flat((n, P + n_pad, C), F32)
    reached(L, "prompt_points_kernel", "prompt_points", [
        lambda: L.msam2_prompt_points_padded(xy.data_ptr(), lab.data_ptr(), gauss.data_ptr(), emb.data_ptr(), nap.data_ptr(), out.view.data_ptr(),
                                             n, P, n_pad, C, S, stream())])
    c = 2.0 * ((xy.double() + 0.5) / S) - 1.0                                       # [n, P, 2]
    g = gauss.double()
    tx, ty = c[..., 0:1] * g[0], c[..., 1:2] * g[1]                                 # [n, P, nf]
    a = 2.0 * math.pi * (tx + ty)
    a_terms = 2.0 * math.pi * (tx.abs() + ty.abs())
    pe = torch.cat([a.sin(), a.cos()], -1)
    l64 = lab.long()
    add = torch.where(((l64 >= 0) & (l64 < 4))[..., None], emb.double()[l64.clamp(0, 3)], torch.zeros((), dtype=F64, device=DEV))
    ref = torch.where((l64 == -1)[..., None], nap.double().expand(n, P, C), pe + add)
    bound = torch.where((l64 == -1)[..., None], torch.zeros((), dtype=F64, device=DEV), PB.prompt_points_bound(torch.cat([a_terms, a_terms], -1), 0.0, ref))
    within(out.view[:, :P], ref, bound, f"prompt_points C={C}")
    if n_pad:
        same_bits(out.view[:, P:], nap[None, None].expand(n, n_pad, C), "prompt_points: the padding points")
    same_bits(out.view[0, 0], nap, "prompt_points: label -1")
    assert out.sentinels_intact()


# =================================================================================================================================
# conv3x3s2_ln_gelu
CONV_SHAPES = [(1, 2, 2), (1, 2, 6), (3, 6, 2), (1, 10, 14), (2, 16, 24)]


def conv_params(cin, seed):
    cout = 4 * cin
    w = randn(cout, cin, 3, 3, seed=seed) * (0.5 / math.sqrt(cin))
    return w, randn(cout, seed=seed + 1), 1.0 + 0.2 * randn(cout, seed=seed + 2), 0.2 * randn(cout, seed=seed + 3)


def conv_run(ops, L, key, x_nhwc, B, H, W, cin, params, mode, mscale, mbias, what):
    w, bias, lw, lb = (nan_guarded(t) for t in params)
    x = nan_guarded(x_nhwc)
    out = Flat((B * (H // 2) * (W // 2), 4 * cin), ops.OP16)
    reached(L, key, "conv3x3s2_ln_gelu", [
        lambda: L.msam2_conv3x3s2_ln_gelu(x.data_ptr(), int(cin != 1), w.data_ptr(), bias.data_ptr(), lw.data_ptr(), lb.data_ptr(), out.view.data_ptr(),
                                          B, H, W, cin, 4 * cin, mode, mscale, mbias, stream())])
    v = x.double().view(B, H, W, cin).permute(0, 3, 1, 2)
    dv = 0.0
    if mode == 1:
        v = mscale * torch.sigmoid(v) + mbias
        dv = abs(mscale) * PB.SIGMOID_ABS + 2 * PB.U * (v.abs() + abs(mbias))
    elif mode == 2:
        v = (v > 0).double() * mscale + mbias
    ref, bound = PB.conv3x3s2_ln_gelu_bound(v, dv, w.double(), bias.double(), lw.double(), lb.double(), op16_is_fp16())
    assert bool(torch.isfinite(out.view).all()), what + ": not finite"
    within(out.view, ref, bound, what)
    assert out.sentinels_intact(), what + ": wrote outside its output"


@pytest.mark.parametrize("B,H,W", CONV_SHAPES)
@pytest.mark.parametrize("cin,mode", [(1, 0), (1, 1), (1, 2), (4, 0), (16, 0)])
def test_conv3x3s2_ln_gelu(ops, L, cin, mode, B, H, W):
    key = {1: "conv3x3s2_ln_gelu_kernel<1,4,float>", 4: "conv3x3s2_ln_gelu_kernel<4,16,T16>", 16: "conv3x3s2_ln_gelu_kernel<16,64,T16>"}[cin]
    x = randn(B * H * W, cin, seed=H * W + cin) * (3.0 if mode else 1.0)
    conv_run(ops, L, key, x.to(F32 if cin == 1 else ops.OP16), B, H, W, cin, conv_params(cin, cin), mode, 20.0, -10.0,
             f"conv3x3s2_ln_gelu cin={cin} mode={mode} {B}x{H}x{W}")


def test_conv3x3s2_ln_gelu_mask_mode_edges(ops, L):
    """mode 2 on exactly 0.0 and -0.0 (neither is > 0); mode 1 at +-90, where __expf overflows: finite and within the bound"""
    B, H, W = 1, 6, 10
    x = randn(B * H * W, 1, seed=1)
    x[0::3], x[1::3] = 0.0, -0.0
    conv_run(ops, L, "conv3x3s2_ln_gelu_kernel<1,4,float>", x, B, H, W, 1, conv_params(1, 5), 2, 20.0, -10.0, "conv3x3s2 mode 2 at +-0")
    x = torch.where(randn(B * H * W, 1, seed=2) > 0, 90.0, -90.0)
    x[5], x[17] = 0.5, -0.25
    conv_run(ops, L, "conv3x3s2_ln_gelu_kernel<1,4,float>", x, B, H, W, 1, conv_params(1, 6), 1, 20.0, -10.0, "conv3x3s2 mode 1 at +-90")


def test_conv3x3s2_ln_gelu_grid_stride_wraps(ops, L):
    B, H, W = 1, 2048, 2050
    assert B * (H // 2) * (W // 2) > 8192 * 128
    conv_run(ops, L, "conv3x3s2_ln_gelu_kernel<1,4,float>", randn(B * H * W, 1, seed=3) * 3, B, H, W, 1, conv_params(1, 7), 1, 20.0, -10.0, "conv3x3s2 wrap")


# =================================================================================================================================
# dwconv7x7_ln
@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (1, 3, 5), (2, 7, 7), (1, 9, 13), (1, 16, 18), (1, 5, 23), (2, 16, 16)])
def test_dwconv7x7_ln(ops, L, B, H, W):
    """W % 4 = 0, 1, 2, 3 (the partial last pixel group), images smaller than the filter, a partly empty last block"""
    C = 256
    x, w = randn(B * H * W, C, seed=H * W), randn(C, 1, 7, 7, seed=1) * 0.2
    bias, lw, lb = randn(C, seed=2), 1.0 + 0.2 * randn(C, seed=3), 0.2 * randn(C, seed=4)
    xg, wt = nan_guarded(x), nan_guarded(w.reshape(C, 49).t().contiguous())
    bg, lwg, lbg = nan_guarded(bias), nan_guarded(lw), nan_guarded(lb)
    out = Flat((B * H * W, C), ops.OP16)
    reached(L, "dwconv7x7_ln_kernel", "dwconv7x7_ln", [
        lambda: L.msam2_dwconv7x7_ln(xg.data_ptr(), wt.data_ptr(), bg.data_ptr(), lwg.data_ptr(), lbg.data_ptr(), out.view.data_ptr(), B, H, W, C, stream())])
    ref, bound = PB.dwconv7x7_ln_bound(x.double().view(B, H, W, C).permute(0, 3, 1, 2), w.double(), bias.double(), lw.double(), lb.double(),
                                       op16_is_fp16())
    within(out.view, ref, bound, f"dwconv7x7_ln {B}x{H}x{W}")
    assert out.sentinels_intact()


# =================================================================================================================================
# convt2x2_shuffle / _f32skip / _shared
PS_SHAPES = [(1, 1, 1), (3, 3, 5), (2, 8, 8)]


def ps_data(ops, B, h, w, C, seed):
    g = randn(B * h * w, 4 * C, seed=seed).to(ops.OP16)
    skip = randn(B * 4 * h * w, C, seed=seed + 1).to(ops.OP16)
    return g, skip, randn(C, seed=seed + 2), 1.0 + 0.2 * randn(C, seed=seed + 3), 0.2 * randn(C, seed=seed + 4)


def ps_run(ops, L, key, B, h, w, C, ln, *, skip32=False, shared=False, g_off=0, seed=0):
    """one launch through the entry that `skip32` / `shared` select; returns the output tensor (checked against the bound and its canary)"""
    g, skip, bias, lw, lb = ps_data(ops, B, h, w, C, seed)
    if shared:
        skip = skip[:4 * h * w]
    sk = skip.float() if skip32 else skip
    gg, sg, bg = nan_guarded(g, offset=g_off), nan_guarded(sk), nan_guarded(bias)
    lwg, lbg = (nan_guarded(lw), nan_guarded(lb)) if ln else (None, None)
    pw, pb = (lwg.data_ptr(), lbg.data_ptr()) if ln else (None, None)
    out = Flat((B * 4 * h * w, C), ops.OP16)
    if shared:
        fn = lambda: L.msam2_convt2x2_shuffle_shared(gg.data_ptr(), bg.data_ptr(), sg.data_ptr(), int(not skip32), pw, pb, out.view.data_ptr(), B, h, w, C, 0, stream())
    elif skip32:
        fn = lambda: L.msam2_convt2x2_shuffle_f32skip(gg.data_ptr(), bg.data_ptr(), sg.data_ptr(), pw, pb, out.view.data_ptr(), B, h, w, C, stream())
    else:
        fn = lambda: L.msam2_convt2x2_shuffle(gg.data_ptr(), bg.data_ptr(), sg.data_ptr(), pw, pb, out.view.data_ptr(), B, h, w, C, stream())
    reached(L, key, "pixel_shuffle", [fn])
    full_skip = skip.repeat(B, 1) if shared else skip
    ref, bound = PB.pixel_shuffle_bound(g.double(), bias.double(), full_skip.double(), lw.double() if ln else None, lb.double() if ln else None, B, h, w,
                                        op16_is_fp16())
    what = f"{key} {B}x{h}x{w} C={C} ln={ln} skip32={skip32} shared={shared} g_off={g_off}"
    within(out.view, ref, bound, what)
    assert out.sentinels_intact(), what + ": wrote outside its output"
    return out.view


@pytest.mark.parametrize("B,h,w", PS_SHAPES)
@pytest.mark.parametrize("C", [64, 32])
def test_pixel_shuffle8(ops, L, C, B, h, w):
    """the eight-channel kernel in all its instantiations; (1, 1, 1) leaves lanes of the block without a pixel.  Bit-identities: the shared-skip
    form against the plain form on the repeated map; the fp32 skip against its 16-bit copy (16-bit representable values)"""
    for ln in (True, False):
        outs = {}
        for skip32 in (False, True):
            for shared in (False, True):
                key = f"pixel_shuffle8_kernel<{C},{'float' if skip32 else 'T16'},{'true' if shared else 'false'}>"
                outs[skip32, shared] = ps_run(ops, L, key, B, h, w, C, ln, skip32=skip32, shared=shared, seed=C)
        same_bits(outs[False, False], outs[True, False], "fp32 skip against 16-bit skip")
        same_bits(outs[False, True], outs[True, True], "shared: fp32 skip against 16-bit skip")
        # the shared form reads the first map for every batch element: equal to the plain form on B copies of that map
        g, skip, bias, lw, lb = ps_data(ops, B, h, w, C, C)
        rep = nan_guarded(skip[:4 * h * w].repeat(B, 1))
        gg, bg, lwg, lbg = nan_guarded(g), nan_guarded(bias), nan_guarded(lw), nan_guarded(lb)
        plain = Flat((B * 4 * h * w, C), ops.OP16)
        rc = L.msam2_convt2x2_shuffle(gg.data_ptr(), bg.data_ptr(), rep.data_ptr(), lwg.data_ptr() if ln else None, lbg.data_ptr() if ln else None,
                                      plain.view.data_ptr(), B, h, w, C, stream())
        assert rc == 0
        same_bits(outs[False, True], plain.view, "shared skip against the plain form on the repeated map")


# (C, ln, g offset in elements): ppw = 1 with LayerNorm (any C), C = 48, C = 24, C = 64 eight bytes off; ppw = 2: C = 32 eight bytes off without
# LayerNorm; ppw = 4: C = 16 without LayerNorm; C = 16 with LayerNorm; C = 1
PS_SCALAR = [(32, True, 4), (48, True, 0), (48, False, 0), (24, False, 0), (64, True, 4), (64, False, 4), (32, False, 4), (16, False, 0), (16, True, 0),
             (1, False, 0), (1, True, 0)]


@pytest.mark.parametrize("B,h,w", PS_SHAPES)
def test_pixel_shuffle_scalar(ops, L, B, h, w):
    for C, ln, g_off in PS_SCALAR:
        out = ps_run(ops, L, "pixel_shuffle_kernel", B, h, w, C, ln, g_off=g_off, seed=C)
        if C in (32, 64) and not ln:
            # without LayerNorm both kernels evaluate op2f(g) + bias + skip and the GELU per element in the same order, no reduction: the
            # same bits.  (With LayerNorm the statistics are summed in different orders -- eight per lane and xor-shuffles against a
            # 64-lane butterfly -- so only the bound holds for both.)
            fast = ps_run(ops, L, f"pixel_shuffle8_kernel<{C},T16,false>", B, h, w, C, ln, seed=C)
            same_bits(out, fast, f"pixel_shuffle_kernel against pixel_shuffle8_kernel C={C}")


# =================================================================================================================================
# every kernel instantiation the matrix is meant to reach, as a literal list: the tables above must name each of them
LISTED = sorted(
    [f"layernorm_kernel<{a},{b},{c}>" for a in ("float", "T16") for b in ("float", "T16") for c in (2, 4, 6, 12, 16)]
    + [f"layernorm_scalar_kernel<{a},{b}>" for a in ("float", "T16") for b in ("float", "T16")]
    + [f"add_cast{v}_kernel<{a},{b},{c}>" for v in ("", "_vec") for a in ("float", "T16") for b in ("float", "T16") for c in ("float", "T16")]
    + [f"maxpool2x2_kernel<{a},{b}>" for a in ("float", "T16") for b in ("float", "T16")]
    + ["upsample2x_add_kernel", "upsample2x_add4_kernel", "rope_inplace_kernel", "bilinear_kernel", "bilinear4_kernel", "aa_downsample_kernel",
       "image_prep_kernel", "space_to_depth_kernel<float>", "space_to_depth_kernel<T16>", "im2col3x3s2_kernel", "gate_rows_kernel",
       "any_positive_kernel", "gather_rows_kernel", "obj_ptr_mix_kernel", "non_overlap_kernel", "select_mask_kernel", "hyper_masks_kernel",
       "prompt_points_kernel", "conv3x3s2_ln_gelu_kernel<1,4,float>", "conv3x3s2_ln_gelu_kernel<4,16,T16>", "conv3x3s2_ln_gelu_kernel<16,64,T16>",
       "dwconv7x7_ln_kernel", "pixel_shuffle_kernel"]
    + [f"pixel_shuffle8_kernel<{c},{t},{s}>" for c in (64, 32) for t in ("T16", "float") for s in ("false", "true")])


def expected_keys():
    """the union of the expected kernels of every case table of this file"""
    keys = {f"layernorm_kernel<{tn(ti)},{tn(to)},{ch}>" for ti, to, ch in LN_VEC_CASES}
    keys |= {f"layernorm_scalar_kernel<{tn(ti)},{tn(to)}>" for ti, to in LN_TYPES}
    keys |= {f"add_cast{v}_kernel<{tn(a)},{tn(b)},{tn(o)}>" for v in ("", "_vec") for a, b, o in AC_TYPES}
    keys |= {f"maxpool2x2_kernel<{tn(ti)},{tn(to)}>" for ti, to in LN_TYPES}
    keys |= {c[0] for c in UP_CASES} | {c[0] for c in BIL_CASES} | {"rope_inplace_kernel", "aa_downsample_kernel", "image_prep_kernel"}
    keys |= {f"space_to_depth_kernel<{tn(c[0])}>" for c in S2D_CASES}
    keys |= {"im2col3x3s2_kernel", "gate_rows_kernel", "any_positive_kernel", "gather_rows_kernel", "obj_ptr_mix_kernel", "non_overlap_kernel",
             "select_mask_kernel", "hyper_masks_kernel", "prompt_points_kernel", "dwconv7x7_ln_kernel"}
    keys |= {"conv3x3s2_ln_gelu_kernel<1,4,float>", "conv3x3s2_ln_gelu_kernel<4,16,T16>", "conv3x3s2_ln_gelu_kernel<16,64,T16>"}
    keys |= {"pixel_shuffle_kernel"} | {f"pixel_shuffle8_kernel<{c},{t},{s}>" for c in (64, 32) for t in ("T16", "float") for s in ("false", "true")}
    return keys


def test_every_listed_instantiation_has_a_case(ops):
    assert sorted(expected_keys()) == LISTED
    assert len({K(k) for k in LISTED}) == len(LISTED)
