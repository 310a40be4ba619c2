"""Variant matrix of the training-side pointwise and row kernels (GPU): the 63 kernel instantiations that the 27 non-GEMM, non-attention entries
of csrc/backward.hip launch, each reached on purpose through its C entry and checked at its edges, in the style of
tests/test_pointwise_variants_gpu.py:
  * each group of launches names the instantiation it must reach; torch.profiler asserts that exactly that one ran among the kernels with the
    entry's prefix (EXPECTED lists them all; test_every_listed_instantiation_has_a_case compares it with a literal list);
  * scalar forms are reached by width or by alignment, never by an environment switch;
  * inputs are views inside NaN-filled buffers (strided where the entry takes a stride, NaN guards on either side otherwise);
  * every output -- the in-place buffers of Adam and window_move and the workspace of hiera_pos_embed_bwd included -- lies between sentinels,
    which must be bit-identical afterwards; accumulated outputs start from a non-zero value;
  * float64 references run on the GPU from the operand-rounded inputs; arithmetic lies element by element within the derived bounds of
    tests/backward_bounds.py (no tolerance here is taken from a kernel's output); pure data movement is bit-exact.
The 16-bit type is ops.OP16 throughout (T16 in the kernel keys), so the bf16 build runs the file unchanged.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backward_bounds as BB  # noqa: E402
import pointwise_bounds as PB  # noqa: E402
from helpers import SENT16, SENT32, Canvas2, Flat, K, kernels_launched, nan_guarded, op16_is_fp16, same_bits, strided_nan, within  # noqa: E402,F401

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


def randint(lo, hi, *shape, seed=0):
    return torch.randint(lo, hi, shape, generator=gen(seed), device=DEV).float()


def reached(L, keys, prefix, launches):
    """run the launches (callables returning the C entry's code) under the profiler: all succeed, and exactly `keys` (one key or a set) ran
    among the kernels whose name starts with `prefix`"""
    def go():
        for fn in launches:
            rc = fn()
            assert rc == 0, L.msam2_last_error().decode()
    got = kernels_launched(go, prefix)
    want = {K(k) for k in ({keys} if isinstance(keys, str) else keys)}
    assert got == want, f"expected {sorted(want)}, launched {sorted(got)}"


def flat_with(values):
    """a sentinel-guarded output that starts from `values` (accumulated or in-place outputs)"""
    f = Flat(tuple(values.shape), values.dtype)
    f.view.copy_(values)
    return f


# =================================================================================================================================
# LayerNorm backward
LNB_SCALAR_C = {1: (1, 63), 2: (65, 127), 4: (129, 255), 6: (257, 383), 8: (385, 512), 12: (513, 768), 16: (769, 1024)}
LNB_VEC_C = {1: (4, 64), 2: (68, 128), 3: (132, 192), 4: (196, 256), 6: (260, 320, 324, 384)}
LNB_ROWS = [1, 17, 33]
LNB_SCALAR_CASES = [(td, ni) for td in (32, 16) for ni in LNB_SCALAR_C]
LNB_VEC_CASES = [(td, ch) for td in (32, 16) for ch in LNB_VEC_C]


def lnb_data(ops, rows, C, td, seed):
    """x like ln_data of the forward matrix (rows of different scale, one row with mean = 1000 std, a constant last row), gamma with mixed
    signs, dy of different scale per row rounded to its type, a residual gradient, and non-zero dgamma / dbeta to add into"""
    ar = torch.arange(rows, device=DEV)
    x = randn(rows, C, seed=seed) * (0.5 + (ar % 4).float())[:, None] + 2.0 * ((ar % 3).float() - 1)[:, None]
    if rows > 2:
        x[1] = 1000.0 + randn(C, seed=seed + 1)
    if rows > 1:
        x[rows - 1] = 2.0
    gamma = (1.0 + 0.5 * randn(C, seed=seed + 2)) * torch.where(torch.arange(C, device=DEV) % 3 == 0, -1.0, 1.0)
    dy = (randn(rows, C, seed=seed + 3) * (0.25 + (ar % 5).float())[:, None]).to(dt(ops, td))
    return x, gamma, dy, randn(rows, C, seed=seed + 4), randn(C, seed=seed + 5), randn(C, seed=seed + 6)


class LnbJob:
    """one msam2_layernorm_bwd call: ldx, ldd, ldo, lda all different from C and from each other (multiples of four unless `odd`); x_off /
    dy_off move a base by that many elements; ldo overrides the output stride"""

    def __init__(self, ops, L, td, C, rows, with_add, *, odd=False, x_off=0, dy_off=0, ldo=None, seed=0, ldx=None, ldd=None, lda=None, dx_left=0,
                 add_off=0, gamma_off=0):
        self.L, self.td, self.C, self.rows = L, td, C, rows
        self.what = (f"layernorm_bwd dy={tn(td)} C={C} rows={rows} add={with_add} odd={odd} x_off={x_off} dy_off={dy_off} ldo={ldo} ldx={ldx} "
                     f"ldd={ldd} lda={lda} dx_left={dx_left} add_off={add_off} gamma_off={gamma_off}")
        x, gamma, dy, add, self.g0, self.b0 = lnb_data(ops, rows, C, td, seed)
        p = (3, 5, 7, 9) if odd else (4, 8, 12, 16)
        self.x = strided_nan(x, ldx if ldx is not None else C + p[0], x_off)
        self.dy = strided_nan(dy, ldd if ldd is not None else C + p[1], dy_off)
        self.gamma = nan_guarded(gamma, gamma_off)
        self.add = strided_nan(add, lda if lda is not None else C + p[3], add_off) if with_add else None
        self.dx = Canvas2(rows, C, F32, ldo if ldo is not None else C + p[2], dx_left)
        self.dg, self.db = flat_with(self.g0), flat_with(self.b0)

    def launch(self):
        a = self.add
        return self.L.msam2_layernorm_bwd(self.x.data_ptr(), self.x.stride(0), self.dy.data_ptr(), int(self.td == 16), self.dy.stride(0),
                                          self.gamma.data_ptr(), self.dx.view.data_ptr(), self.dx.view.stride(0), self.dg.view.data_ptr(),
                                          self.db.view.data_ptr(), self.rows, self.C, 1e-6, a.data_ptr() if a is not None else None,
                                          a.stride(0) if a is not None else 0, stream())

    def check(self):
        refs, bounds = BB.layernorm_bwd_bound(self.x.double(), self.dy.double(), self.gamma.double(), 1e-6,
                                              self.add.double() if self.add is not None else None, self.g0.double(), self.b0.double())
        within(self.dx.view, refs[0], bounds[0], self.what + ": dx")
        within(self.dg.view, refs[1], bounds[1], self.what + ": dgamma")
        within(self.db.view, refs[2], bounds[2], self.what + ": dbeta")
        assert self.dx.sentinels_intact() and self.dg.sentinels_intact() and self.db.sentinels_intact(), self.what + ": wrote outside an output"


def run_lnb(L, key, jobs):
    reached(L, key, "layernorm_bwd_", [j.launch for j in jobs])
    for j in jobs:
        j.check()


@pytest.mark.parametrize("td,ni", LNB_SCALAR_CASES)
def test_layernorm_bwd_scalar(ops, L, td, ni):
    """both ends of each NI band, odd strides (so the vector test fails whatever C is); C = 128 reaches NI = 2 when x is one float off a
    16-byte boundary and again when ldo is odd"""
    jobs = [LnbJob(ops, L, td, C, rows, a, odd=True, seed=C + rows) for C in LNB_SCALAR_C[ni] for rows in LNB_ROWS for a in (False, True)]
    if ni == 2:
        jobs += [LnbJob(ops, L, td, 128, 17, True, x_off=1, seed=3), LnbJob(ops, L, td, 128, 17, False, ldo=141, seed=4)]
    run_lnb(L, f"layernorm_bwd_kernel<{tn(td)},{ni}>", jobs)


@pytest.mark.parametrize("td,ch", LNB_VEC_CASES)
def test_layernorm_bwd_vector(ops, L, td, ch):
    """both ends of each CHUNKS band (CHUNKS = 6 also at the five-chunk widths, where one lane group is half empty); 16-bit dy that is only
    8-byte aligned stays on the vector kernel"""
    jobs = [LnbJob(ops, L, td, C, rows, a, seed=C + rows) for C in LNB_VEC_C[ch] for rows in LNB_ROWS for a in (False, True)]
    if td == 16:
        jobs.append(LnbJob(ops, L, td, LNB_VEC_C[ch][-1], 17, True, dy_off=4, seed=5))
    run_lnb(L, f"layernorm_bwd_vec_kernel<{tn(td)},{ch}>", jobs)


@pytest.mark.parametrize("td", [32, 16])
def test_layernorm_bwd_scalar_by_one_term_each(ops, L, td):
    """rows = 17, every stride a multiple of four and every base aligned except ONE term of the vector test (the terms
    test_layernorm_bwd_scalar does not flip on their own: its odd strides break ldx, ldd, ldo and lda together with C % 4 and C <= 384).
    C = 128 (NI = 2): ldx, ldd, lda off by one; dx, dy, add, gamma one element off; an fp32 dy that is only 8-byte aligned (the dy test goes
    by element size: a 16-bit dy there stays on the vector kernel, test_layernorm_bwd_vector).  C = 126: C % 4 alone.  C = 388 (NI = 8):
    C <= 384 alone."""
    rows = 17
    one = [dict(ldx=133), dict(ldd=137), dict(lda=145), dict(dx_left=1), dict(dy_off=1), dict(add_off=1), dict(gamma_off=1)]
    if td == 32:
        one.append(dict(dy_off=2))
    run_lnb(L, f"layernorm_bwd_kernel<{tn(td)},2>", [LnbJob(ops, L, td, 128, rows, True, seed=10 + i, **kw) for i, kw in enumerate(one)] +
            [LnbJob(ops, L, td, 126, rows, True, ldx=132, ldd=136, ldo=140, lda=144, seed=20)])
    run_lnb(L, f"layernorm_bwd_kernel<{tn(td)},8>", [LnbJob(ops, L, td, 388, rows, True, seed=21)])


@pytest.mark.parametrize("td,rows", [(32, 4097), (16, 32769)])
def test_layernorm_bwd_row_loop_and_large_grid(ops, L, td, rows):
    """C = 4: rows = 4097 is the second trip of the row loop at 256 workgroups x 16 rows, rows = 32769 the 512-workgroup grid"""
    run_lnb(L, f"layernorm_bwd_vec_kernel<{tn(td)},1>", [LnbJob(ops, L, td, 4, rows, True, seed=rows)])


# =================================================================================================================================
# activation backward
ACT_TYPES = [(32, 32), (32, 16), (16, 32), (16, 16)]


def act_data(ops, n, tp, td, seed=0):
    """pre: +-0.443 (the polynomial's worst point), +-4.5 (its clamp), 0 and +-10 first, then a fine grid over [-6, 6]; dy up to the fp16
    maximum (the store saturates in the fp16 build)"""
    base = torch.cat([torch.tensor([0.443, -0.443, 4.5, -4.5, 0.0, 10.0, -10.0], device=DEV), torch.linspace(-6, 6, 2041, device=DEV)])
    pre = base[torch.arange(n, device=DEV) % base.numel()]
    dy = randn(n, seed=seed + n % 1000) * 3
    dy[::97] = 65504.0
    dy[1::97] = -65504.0
    return pre.to(dt(ops, tp)), dy.to(dt(ops, td))


class ActJob:
    def __init__(self, ops, L, tp, td, n, act, *, offs=(0, 0, 0), seed=0):
        self.ops, self.L, self.n, self.act = ops, L, n, act
        pre, dy = act_data(ops, n, tp, td, seed)
        self.pre, self.dy = nan_guarded(pre, offs[0]), nan_guarded(dy, offs[1])
        self.out = Flat((n,), ops.OP16, offs[2])
        self.what = f"act_bwd {tn(tp)},{tn(td)} n={n} act={act} offsets={offs}"

    def launch(self):
        o = self.ops
        return self.L.msam2_act_bwd(self.pre.data_ptr(), int(self.pre.dtype == o.OP16), self.dy.data_ptr(), int(self.dy.dtype == o.OP16),
                                    self.out.view.data_ptr(), self.n, self.act, stream())

    def check(self, poly):
        ref, bound = BB.act_bwd_bound(self.pre.double(), self.dy.double(), self.act, poly, op16_is_fp16())
        within(self.out.view, ref, bound, self.what)
        assert self.out.sentinels_intact(), self.what + ": wrote outside its output"


def off8(bits):
    """elements in 8 bytes"""
    return 2 if bits == 32 else 4


@pytest.mark.parametrize("tp,td", ACT_TYPES)
def test_act_bwd_vector(ops, L, tp, td):
    """n / 8 in {1, 7, 8, 257}"""
    jobs = [ActJob(ops, L, tp, td, n, act) for n in (8, 56, 64, 2056) for act in (1, 2)]
    reached(L, f"act_bwd_vec_kernel<{tn(tp)},{tn(td)}>", "act_bwd_", [j.launch for j in jobs])
    for j in jobs:
        j.check(True)


@pytest.mark.parametrize("tp,td", ACT_TYPES)
def test_act_bwd_scalar(ops, L, tp, td):
    """n % 8 != 0; n = 2056 with pre, dy or out 8 bytes off a 16-byte boundary"""
    jobs = [ActJob(ops, L, tp, td, n, act) for n in (1, 7, 2055) for act in (1, 2)]
    jobs += [ActJob(ops, L, tp, td, 2056, 1, offs=o) for o in ((off8(tp), 0, 0), (0, off8(td), 0), (0, 0, 4))]
    reached(L, f"act_bwd_kernel<{tn(tp)},{tn(td)}>", "act_bwd_", [j.launch for j in jobs])
    for j in jobs:
        j.check(False)


@pytest.mark.parametrize("tp,td", ACT_TYPES)
def test_act_bwd_forms_agree(ops, L, tp, td):
    """the vector form takes Phi from the polynomial of csrc/common.h, the scalar form from erff(): on equal inputs they may differ by
    GELU_CDF_ABS |dy| and the two 16-bit roundings, and by no more (ReLU: not at all)"""
    n = 2056
    for act in (1, 2):
        a, b = ActJob(ops, L, tp, td, n, act), ActJob(ops, L, tp, td, n, act, offs=(0, 0, 4))
        reached(L, f"act_bwd_vec_kernel<{tn(tp)},{tn(td)}>", "act_bwd_", [a.launch])
        reached(L, f"act_bwd_kernel<{tn(tp)},{tn(td)}>", "act_bwd_", [b.launch])
        if act == 2:
            same_bits(a.out.view, b.out.view, "relu': the two forms")
            continue
        ref, _ = BB.act_bwd_bound(a.pre.double(), a.dy.double(), 1, True, op16_is_fp16())
        e = BB.GELU_CDF_ABS * a.dy.double().abs() + 16 * BB.U * ref.abs()
        within(a.out.view, b.out.view.double(), 2 * (PB.store16(ref, e, op16_is_fp16()) - e) + e, "gelu': the two forms")
        e5 = 1e-5 * a.dy.double().abs() + 16 * BB.U * ref.abs()                    # (a figure, not a check: the comment the kernel used to carry)
        beyond = int(((a.out.view.double() - b.out.view.double()).abs() > 2 * (PB.store16(ref, e5, op16_is_fp16()) - e5) + e5).sum())
        print(f"act_bwd forms {tn(tp)},{tn(td)}: {beyond} of {n} elements differ by more than a 1e-5 error of Phi would allow")


@pytest.mark.parametrize("key,n", [("act_bwd_kernel<float,float>", 16384 * 256 + 1), ("act_bwd_vec_kernel<T16,T16>", 8 * (8192 * 256 + 1))])
def test_act_bwd_grid_stride_wraps(ops, L, key, n):
    t = 32 if "float" in key else 16
    j = ActJob(ops, L, t, t, n, 1)
    reached(L, key, "act_bwd_", [j.launch])
    j.check("vec" in key)


# =================================================================================================================================
# colsum, transpose16
RC_SHAPES = [(R, C) for R in (1, 255, 257, 65537) for C in (1, 63, 65)]


@pytest.mark.parametrize("t", [32, 16])
def test_colsum(ops, L, t):
    """integer-valued data: exact in any order; R = 65537 gives 256 slabs and a ragged last slab; the output is added into"""
    jobs = []
    for R, C in RC_SHAPES:
        x = strided_nan(randint(-3, 4, R, C, seed=R + C).to(dt(ops, t)), C + 3)
        init = randint(-5, 6, C, seed=C)
        jobs.append((x, init, flat_with(init)))
    reached(L, f"colsum_kernel<{tn(t)}>", "colsum_kernel", [lambda x=x, o=o: L.msam2_colsum(x.data_ptr(), int(t == 16), x.stride(0), o.view.data_ptr(), x.shape[0],
                                                                                        x.shape[1], stream()) for x, _, o in jobs])
    for x, init, o in jobs:
        same_bits(o.view, (init.double() + x.double().sum(0)).float(), f"colsum {tuple(x.shape)}")
        assert o.sentinels_intact()


def test_transpose16(ops, L):
    jobs = []
    for R, C in RC_SHAPES:
        x = strided_nan(randn(R, C, seed=R + C).to(ops.OP16), C + 3)
        jobs.append((x, Canvas2(C, R, ops.OP16, R + 5, 1)))
    reached(L, "transpose16_kernel", "transpose16", [lambda x=x, o=o: L.msam2_transpose16(x.data_ptr(), x.stride(0), o.view.data_ptr(), o.view.stride(0), x.shape[0],
                                                                                        x.shape[1], stream()) for x, o in jobs])
    for x, o in jobs:
        same_bits(o.view, x.t(), f"transpose16 {tuple(x.shape)}")
        assert o.sentinels_intact()


# =================================================================================================================================
# softmax rows
SM_SHAPES = [(rows, cols) for rows in (1, 3, 5) for cols in (1, 63, 64, 65, 200)]


def softmax_data(rows, cols, seed):
    s = randn(rows, cols, seed=seed) * 3
    if cols > 1:
        s[0] = torch.linspace(40.0, 100.0, cols, device=DEV)  # a spread of 60, far from zero
    if rows > 1:
        s[rows - 1] = 0.7                                     # equal logits
    return s


def test_softmax_rows(ops, L):
    jobs = []
    for rows, cols in SM_SHAPES:
        for scale in (0.125, 1.0):
            jobs.append((strided_nan(softmax_data(rows, cols, rows + cols), cols + 3), scale, Canvas2(rows, cols, ops.OP16, cols + 5, 1)))
    reached(L, "softmax_rows_kernel", "softmax_rows", [lambda s=s, sc=sc, o=o: L.msam2_softmax_rows(s.data_ptr(), s.stride(0), o.view.data_ptr(), o.view.stride(0),
                                                                                                 s.shape[0], s.shape[1], sc, stream()) for s, sc, o in jobs])
    for s, sc, o in jobs:
        ref, bound = BB.softmax_rows_bound(s.double(), BB.f32(sc), op16_is_fp16())
        within(o.view, ref, bound, f"softmax_rows {tuple(s.shape)} scale={sc}")
        assert o.sentinels_intact()


def test_softmax_bwd_rows(ops, L):
    jobs = []
    for rows, cols in SM_SHAPES:
        for scale in (0.125, 1.0):
            p = torch.softmax(softmax_data(rows, cols, rows + cols).double() * scale, -1).to(ops.OP16)
            jobs.append((strided_nan(p, cols + 3), strided_nan(randn(rows, cols, seed=cols) * 2, cols + 7), scale, Canvas2(rows, cols, ops.OP16, cols + 5, 1)))
    reached(L, "softmax_bwd_rows_kernel", "softmax_bwd_rows", [
        lambda p=p, d=d, sc=sc, o=o: L.msam2_softmax_bwd_rows(p.data_ptr(), p.stride(0), d.data_ptr(), d.stride(0), o.view.data_ptr(), o.view.stride(0),
                                                            p.shape[0], p.shape[1], sc, stream()) for p, d, sc, o in jobs])
    for p, d, sc, o in jobs:
        ref, bound = BB.softmax_bwd_rows_bound(p.double(), d.double(), BB.f32(sc), op16_is_fp16())
        within(o.view, ref, bound, f"softmax_bwd_rows {tuple(p.shape)} scale={sc}")
        assert o.sentinels_intact()


# =================================================================================================================================
# ConvTranspose2d(k2, s2) tails
CONVT_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (1, 2, 2, 64)]
CONVT_WRAP = (1, 1, 149797, 7)       # 4 B h w C is a multiple of 4 C, so 16384 * 256 + C cannot be met: the smallest total above 16384 * 256 at C = 7


def convt_gather_job(ops, L, B, h, w, C, with_skip):
    g = nan_guarded(randn(B * h * w, 4 * C, seed=C).to(ops.OP16))
    bias = nan_guarded(randn(C, seed=C + 1))
    skip = nan_guarded(randn(B * 4 * h * w, C, seed=C + 2).to(ops.OP16)) if with_skip else None
    z = Flat((B * 4 * h * w, C), F32)
    launch = lambda: L.msam2_convt2x2_gather(g.data_ptr(), bias.data_ptr(), skip.data_ptr() if skip is not None else None, z.view.data_ptr(), B, h, w, C, stream())

    def check():
        ref, bound = BB.convt2x2_gather_bound(g.double(), bias.double(), skip.double() if skip is not None else None, B, h, w)
        within(z.view, ref, bound, f"convt2x2_gather {(B, h, w, C)} skip={with_skip}")
        assert z.sentinels_intact()
    return launch, check


@pytest.mark.parametrize("shapes", [CONVT_SHAPES, [CONVT_WRAP]], ids=["edges", "wrap"])
def test_convt2x2_gather(ops, L, shapes):
    jobs = [convt_gather_job(ops, L, *s, with_skip=k) for s in shapes for k in ((False, True) if len(shapes) > 1 else (True,))]
    reached(L, "convt2x2_gather_kernel", "convt2x2_", [j[0] for j in jobs])
    for j in jobs:
        j[1]()


@pytest.mark.parametrize("t", [32, 16])
def test_convt2x2_scatter_grad(ops, L, t):
    """bit-exact after the 16-bit rounding; the wrap case runs in the fp32 instantiation"""
    jobs = []
    for B, h, w, C in CONVT_SHAPES + ([CONVT_WRAP] if t == 32 else []):
        dz = nan_guarded(randn(B * 4 * h * w, C, seed=C + 3).to(dt(ops, t)))
        jobs.append((dz, Flat((B * h * w, 4 * C), ops.OP16), (B, h, w, C)))
    reached(L, f"convt2x2_scatter_grad_kernel<{tn(t)}>", "convt2x2_", [lambda dz=dz, o=o, s=s: L.msam2_convt2x2_scatter_grad(dz.data_ptr(), int(t == 16), o.view.data_ptr(),
                                                                                                                           *s, stream()) for dz, o, s in jobs])
    for dz, o, s in jobs:
        same_bits(o.view, BB.convt_unsub(dz.to(ops.OP16), *s), f"convt2x2_scatter_grad {s}")
        assert o.sentinels_intact()


# =================================================================================================================================
# depthwise 7x7, its weight gradient, col2im
DW_HW = [(1, 1), (2, 5), (7, 7), (9, 13)]


def nchw(t, B, H, W):
    return t.view(B, H, W, -1).permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def test_dwconv7x7(ops, L):
    """an image smaller than the kernel and a 1-pixel image make every tap a border; both flips, bias and none; the flipped correlation without
    a bias equals the autograd input gradient of the forward convolution"""
    B, jobs = 2, []
    for H, W in DW_HW:
        for C in (4, 68):
            for flip in (0, 1):
                for with_bias in (False, True):
                    x, w = nan_guarded(randn(B * H * W, C, seed=H + C)), nan_guarded(randn(49, C, seed=C))
                    bias = nan_guarded(randn(C, seed=C + 1)) if with_bias else None
                    jobs.append((x, w, bias, Flat((B * H * W, C), F32), (B, H, W, C), flip))
    reached(L, "dwconv7x7_kernel", "dwconv7x7_", [lambda x=x, w=w, b=b, o=o, s=s, f=f: L.msam2_dwconv7x7(x.data_ptr(), w.data_ptr(), b.data_ptr() if b is not None else None,
                                                                                                       o.view.data_ptr(), *s, f, stream()) for x, w, b, o, s, f in jobs])
    for x, w, b, o, s, f in jobs:
        Bn, H, W, C = s
        ref, bound = BB.dwconv7x7_bound(nchw(x.double(), Bn, H, W), w.double(), b.double() if b is not None else None, f)
        within(o.view, nhwc(ref), nhwc(bound), f"dwconv7x7 {s} flip={f} bias={b is not None}")
        assert o.sentinels_intact()
        if f and b is None:
            xg = torch.zeros(Bn, C, H, W, dtype=F64, device=DEV, requires_grad=True)
            F.conv2d(xg, BB.dw_taps(w.double()), None, padding=3, groups=C).backward(nchw(x.double(), Bn, H, W))
            assert float((ref - xg.grad).abs().max()) <= 1e-12 * float(ref.abs().max() + 1)


def test_dwconv7x7_wgrad(ops, L):
    """the last case has more than 512 * 32 pixels, so a slab takes more than 32 of them; the output is added into"""
    jobs = []
    for (H, W), C, B in [(hw, C, 2) for hw in DW_HW for C in (1, 63, 65)] + [((129, 128), 65, 1)]:
        x, dy = nan_guarded(randn(B * H * W, C, seed=H + C)), nan_guarded(randn(B * H * W, C, seed=H + C + 1))
        init = randn(49, C, seed=C + 2)
        jobs.append((x, dy, init, flat_with(init), (B, H, W, C)))
    reached(L, "dwconv7x7_wgrad_kernel", "dwconv7x7_", [lambda x=x, d=d, o=o, s=s: L.msam2_dwconv7x7_wgrad(x.data_ptr(), d.data_ptr(), o.view.data_ptr(), *s, stream())
                                                      for x, d, _, o, s in jobs])
    for x, d, init, o, s in jobs:
        ref, bound = BB.dwconv7x7_wgrad_bound(nchw(x.double(), *s[:3]), nchw(d.double(), *s[:3]), init.double())
        within(o.view, ref, bound, f"dwconv7x7_wgrad {s}")
        assert o.sentinels_intact()


def test_col2im3x3s2(ops, L):
    """H and W even (the entry's contract), ld > 9 C; checked against the autograd adjoint of unfold"""
    B, jobs = 2, []
    for H, W in [(2, 2), (2, 6), (8, 8), (10, 14)]:
        for C in (1, 63, 65):
            jobs.append((strided_nan(randn(B * (H // 2) * (W // 2), 9 * C, seed=H + C), 9 * C + 5), Flat((B * H * W, C), F32), (B, H, W, C)))
    reached(L, "col2im3x3s2_kernel", "col2im", [lambda d=d, o=o, s=s: L.msam2_col2im3x3s2(d.data_ptr(), d.stride(0), o.view.data_ptr(), *s, stream()) for d, o, s in jobs])
    for d, o, s in jobs:
        Bn, H, W, C = s
        ref, bound = BB.col2im3x3s2_bound(d.double().contiguous(), *s)
        xg = torch.zeros(Bn, C, H, W, dtype=F64, device=DEV, requires_grad=True)
        F.unfold(xg, 3, padding=1, stride=2).view(Bn, C, 9, -1).permute(0, 3, 2, 1).reshape(-1, 9 * C).backward(d.double())
        assert float((ref - nhwc(xg.grad)).abs().max()) <= 1e-12
        within(o.view, ref, bound, f"col2im3x3s2 {s}")
        assert o.sentinels_intact()


# =================================================================================================================================
# bilinear adjoint
BIL_SHAPES = [(1, 1, 1, 1), (1, 1, 5, 3), (7, 5, 7, 5), (3, 4, 10, 9), (16, 24, 50, 97), (5, 5, 20, 20)]


def test_bilinear_upsample_bwd(ops, L):
    jobs = [(nan_guarded(randn(P, H, W, seed=H + W + P)), Flat((P, h, w), F32), (P, h, w, H, W)) for h, w, H, W in BIL_SHAPES for P in (1, 3)]
    reached(L, "bilinear_bwd_kernel", "bilinear_bwd", [lambda g=g, o=o, s=s: L.msam2_bilinear_upsample_bwd(g.data_ptr(), o.view.data_ptr(), *s, stream()) for g, o, s in jobs])
    for g, o, s in jobs:
        P, h, w, H, W = s
        ref, bound = BB.bilinear_bwd_bound(g.double(), h, w)
        x = torch.zeros(P, h, w, dtype=F64, device=DEV, requires_grad=True)
        PB.bilinear_ref(x, H, W)[0].backward(g.double())
        assert float((ref - x.grad).abs().max()) <= 1e-12 * float(ref.abs().max() + 1), "the reference is the adjoint of pointwise_bounds.bilinear_ref"
        within(o.view, ref, bound, f"bilinear_upsample_bwd {s}")
        assert o.sentinels_intact()


# =================================================================================================================================
# loss and optimiser
def bce_data(n, seed):
    x = randn(n, seed=seed) * 4
    y = torch.tensor([0.0, 1.0, 0.3], device=DEV)[torch.arange(n, device=DEV) % 3]
    for i, v in enumerate((100.0, -100.0, 0.0, 100.0, -100.0, 0.0)):
        if i < n:
            x[i] = v
    return x, y


def test_bce_logits(ops, L):
    """logits including +-100 and 0 against every target value; the loss is added into a non-zero scalar"""
    jobs = []
    for n in (1, 63, 257, 1024 * 256 + 1):
        for pw in (1.0, 2.5):
            x, y = bce_data(n, n)
            jobs.append((nan_guarded(x), nan_guarded(y), Flat((n,), F32), flat_with(torch.full((1,), 0.75, device=DEV)), pw))
    reached(L, "bce_logits_kernel", "bce_logits", [lambda x=x, y=y, d=d, l=l, pw=pw: L.msam2_bce_logits(x.data_ptr(), y.data_ptr(), d.view.data_ptr(), l.view.data_ptr(),
                                                                                                      x.numel(), pw, stream()) for x, y, d, l, pw in jobs])
    for x, y, d, l, pw in jobs:
        refs, bounds = BB.bce_logits_bound(x.double(), y.double(), pw, 0.75)
        within(l.view, refs[0].view(1), bounds[0].view(1), f"bce loss n={x.numel()} pos_weight={pw}")
        within(d.view, refs[1], bounds[1], f"bce gradient n={x.numel()} pos_weight={pw}")
        assert d.sentinels_intact() and l.sentinels_intact()


ADAM = dict(lr=BB.f32(1e-2), b1=BB.f32(0.9), b2=BB.f32(0.999), eps=BB.f32(1e-8))


def adam_state(n, seed, fresh):
    p, g = randn(n, seed=seed), randn(n, seed=seed + 1) * 0.1
    m, v = randn(n, seed=seed + 2) * 0.05, (randn(n, seed=seed + 3) * 0.03) ** 2
    if fresh:
        m, v = torch.zeros_like(m), torch.zeros_like(v)
    g[0] = 0.0
    v[0] = 0.0
    return p, g, m, v


@pytest.mark.parametrize("step", [1, 1000])
def test_adam_step(ops, L, step):
    jobs = []
    for n in (1, 257, 4096 * 256 + 1):
        p, g, m, v = adam_state(n, n, step == 1)
        jobs.append(((p, g, m, v), flat_with(p), nan_guarded(g), flat_with(m), flat_with(v)))
    a = ADAM
    reached(L, "adam_step_kernel", "adam_", [lambda P=P, G=G, M=M, V=V: L.msam2_adam_step(P.view.data_ptr(), G.data_ptr(), M.view.data_ptr(), V.view.data_ptr(), G.numel(),
                                                                                       a["lr"], a["b1"], a["b2"], a["eps"], step, stream()) for _, P, G, M, V in jobs])
    for init, P, G, M, V in jobs:
        refs, bounds = BB.adam_bound(*[t.double() for t in init], a["lr"], a["b1"], a["b2"], a["eps"], step)
        for name, o, r, b in zip("pmv", (P, M, V), refs, bounds):
            within(o.view, r, b, f"adam_step {name} n={G.numel()} step={step}")
            assert o.sentinels_intact()


ADAM_SIZES = [1, 128 * 256 + 1, 7, 300, 64, 1000]


@pytest.mark.parametrize("count,device_step", [(1, False), (24, True), (25, False), (49, True)])
def test_adam_step_multi(ops, L, count, device_step):
    """tensor counts at the edges of ADAM_CHUNK, unequal sizes; grad_scale and weight_decay non-trivial; +-inf and NaN gradient elements leave
    p, m and v bit-identical and are counted one by one"""
    step, gscale, wd, a = 1000, BB.f32(1 / 128), BB.f32(0.1), ADAM
    tensors, n_bad = [], 0
    for i in range(count):
        n = ADAM_SIZES[i % len(ADAM_SIZES)]
        p, g, m, v = adam_state(n, 10 * i, False)
        g = g * 128
        bad = torch.zeros(n, dtype=torch.bool, device=DEV)
        if n > 3 and i % 2 == 0:
            g[1], g[2], g[n - 1] = float("inf"), float("-inf"), float("nan")
            bad[1] = bad[2] = bad[n - 1] = True
            n_bad += 3
        tensors.append(((p, g, m, v), bad, flat_with(p), nan_guarded(g), flat_with(m), flat_with(v)))
    tabs = [(ctypes.c_void_p * count)(*[(t[k].view if k != 3 else t[k]).data_ptr() for t in tensors]) for k in (2, 3, 4, 5)]
    numel = (ctypes.c_int64 * count)(*[t[3].numel() for t in tensors])
    ctr = torch.tensor([7, step - 1, 5, 7], dtype=torch.int32, device=DEV)          # [guard, step counter, skipped (added into), guard]
    launch = lambda: L.msam2_adam_step_multi(tabs[0], tabs[1], tabs[2], tabs[3], numel, count, a["lr"], a["b1"], a["b2"], a["eps"], 0 if device_step else step,
                                             gscale, wd, ctr[1:].data_ptr() if device_step else None, ctr[2:].data_ptr(), stream())
    reached(L, {"adam_tick_kernel", "adam_multi_kernel"} if device_step else "adam_multi_kernel", "adam_", [launch])
    assert ctr.tolist() == [7, step if device_step else step - 1, 5 + n_bad, 7]
    for (p, g, m, v), bad, P, G, M, V in tensors:
        g0 = torch.where(bad, torch.zeros_like(g), g)
        refs, bounds = BB.adam_bound(p.double(), g0.double(), m.double(), v.double(), a["lr"], a["b1"], a["b2"], a["eps"], step, gscale, wd, device_step)
        for name, o, init, r, b in zip("pmv", (P, M, V), (p, m, v), refs, bounds):
            within(o.view[~bad], r[~bad], b[~bad], f"adam_step_multi {name} n={g.numel()} of {count} device_step={device_step}")
            same_bits(o.view[bad], init[bad], f"adam_step_multi {name}: elements with a non-finite gradient")
            assert o.sentinels_intact()


# =================================================================================================================================
# maxpool2x2 backward, sumpool2x2
POOL_SHAPES = [(1, 2, 2, 1), (2, 6, 8, 40), (1, 4, 2, 65)]


def pool_bwd_input(B, H, W, C, seed):
    """small integers (ties everywhere); in channel 0 of the larger shapes: windows with a tie of the maximum in each of the six pair positions,
    an all-equal window, and a NaN in each of the four positions"""
    x = randint(0, 3, B, H // 2, W // 2, C, 2, 2, seed=seed)
    wins = x.view(-1, C, 4)
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    if wins.shape[0] >= 11:
        for k, (i, j) in enumerate(pairs):
            wins[k, 0] = 1.0
            wins[k, 0, i] = wins[k, 0, j] = 5.0
        wins[6, 0] = 4.0
        for k in range(4):
            wins[7 + k, 0] = torch.tensor([3.0, 1.0, 2.0, 0.0], device=DEV).roll(k)
            wins[7 + k, 0, k] = float("nan")
    elif wins.shape[0] >= 2:
        wins[0, 0] = torch.tensor([1.0, 5.0, 5.0, 0.0], device=DEV)
        wins[1, 0] = torch.tensor([2.0, float("nan"), 3.0, 3.0], device=DEV)
    return x.view(B, H // 2, W // 2, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B * H * W, C)


@pytest.mark.parametrize("t", [32, 16])
def test_maxpool2x2_bwd(ops, L, t):
    """all three strides differ from C; the routing (ties, NaN) is F.max_pool2d's in float64; every dx element is written: bit-exact"""
    jobs = []
    for B, H, W, C in POOL_SHAPES:
        x = strided_nan(pool_bwd_input(B, H, W, C, C).to(dt(ops, t)), C + 3)
        dy = strided_nan(randn(B * (H // 2) * (W // 2), C, seed=C + 1), C + 5)
        jobs.append((x, dy, Canvas2(B * H * W, C, F32, C + 7, 1), (B, H, W, C)))
    reached(L, f"maxpool2x2_bwd_kernel<{tn(t)}>", "maxpool2x2_bwd", [
        lambda x=x, d=d, o=o, s=s: L.msam2_maxpool2x2_bwd(x.data_ptr(), int(t == 16), x.stride(0), d.data_ptr(), d.stride(0), o.view.data_ptr(), o.view.stride(0), *s,
                                                        stream()) for x, d, o, s in jobs])
    for x, d, o, s in jobs:
        B, H, W, C = s
        xg = nchw(x.double(), B, H, W).clone().requires_grad_(True)
        F.max_pool2d(xg, 2).backward(nchw(d.double(), B, H // 2, W // 2))
        same_bits(o.view, nhwc(xg.grad).float(), f"maxpool2x2_bwd {s}")
        assert o.sentinels_intact()


def test_sumpool2x2(ops, L):
    """multiples of 1/8: the four-term sums are exact in any order"""
    jobs = [(nan_guarded(randint(-40, 41, B * H * W, C, seed=C) / 8), Flat((B * (H // 2) * (W // 2), C), F32), (B, H, W, C)) for B, H, W, C in POOL_SHAPES]
    reached(L, "sumpool2x2_kernel", "sumpool2x2", [lambda d=d, o=o, s=s: L.msam2_sumpool2x2(d.data_ptr(), o.view.data_ptr(), *s, stream()) for d, o, s in jobs])
    for d, o, s in jobs:
        B, H, W, C = s
        same_bits(o.view, d.view(B, H // 2, 2, W // 2, 2, C).double().sum((2, 4)).reshape(-1, C).float(), f"sumpool2x2 {s}")
        assert o.sentinels_intact()


# =================================================================================================================================
# window partition / un-partition
WIN_SHAPES = [(1, 1, 1, 1, 8, 1), (2, 16, 20, 2, 56, 14), (1, 7, 9, 3, 8, 8), (2, 16, 16, 2, 24, 8)]


def windows_ref(img, B, H, W, heads, D, ws, fill):
    """window_partition of backbones/utils.py on [B*H*W, heads*D] rows -> [B*nW, heads, ws*ws, D]; padded tokens take fill (or zero)"""
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    buf = (torch.zeros(heads * D, dtype=img.dtype, device=DEV) if fill is None else fill).view(1, 1, 1, heads, D).expand(B, Hp, Wp, heads, D).clone()
    buf[:, :H, :W] = img.reshape(B, H, W, heads, D)
    return buf.view(B, Hp // ws, ws, Wp // ws, ws, heads, D).permute(0, 1, 3, 5, 2, 4, 6).reshape(B * (Hp // ws) * (Wp // ws), heads, ws * ws, D)


def img_slice(src, width):
    """src [rows, width] as a column slice (eight elements in) of a NaN-filled buffer of row length width + 16"""
    buf = torch.full((src.shape[0] + 2, width + 16), float("nan"), dtype=src.dtype, device=DEV)
    v = buf[1:1 + src.shape[0], 8:8 + width]
    v.copy_(src)
    return v


@pytest.mark.parametrize("es", [2, 4])
def test_window_move_round_trip(ops, L, es):
    """partition (fill present and absent) against the torch reference; un-partition of the result reproduces the image's bits"""
    t = ops.OP16 if es == 2 else F32
    part, unpart, checks = [], [], []
    for B, H, W, heads, D, ws in WIN_SHAPES:
        for with_fill in (False, True):
            s = (B, H, W, heads, D, ws)
            img = img_slice(randn(B * H * W, heads * D, seed=H + D).to(t), heads * D)
            fill = nan_guarded(randn(heads * D, seed=D).to(t)) if with_fill else None
            nw = B * (-(-H // ws)) * (-(-W // ws))
            win = Flat((nw, heads, ws * ws, D), t)
            back = Canvas2(B * H * W, heads * D, t, heads * D + 16, 8)
            part.append(lambda img=img, win=win, fill=fill, s=s: L.msam2_window_move(img.data_ptr(), img.stride(0), win.view.data_ptr(),
                                                                                     fill.data_ptr() if fill is not None else None, *s, es, 1, stream()))
            unpart.append(lambda back=back, win=win, s=s: L.msam2_window_move(back.view.data_ptr(), back.view.stride(0), win.view.data_ptr(), None, *s, es, 0, stream()))
            checks.append((img, fill, win, back, s))
    reached(L, "window_move_kernel<true,unsignedint>", "window_move_kernel", part)
    reached(L, "window_move_kernel<false,unsignedint>", "window_move_kernel", unpart)
    for img, fill, win, back, s in checks:
        same_bits(win.view, windows_ref(img, *s, fill), f"window partition {s} fill={fill is not None}")
        same_bits(back.view, img, f"window un-partition {s}")
        assert win.sentinels_intact() and back.sentinels_intact()


def test_window_unpartition_cvt(ops, L):
    """equals the fp32 un-partition followed by the cast, bit for bit"""
    jobs = []
    for s in WIN_SHAPES:
        B, H, W, heads, D, ws = s
        win = nan_guarded(windows_ref(randn(B * H * W, heads * D, seed=H + D), *s, None))
        jobs.append((win, Canvas2(B * H * W, heads * D, ops.OP16, heads * D + 16, 8), Canvas2(B * H * W, heads * D, F32, heads * D + 16, 8), s))
    reached(L, "window_unpartition_cvt_kernel", "window_unpartition_cvt", [
        lambda w=w, o=o, s=s: L.msam2_window_unpartition_cvt(o.view.data_ptr(), o.view.stride(0), w.data_ptr(), *s, stream()) for w, o, _, s in jobs])
    reached(L, "window_move_kernel<false,unsignedint>", "window_move_kernel", [
        lambda w=w, o=o, s=s: L.msam2_window_move(o.view.data_ptr(), o.view.stride(0), w.data_ptr(), None, *s, 4, 0, stream()) for w, _, o, s in jobs])
    for w, o16, o32, s in jobs:
        same_bits(o16.view, o32.view.to(ops.OP16), f"window_unpartition_cvt {s}")
        assert o16.sentinels_intact() and o32.sentinels_intact()


def test_window_pad_colsum(ops, L):
    """integer-valued windows: exact; added into a non-zero output; a shape without padding launches nothing and leaves the output alone"""
    jobs = []
    for s in WIN_SHAPES:
        B, H, W, heads, D, ws = s
        nw = B * (-(-H // ws)) * (-(-W // ws))
        win = nan_guarded(randint(-3, 4, nw, heads, ws * ws, D, seed=H + D))
        init = randint(-5, 6, heads * D, seed=D)
        jobs.append((win, init, flat_with(init), s))
    is_padded = lambda j: bool(j[3][1] % j[3][5] or j[3][2] % j[3][5])
    launch = lambda j: (lambda: L.msam2_window_pad_colsum(j[0].data_ptr(), j[2].view.data_ptr(), *j[3], stream()))
    assert sum(is_padded(j) for j in jobs) == 2
    reached(L, "window_pad_colsum_kernel", "window_pad_colsum", [launch(j) for j in jobs if is_padded(j)])
    reached(L, set(), "window_pad_colsum", [launch(j) for j in jobs if not is_padded(j)])
    for win, init, o, s in jobs:
        B, H, W, heads, D, ws = s
        inside = windows_ref(torch.ones(B * H * W, heads * D, device=DEV), *s, None)          # 1 on image tokens, 0 on padding
        ref = init.double() + (win.double() * (1 - inside.double())).sum((0, 2)).reshape(-1)
        same_bits(o.view, ref.float(), f"window_pad_colsum {s}")
        assert o.sentinels_intact()


# =================================================================================================================================
# position-embedding adjoint
POS_SHAPES = [(1, 1, 1, 8, 8, 8), (24, 7, 7, 56, 56, 8), (130, 8, 8, 16, 16, 8), (24, 14, 9, 14, 28, 7), (24, 16, 16, 32, 32, 8), (5, 14, 14, 7, 7, 1)]


@pytest.mark.parametrize("maxb", [8, 16])
def test_hiera_pos_embed_bwd(ops, L, maxb):
    """bw <= 8 runs hiera_pos_bwd_rows_kernel<8,8>, bw in 9..16 <16,8>; C = 130 gives threads a second channel trip; the workspace has exactly
    the size the library asks for and its tail stays intact; checked against float64 autograd of F.interpolate(bicubic) + tile"""
    jobs = []
    for s in [s for s in POS_SHAPES if (s[2] <= 8) == (maxb == 8)]:
        C, bh, bw, h, w, window = s
        nb = L.msam2_hiera_pos_embed_bwd_workspace_bytes(C, bw, h, window)
        assert nb == h * (bw + window) * C * 4
        jobs.append((nan_guarded(randn(h * w, C, seed=h + bw)), Flat((C, bh, bw), F32), Flat((C, window, window), F32), Flat((nb // 4,), F32), nb, s))
    reached(L, {f"hiera_pos_bwd_rows_kernel<{maxb},8>", "hiera_pos_bwd_final_kernel"}, "hiera_pos_bwd_", [
        lambda d=d, a=a, b=b, ws=ws, nb=nb, s=s: L.msam2_hiera_pos_embed_bwd(d.data_ptr(), a.view.data_ptr(), b.view.data_ptr(), *s, ws.view.data_ptr(), nb, stream())
        for d, a, b, ws, nb, s in jobs])
    for d, a, b, ws, nb, s in jobs:
        C, bh, bw, h, w, window = s
        refs, bounds = BB.hiera_pos_embed_bwd_bound(d.double(), *s)
        pe = torch.zeros(1, C, bh, bw, dtype=F64, device=DEV, requires_grad=True)
        pw = torch.zeros(1, C, window, window, dtype=F64, device=DEV, requires_grad=True)
        (F.interpolate(pe, size=(h, w), mode="bicubic") + pw.tile(1, 1, h // window, w // window))[0].permute(1, 2, 0).reshape(h * w, C).backward(d.double())
        assert float((refs[0] - pe.grad[0]).abs().max()) <= 1e-11 * float(refs[0].abs().max() + 1)
        assert float((refs[1] - pw.grad[0]).abs().max()) <= 1e-11 * float(refs[1].abs().max() + 1)
        within(a.view, refs[0], bounds[0], f"hiera_pos_embed_bwd {s}: d pos_embed")
        within(b.view, refs[1], bounds[1], f"hiera_pos_embed_bwd {s}: d pos_embed_window")
        assert a.sentinels_intact() and b.sentinels_intact() and ws.sentinels_intact(), f"hiera_pos_embed_bwd {s}: wrote outside an output or its workspace"


# =================================================================================================================================
# dropout, counter_bump
def dropout_run(ops, L, ti, to, p, with_res, *, seed=12345, offset=77, seed_dev=None, rows=5, cols=61, x=None):
    x = strided_nan((randn(rows, cols, seed=cols) * 2 if x is None else x).to(dt(ops, ti)), cols + 3)
    res = strided_nan(randn(rows, cols, seed=cols + 1), cols + 5) if with_res else None
    y = Canvas2(rows, cols, dt(ops, to), cols + 7, 1)
    launch = lambda: L.msam2_dropout(x.data_ptr(), int(ti == 16), x.stride(0), res.data_ptr() if with_res else None, res.stride(0) if with_res else 0, y.view.data_ptr(),
                                     int(to == 16), y.view.stride(0), rows, cols, p, seed, offset, seed_dev.data_ptr() if seed_dev is not None else None, stream())
    return x, res, y, launch


def keep_mask(seed, offset, rows, cols, p):
    idx = np.arange(rows * cols, dtype=np.uint64) + np.uint64(offset)
    return torch.from_numpy(BB.dropout_keep_np(seed, idx, BB.dropout_thr(p))).view(rows, cols).to(DEV)


@pytest.mark.parametrize("ti,to", ACT_TYPES)
def test_dropout(ops, L, ti, to):
    """strided x, residual and y; the mask is the numpy restatement of dropout_keep; p = 0 is bit-exact; the device seed agrees with the same
    value passed by `seed`"""
    runs = [(p, r, dropout_run(ops, L, ti, to, p, r)) for p in (0.0, 0.1, 0.999) for r in (False, True)]
    sd = torch.tensor([-1, 5000, -1], dtype=torch.int64, device=DEV)
    dev = dropout_run(ops, L, ti, to, 0.1, True, seed=12345 - 5000, seed_dev=sd[1:])
    reached(L, f"dropout_kernel<{tn(ti)},{tn(to)}>", "dropout_kernel", [r[2][3] for r in runs] + [dev[3]])
    for p, r, (x, res, y, _) in runs:
        keep = keep_mask(12345, 77, 5, 61, p)
        ref, bound = BB.dropout_bound(x.double(), keep, p, res.double() if r else None, to == 16, op16_is_fp16())
        within(y.view, ref, bound, f"dropout {tn(ti)}->{tn(to)} p={p} residual={r}")
        if p == 0.0:
            same_bits(y.view, ((x.float() + res) if r else x.float()).to(dt(ops, to)), "dropout p = 0")
        if p == 0.1:
            assert 0 < int((~keep).sum()) < keep.numel() // 2
        assert y.sentinels_intact()
    same_bits(dev[2].view, runs[3][2][2].view, "dropout: seed_dev + seed against the same value passed by seed")
    assert sd.tolist() == [-1, 5000, -1] and dev[2].sentinels_intact()


def test_dropout_saturates(ops, L):
    """x = +-65504 at p = 0.1: x / 0.9 exceeds the fp16 range; the fp16 build stores +-65504 like every other 16-bit store of the library,
    never inf (bf16: finite and within the bound)"""
    x = torch.full((5, 61), 65504.0, device=DEV)
    x[::2] = -65504.0
    for ti in (32, 16):
        xi, _, y, launch = dropout_run(ops, L, ti, 16, 0.1, False, x=x)
        reached(L, f"dropout_kernel<{tn(ti)},T16>", "dropout_kernel", [launch])
        keep = keep_mask(12345, 77, 5, 61, 0.1)
        assert bool(torch.isfinite(y.view.float()).all()), "dropout stored inf"
        ref, bound = BB.dropout_bound(xi.double(), keep, 0.1, None, True, op16_is_fp16())
        within(y.view, ref, bound, "dropout at the fp16 maximum")
        if op16_is_fp16():
            assert bool((y.view.float()[keep].abs() == 65504.0).all())
        assert y.sentinels_intact()


def test_counter_bump(ops, L):
    buf = torch.tensor([-1, 41, -1, 0, -1], dtype=torch.int64, device=DEV)
    reached(L, "counter_bump_kernel", "counter_bump", [lambda: L.msam2_counter_bump(buf[1:].data_ptr(), buf[3:].data_ptr(), stream())] * 2
            + [lambda: L.msam2_counter_bump(buf[1:].data_ptr(), None, stream())])
    assert buf.tolist() == [-1, 44, -1, 43, -1]
    assert L.msam2_counter_bump(buf[1:].data_ptr(), buf[3:].data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert buf.tolist() == [-1, 45, -1, 45, -1]


# =================================================================================================================================
# every kernel instantiation the matrix is meant to reach, as a literal list: the tables above must name each of them
T2 = ("float", "T16")
LISTED = sorted(
    ["transpose16_kernel"] + [f"colsum_kernel<{t}>" for t in T2]
    + [f"act_bwd{v}_kernel<{a},{b}>" for v in ("", "_vec") for a in T2 for b in T2]
    + [f"layernorm_bwd_kernel<{t},{n}>" for t in T2 for n in (1, 2, 4, 6, 8, 12, 16)]
    + [f"layernorm_bwd_vec_kernel<{t},{c}>" for t in T2 for c in (1, 2, 3, 4, 6)]
    + ["softmax_rows_kernel", "softmax_bwd_rows_kernel", "convt2x2_gather_kernel"] + [f"convt2x2_scatter_grad_kernel<{t}>" for t in T2]
    + ["dwconv7x7_kernel", "dwconv7x7_wgrad_kernel", "col2im3x3s2_kernel", "bilinear_bwd_kernel", "bce_logits_kernel", "adam_step_kernel", "adam_tick_kernel",
       "adam_multi_kernel"]
    + [f"maxpool2x2_bwd_kernel<{t}>" for t in T2]
    + ["window_move_kernel<true,unsignedint>", "window_move_kernel<false,unsignedint>", "window_unpartition_cvt_kernel", "window_pad_colsum_kernel",
       "sumpool2x2_kernel", "hiera_pos_bwd_rows_kernel<8,8>", "hiera_pos_bwd_rows_kernel<16,8>", "hiera_pos_bwd_final_kernel"]
    + [f"dropout_kernel<{a},{b}>" for a in T2 for b in T2] + ["counter_bump_kernel"])

# instantiations the library holds that no test can reach, with the reason
NOT_REACHED = {
    "window_move_kernel<true,long>": "taken from 2^32 - 2^22 sixteen-byte chunks on: a 64 GiB volume",
    "window_move_kernel<false,long>": "taken from 2^32 - 2^22 sixteen-byte chunks on: a 64 GiB volume",
}


def expected_keys():
    """the union of the expected kernels of every case table of this file"""
    keys = {f"layernorm_bwd_kernel<{tn(td)},{ni}>" for td, ni in LNB_SCALAR_CASES} | {f"layernorm_bwd_vec_kernel<{tn(td)},{ch}>" for td, ch in LNB_VEC_CASES}
    keys |= {f"act_bwd{v}_kernel<{tn(a)},{tn(b)}>" for v in ("", "_vec") for a, b in ACT_TYPES}
    keys |= {f"{k}<{tn(t)}>" for k in ("colsum_kernel", "convt2x2_scatter_grad_kernel", "maxpool2x2_bwd_kernel") for t in (32, 16)}
    keys |= {f"dropout_kernel<{tn(a)},{tn(b)}>" for a, b in ACT_TYPES}
    keys |= {f"hiera_pos_bwd_rows_kernel<{8 if s[2] <= 8 else 16},8>" for s in POS_SHAPES} | {"hiera_pos_bwd_final_kernel"}
    keys |= {"window_move_kernel<true,unsignedint>", "window_move_kernel<false,unsignedint>", "window_unpartition_cvt_kernel", "window_pad_colsum_kernel"}
    keys |= {"transpose16_kernel", "softmax_rows_kernel", "softmax_bwd_rows_kernel", "convt2x2_gather_kernel", "dwconv7x7_kernel", "dwconv7x7_wgrad_kernel",
             "col2im3x3s2_kernel", "bilinear_bwd_kernel", "bce_logits_kernel", "adam_step_kernel", "adam_tick_kernel", "adam_multi_kernel", "sumpool2x2_kernel",
             "counter_bump_kernel"}
    return keys


EXPECTED = sorted(expected_keys())


def test_every_listed_instantiation_has_a_case(ops):
    assert EXPECTED == LISTED and len(LISTED) == 63
    assert len({K(k) for k in LISTED}) == len(LISTED)
    assert not set(NOT_REACHED) & set(LISTED)
