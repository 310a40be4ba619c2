"""The bounds of tests/backward_bounds.py are neither wrong nor slack (CPU): per kernel family, at shapes of the GPU matrix
(tests/test_backward_variants_gpu.py), fp32 torch evaluations in two OTHER operation orders than the float64 reference lie within the bound at
every element; a fixed list of mutants -- each a mistake a real kernel makes -- lies outside it at some element.  If a mutant survives, the
bound or the data is too weak: that is what gets fixed, never the list.  Also here: GELU_CDF_ABS is MEASURED from the coefficients of
csrc/common.h against math.erf (the reference, not the kernel)."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backward_bounds as BB  # noqa: E402
import pointwise_bounds as PB  # noqa: E402
from helpers import ROOT, kernel_key  # noqa: E402

F32, F64 = torch.float32, torch.float64
T16 = [(torch.float16, True), (torch.bfloat16, False)]


def randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def inside(got, ref, bound):
    return bool(((got.double() - ref).abs() <= bound).all())


def assert_inside(got, ref, bound, what):
    d = (got.double() - ref).abs()
    assert bool((d <= bound).all()), f"{what}: an fp32 evaluation is {float((d / bound.clamp(min=1e-300)).max()):.2f} x the bound somewhere"


def assert_outside(got, ref, bound, what):
    assert not inside(got, ref, bound), f"mutant survived: {what}"


def test_kernel_key_on_the_backward_names():
    cases = {
        "_Z18window_move_kernelILb1EjEvPhlS0_PKhiiiiiiii": "window_move_kernel<true,unsignedint>",
        "void window_move_kernel<true, unsigned int>(unsigned char*, long, unsigned char*)": "window_move_kernel<true,unsignedint>",
        "_Z18window_move_kernelILb0ElEvPhlS0_PKhiiiiiiii": "window_move_kernel<false,long>",
        "void window_move_kernel<false, long>(unsigned char*, long)": "window_move_kernel<false,long>",
        "_Z25hiera_pos_bwd_rows_kernelILi16ELi8EEvPKfPfiiii": "hiera_pos_bwd_rows_kernel<16,8>",
        "void hiera_pos_bwd_rows_kernel<8, 8>(float const*, float*, int, int, int, int)": "hiera_pos_bwd_rows_kernel<8,8>",
        "_Z14dropout_kernelIfDF16_EvPKT_lPKflPT0_llljfmmPKm": "dropout_kernel<float,_Float16>",
        "_Z14act_bwd_kernelIDF16bfEvPKT_PKT0_PDF16bli": "act_bwd_kernel<__bf16,float>",
        "void layernorm_bwd_vec_kernel<_Float16, 6>(float const*, long)": "layernorm_bwd_vec_kernel<_Float16,6>",
        "_Z24layernorm_bwd_vec_kernelIDF16bLi6EEvPKfl": "layernorm_bwd_vec_kernel<__bf16,6>",
        "_Z18transpose16_kernelPKDF16_lPS_lii": "transpose16_kernel",
    }
    for name, key in cases.items():
        assert kernel_key(name) == key, name


# ---------------------------------------------------------------------------------------------------------------------------------
# GELU': the polynomial Phi of csrc/common.h against math.erf
def gelu_coefficients():
    src = open(os.path.join(ROOT, "medical-sam2_amd", "csrc", "common.h")).read()
    q = [float(re.search(rf"#define MSAM2_GELU_Q{i} (\S+?)f\n", src).group(1)) for i in range(9)]
    xmax = float(re.search(r"#define MSAM2_GELU_X (\S+?)f\n", src).group(1))
    return q, xmax


def test_gelu_cdf_abs_is_the_measured_error_of_the_polynomial():
    q, xmax = gelu_coefficients()
    x = np.concatenate([np.linspace(-10.0, 10.0, 1_000_001), np.array([0.443, -0.443, 4.5, -4.5, 0.0])])
    phi = 0.5 * (1.0 + np.vectorize(math.erf)(x / math.sqrt(2.0)))
    # float64, exactly those coefficients (as fp32 values)
    q32 = [np.float32(c) for c in q]
    xc = np.clip(x, -xmax, xmax)
    u = xc * xc
    acc = np.float64(q32[8]) * u + np.float64(q32[7])
    for c in q32[6::-1]:
        acc = acc * u + np.float64(c)
    err64 = float(np.abs(xc * acc + 0.5 - phi).max())
    # the kernel's fp32 fma chain: every fma = the float64 operation rounded once to fp32 (products of two fp32 values are exact in float64;
    # the sum's double rounding moves a result by far less than the 5 % this test allows)
    x32 = x.astype(np.float32)
    xc32 = np.clip(x32, np.float32(-xmax), np.float32(xmax))
    u32 = (xc32 * xc32).astype(np.float32)
    fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + np.float64(c)).astype(np.float32)
    a32 = fma(u32, np.full_like(u32, q32[8]), q32[7])
    for c in q32[6::-1]:
        a32 = fma(a32, u32, c)
    cdf32 = fma(xc32, a32, np.float32(0.5))
    phi32 = 0.5 * (1.0 + np.vectorize(math.erf)(x32.astype(np.float64) / math.sqrt(2.0)))
    err32 = float(np.abs(cdf32.astype(np.float64) - phi32).max())
    measured = max(err64, err32)
    print(f"max |Phi_poly - Phi|: float64 {err64:.4e}, fp32 {err32:.4e}; GELU_CDF_ABS {BB.GELU_CDF_ABS:.4e}")
    assert measured <= BB.GELU_CDF_ABS <= 1.05 * measured
    assert measured > 5e-5, "the polynomial is NOT within 1e-5 of Phi (what the kernel's comment said)"
    i = int(np.abs(xc * acc + 0.5 - phi).argmax())
    assert abs(abs(x[i]) - 0.443) < 0.01


def act_samples():
    x = torch.cat([torch.linspace(-6, 6, 2049), torch.tensor([0.443, -0.443, 4.5, -4.5, 0.0, 10.0, -10.0])])
    dy = randn(x.numel(), seed=5) * 3
    dy[::97] = 65504.0
    dy[1::97] = -65504.0
    return x, dy


def gelu_grad32(x, order):
    if order == 0:
        return 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0)))) + x * torch.exp(-0.5 * x * x) * BB.INV_SQRT_2PI
    return 0.5 + (0.5 * torch.erf(x / math.sqrt(2.0)) + (x * BB.INV_SQRT_2PI) * torch.exp2(x * x * -0.72134752044448170368))


def poly_cdf32(x):
    q, xmax = gelu_coefficients()
    xc = x.clamp(-xmax, xmax)
    u = xc * xc
    acc = torch.full_like(x, q[8]) * u + q[7]
    for c in q[6::-1]:
        acc = acc * u + c
    return xc * acc + 0.5


def test_act_bwd_bound_and_mutants():
    x, dy = act_samples()
    for tp in (F32, torch.float16, torch.bfloat16):
        xr, gr = x.to(tp).float(), dy.to(tp).float()
        for t16, fp16 in T16:
            for poly in (False, True):
                ref, bound = BB.act_bwd_bound(xr.double(), gr.double(), 1, poly, fp16)
                sat = (lambda v: v.clamp(-65504, 65504)) if fp16 else (lambda v: v)
                for order in (0, 1):
                    assert_inside(sat(gr * gelu_grad32(xr, order)).to(t16), ref, bound, f"gelu' order {order} poly={poly} {tp}->{t16}")
                if poly:
                    d = poly_cdf32(xr) + xr * BB.INV_SQRT_2PI * torch.exp(-0.5 * xr * xr)
                    assert_inside(sat(gr * d).to(t16), ref, bound, f"gelu' polynomial form {tp}->{t16}")
            ref, bound = BB.act_bwd_bound(xr.double(), gr.double(), 2, True, fp16)
            assert_inside(sat(gr * (xr > 0).float()).to(t16), ref, bound, "relu'")
            assert_inside(sat(torch.where(xr > 0, gr, torch.zeros_like(gr))).to(t16), ref, bound, "relu' as a select")
            assert_outside(sat(gr * (xr >= 0).float()).to(t16), ref, bound, "relu' with >= instead of >")
    x64, g64 = x.double(), dy.double()
    small = dy.abs() < 100                                   # (the saturated samples hide nothing: the mutants must show on ordinary dy too)
    for fp16 in (True, False):
        ref, bound = BB.act_bwd_bound(x64, g64, 1, True, fp16)
        assert_outside((g64 * BB.phi64(x64))[small], ref[small], bound[small], "gelu': the x phi(x) term missing")
        assert_outside((g64 * (BB.phi64(x64) + x64 * 0.5 * torch.exp(-0.5 * x64 * x64)))[small], ref[small], bound[small], "gelu': phi with the wrong constant")
        xt = x64.detach().clone().requires_grad_(True)
        F.gelu(xt, approximate="tanh").sum().backward()
        assert_outside((g64 * xt.grad)[small], ref[small], bound[small], "gelu': tanh form")
    # the two forms of the entry: what test_act_bwd_forms_agree allows is no tighter than the two bounds together and a 1e-5 comment would fail
    d_poly = (poly_cdf32(x) - BB.phi64(x.double()).float()).abs().max()
    assert 6e-5 < float(d_poly) <= BB.GELU_CDF_ABS


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm backward
def lnb_rows(rows, C, seed):
    x = randn(rows, C, seed=seed) * (0.5 + (torch.arange(rows) % 4).float())[:, None] + 2.0 * ((torch.arange(rows) % 3).float() - 1)[:, None]
    if rows > 2:
        x[1] = 1000.0 + randn(C, seed=seed + 1)
    if rows > 1:
        x[rows - 1] = 2.0
    gamma = (1.0 + 0.5 * randn(C, seed=seed + 2)) * torch.where(torch.arange(C) % 3 == 0, -1.0, 1.0)
    dy = randn(rows, C, seed=seed + 3) * (0.25 + (torch.arange(rows) % 5).float())[:, None]
    add = randn(rows, C, seed=seed + 4)
    return x, gamma, dy, add, randn(C, seed=seed + 5), randn(C, seed=seed + 6)


def lnb32(x, dy, gamma, eps, add, g0, b0, order=0, *, no_m2=False, use_eps=True, c_div=None, dgamma_from_g=False, drop_last=False, no_add=False):
    """fp32 LayerNorm backward; order 1 sums from the other end and arranges dx as rstd / C * (C g - sum g - xhat sum(g xhat))"""
    C = x.shape[-1]
    fl = (lambda t: t.flip(-1)) if order else (lambda t: t)
    n = c_div or C
    mean = fl(x).sum(-1, keepdim=True) / n
    var = fl((x - mean) ** 2).sum(-1, keepdim=True) / n
    rstd = 1.0 / torch.sqrt(var + (eps if use_eps else 0.0))
    xh = (x - mean) * rstd
    g = dy * gamma
    s1, s2 = fl(g).sum(-1, keepdim=True), fl(g * xh).sum(-1, keepdim=True)
    if no_m2:
        s2 = s2 * 0
    dx = (rstd / n) * (n * g - s1 - xh * s2) if order else rstd * (g - s1 / n - xh * (s2 / n))
    if drop_last:
        dx = torch.cat([dx[:, :-1], torch.zeros_like(dx[:, -1:])], 1)
    if not no_add and add is not None:
        dx = dx + add
    src = g if dgamma_from_g else dy
    rf = (lambda t: t.flip(0)) if order else (lambda t: t)
    return dx, g0 + rf(src * xh).sum(0), b0 + rf(dy).sum(0)


LNB_C = [1, 4, 63, 64, 68, 127, 128, 260, 320, 384, 385, 513, 1024]


@pytest.mark.parametrize("C", LNB_C)
def test_layernorm_bwd_bound(C):
    for rows in (1, 17, 33):
        x, gamma, dy, add, g0, b0 = lnb_rows(rows, C, C + rows)
        for td in (F32, torch.float16, torch.bfloat16):
            dyr = dy.to(td).float()
            for a in (None, add):
                refs, bounds = BB.layernorm_bwd_bound(x.double(), dyr.double(), gamma.double(), 1e-6, None if a is None else a.double(), g0.double(), b0.double())
                for order in (0, 1):
                    got = lnb32(x, dyr, gamma, 1e-6, a, g0, b0, order)
                    for name, gt, r, b in zip(("dx", "dgamma", "dbeta"), got, refs, bounds):
                        assert_inside(gt, r, b, f"layernorm_bwd {name} C={C} rows={rows} dy={td} add={a is not None} order={order}")


def test_layernorm_bwd_mutants():
    for C, rows in ((4, 17), (68, 17), (100, 33)):
        x, gamma, dy, add, g0, b0 = lnb_rows(rows, C, C + rows)
        a64 = [t.double() for t in (x, dy, gamma)]
        refs, bounds = BB.layernorm_bwd_bound(a64[0], a64[1], a64[2], 1e-6, add.double(), g0.double(), b0.double())
        run = lambda **kw: lnb32(a64[0], a64[1], a64[2], 1e-6, add.double(), g0.double(), b0.double(), 0, **kw)
        assert_outside(run(no_m2=True)[0], refs[0], bounds[0], f"m2 missing (C={C})")
        # rstd without eps shows on the row whose variance is comparable with eps
        xs = x.clone()
        xs[0] = 1e-3 * randn(C, seed=9)
        r2, b2 = BB.layernorm_bwd_bound(xs.double(), a64[1], a64[2], 1e-6, add.double(), g0.double(), b0.double())
        assert_outside(lnb32(xs.double(), a64[1], a64[2], 1e-6, add.double(), g0.double(), b0.double(), 0, use_eps=False)[0][:1], r2[0][:1], b2[0][:1],
                       f"rstd without eps (C={C})")
        if C % 64:
            assert_outside(run(c_div=-(-C // 64) * 64)[0], refs[0], bounds[0], f"mean over NI * 64 instead of C (C={C})")
        assert_outside(run(dgamma_from_g=True)[1], refs[1], bounds[1], f"dgamma from g instead of dy (C={C})")
        assert_outside(run(drop_last=True)[0], refs[0], bounds[0], f"last column dropped (C={C})")
        assert_outside(run(no_add=True)[0], refs[0], bounds[0], f"residual add dropped (C={C})")
        z = torch.zeros(C, dtype=F64)
        assert_outside(lnb32(a64[0], a64[1], a64[2], 1e-6, add.double(), z, z, 0)[1], refs[1], bounds[1], "dgamma zeroed instead of accumulated")
        assert_outside(lnb32(a64[0], a64[1], a64[2], 1e-6, add.double(), z, z, 0)[2], refs[2], bounds[2], "dbeta zeroed instead of accumulated")


# ---------------------------------------------------------------------------------------------------------------------------------
# softmax rows
def softmax_data(rows, cols, seed):
    s = randn(rows, cols, seed=seed) * 3
    if cols > 1:
        s[0] = torch.linspace(40.0, 100.0, cols)             # a spread of 60 far from zero: exp overflows without the max subtraction
    if rows > 1:
        s[rows - 1] = 0.7                                    # equal logits
    return s


@pytest.mark.parametrize("cols", [1, 63, 64, 65, 200])
def test_softmax_bounds_and_mutants(cols):
    for rows in (1, 3, 5):
        s = softmax_data(rows, cols, cols + rows)
        for scale in (0.125, 1.0):
            for t16, fp16 in T16:
                ref, bound = BB.softmax_rows_bound(s.double(), scale, fp16)
                assert_inside(torch.softmax(s * scale, -1).to(t16), ref, bound, f"softmax cols={cols} scale={scale}")
                m = s.max(-1, keepdim=True).values
                e = torch.exp2((s - m) * (scale * BB.LOG2E))
                assert_inside((e / e.flip(-1).sum(-1, keepdim=True)).to(t16), ref, bound, f"softmax exp2 form cols={cols} scale={scale}")
                if cols > 1 and scale == 1.0:
                    e = torch.exp(s * scale)
                    assert_outside((e / e.sum(-1, keepdim=True))[:1].to(t16), ref[:1], bound[:1], "softmax without the max subtraction on the spread-60 row")
                p = torch.softmax(s.double() * scale, -1).to(t16)
                dp = randn(rows, cols, seed=cols + 50) * 2
                ref, bound = BB.softmax_bwd_rows_bound(p.double(), dp.double(), scale, fp16)
                pf = p.float()
                acc = (pf * dp).sum(-1, keepdim=True)
                assert_inside((scale * pf * (dp - acc)).to(t16), ref, bound, f"softmax_bwd cols={cols}")
                acc = (pf * dp).flip(-1).sum(-1, keepdim=True)
                assert_inside((pf * scale * dp - pf * scale * acc).to(t16), ref, bound, f"softmax_bwd order 2 cols={cols}")
                if scale != 1.0 and cols > 1:
                    assert_outside((pf * (dp - acc)).to(t16), ref, bound, "softmax_bwd without scale")
                    assert_outside((scale * pf * dp).to(t16), ref, bound, "softmax_bwd without the sum term")


# ---------------------------------------------------------------------------------------------------------------------------------
# convolution tails
def test_convt_gather_bound():
    B, h, w, C = 2, 3, 5, 7
    for t16, _ in T16:
        g, bias, skip = randn(B * h * w, 4 * C, seed=1).to(t16).float(), randn(C, seed=2), randn(B * 4 * h * w, C, seed=3).to(t16).float()
        ref, bound = BB.convt2x2_gather_bound(g.double(), bias.double(), skip.double(), B, h, w)
        gs = BB.convt_sub(g, B, h, w, C)
        assert_inside(gs + bias + skip, ref, bound, "convt gather")
        assert_inside(skip + (bias + gs), ref, bound, "convt gather order 2")
        assert_outside(BB.convt_sub(g.view(B, h, w, 2, 2, C).transpose(3, 4).reshape(B * h * w, 4 * C), B, h, w, C) + bias + skip, ref, bound, "sub-block transposed")
        assert bool((BB.convt_unsub(gs, B, h, w, C) == g).all())


@pytest.mark.parametrize("H,W", [(1, 1), (2, 5), (7, 7), (9, 13)])
def test_dwconv_bounds_and_mutants(H, W):
    B, C = 2, 8
    x, w, bias, dy = randn(B, C, H, W, seed=1), randn(49, C, seed=2), randn(C, seed=3), randn(B, C, H, W, seed=4)
    for flip in (0, 1):
        ref, bound = BB.dwconv7x7_bound(x.double(), w.double(), bias.double(), flip)
        k = BB.dw_taps(w).flip(2, 3) if flip else BB.dw_taps(w)
        assert_inside(F.conv2d(x, k, bias, padding=3, groups=C), ref, bound, f"dwconv flip={flip}")
        assert_inside(F.conv2d(x.flip(2, 3), k.flip(2, 3), bias, padding=3, groups=C).flip(2, 3), ref, bound, f"dwconv flip={flip} from the other corner")
        if H * W > 1:
            assert_outside(F.conv2d(x.double(), BB.dw_taps(w.double()) if flip else BB.dw_taps(w.double()).flip(2, 3), bias.double(), padding=3, groups=C),
                           ref, bound, f"dwconv with the wrong flip ({flip})")
    # the flipped correlation without a bias IS the input gradient of the forward convolution
    xg = x.double().requires_grad_(True)
    F.conv2d(xg, BB.dw_taps(w.double()), None, padding=3, groups=C).backward(dy.double())
    ref, _ = BB.dwconv7x7_bound(dy.double(), w.double(), None, 1)
    assert float((ref - xg.grad).abs().max()) < 1e-12
    # weight gradient
    dw0 = randn(49, C, seed=5)
    ref, bound = BB.dwconv7x7_wgrad_bound(x.double(), dy.double(), dw0.double())
    wg = BB.dw_taps(w.double()).requires_grad_(True)
    F.conv2d(x.double(), wg, None, padding=3, groups=C).backward(dy.double())
    assert float((ref - dw0.double() - wg.grad.reshape(C, 49).t()).abs().max()) < 1e-12
    w32 = BB.dw_taps(w).requires_grad_(True)
    F.conv2d(x, w32, None, padding=3, groups=C).backward(dy)
    assert_inside(dw0 + w32.grad.reshape(C, 49).t(), ref, bound, "dwconv wgrad")
    got = BB.dwconv7x7_wgrad_bound(x.flip(0), dy.flip(0), dw0)[0]
    assert_inside(got, ref, bound, "dwconv wgrad, batches in the other order")
    assert_outside(w32.grad.reshape(C, 49).t().double(), ref, bound, "dwconv wgrad overwrites instead of adding")


@pytest.mark.parametrize("C", [1, 63, 65])
def test_col2im_bound(C):
    B, H, W = 2, 4, 6
    dcols = randn(B * (H // 2) * (W // 2), 9 * C, seed=C)
    ref, bound = BB.col2im3x3s2_bound(dcols.double(), B, H, W, C)
    x = randn(B, C, H, W, seed=1).double().requires_grad_(True)
    cols = F.unfold(x, 3, padding=1, stride=2)               # [B, C*9, L], rows (c, ky, kx)
    cols = cols.view(B, C, 9, -1).permute(0, 3, 2, 1).reshape(-1, 9 * C)
    cols.backward(dcols.double())
    assert float((ref - x.grad.permute(0, 2, 3, 1).reshape(-1, C)).abs().max()) < 1e-12
    assert_inside(BB.col2im3x3s2_bound(dcols, B, H, W, C)[0], ref, bound, "col2im fp32")
    assert_outside(BB.col2im3x3s2_bound(dcols.double().roll(C, 1), B, H, W, C)[0], ref, bound, "col2im one tap off")


# ---------------------------------------------------------------------------------------------------------------------------------
# resize adjoints
BIL_SHAPES = [(1, 1, 1, 1), (1, 1, 5, 3), (7, 5, 7, 5), (3, 4, 10, 9), (16, 24, 50, 97), (5, 5, 20, 20)]


def bil_adjoint32(g, h, w, align=False, clamp=True):
    """fp32 adjoint of the bilinear resize with fp32 coordinates (scale = fl(h / H)); the keyword arguments are the mutants"""
    P, H, W = g.shape

    def mat(n_out, n_src):
        o = torch.arange(n_out, dtype=F32)
        if align:
            f = o * ((n_src - 1) / max(n_out - 1, 1))
        else:
            f = (o + 0.5) * torch.tensor(n_src / n_out, dtype=F32) - 0.5
            if clamp:
                f = f.clamp(min=0)
        i0 = f.floor()
        l = f - i0
        M = torch.zeros(n_out, n_src, dtype=F32)
        i0l = i0.long()
        ok0 = (i0l >= 0) & (i0l < n_src) if not clamp else torch.ones_like(i0l, dtype=torch.bool)
        M.scatter_add_(1, i0l.clamp(0, n_src - 1).view(-1, 1), ((1 - l) * ok0).view(-1, 1))
        i1 = i0l + 1
        ok1 = (i1 < n_src) if not clamp else torch.ones_like(i1, dtype=torch.bool)
        M.scatter_add_(1, i1.clamp(0, n_src - 1).view(-1, 1), (l * ok1).view(-1, 1))
        return M
    return torch.einsum("Yy,pYX,Xx->pyx", mat(H, h), g, mat(W, w)), torch.einsum("Xx,pYX,Yy->pyx", mat(W, w), g, mat(H, h))


@pytest.mark.parametrize("h,w,H,W", BIL_SHAPES)
def test_bilinear_bwd_bound_and_mutants(h, w, H, W):
    for P in (1, 3):
        g = randn(P, H, W, seed=h + W)
        ref, bound = BB.bilinear_bwd_bound(g.double(), h, w)
        x = randn(P, h, w, seed=1).double().requires_grad_(True)
        PB.bilinear_ref(x, H, W)[0].backward(g.double())
        assert float((ref - x.grad).abs().max()) < 1e-12, "the matrices are pointwise_bounds.bilinear_ref's own weights"
        x2 = x.detach().clone().requires_grad_(True)
        F.interpolate(x2[None], size=(H, W), mode="bilinear", align_corners=False)[0].backward(g.double())
        assert float((ref - x2.grad).abs().max()) < 1e-12
        for got in bil_adjoint32(g, h, w):
            assert_inside(got, ref, bound, f"bilinear adjoint {(h, w, H, W)}")
        if (H, W) != (h, w) and h > 1:
            assert_outside(bil_adjoint32(g, h, w, align=True)[0], ref, bound, "bilinear adjoint with align_corners weights")
        if H > h and h > 1:
            assert_outside(bil_adjoint32(g, h, w, clamp=False)[0], ref, bound, "bilinear adjoint without the border clamp")


POS_SHAPES = [(1, 1, 1, 8, 8, 8), (24, 7, 7, 56, 56, 8), (130, 8, 8, 16, 16, 8), (24, 14, 9, 14, 28, 7), (24, 16, 16, 32, 32, 8), (5, 14, 14, 7, 7, 1)]


def pos_autograd(d_table, C, bh, bw, h, w, window, dtype):
    pe = torch.zeros(1, C, bh, bw, dtype=dtype, requires_grad=True)
    pw = torch.zeros(1, C, window, window, dtype=dtype, requires_grad=True)
    t = F.interpolate(pe, size=(h, w), mode="bicubic") + pw.tile(1, 1, h // window, w // window)
    t[0].permute(1, 2, 0).reshape(h * w, C).backward(d_table.to(dtype))
    return pe.grad[0], pw.grad[0]


@pytest.mark.parametrize("C,bh,bw,h,w,window", POS_SHAPES)
def test_hiera_pos_embed_bwd_bound_and_mutants(C, bh, bw, h, w, window):
    C = min(C, 6)                                            # (the channel count changes nothing per channel; the GPU test runs the full widths)
    d = randn(h * w, C, seed=h + bw)
    refs, bounds = BB.hiera_pos_embed_bwd_bound(d.double(), C, bh, bw, h, w, window)
    a64 = pos_autograd(d, C, bh, bw, h, w, window, F64)
    for r, a in zip(refs, a64):
        assert float((r - a).abs().max()) < 1e-11, "the matrices are F.interpolate(bicubic)'s own weights"
    a32 = pos_autograd(d, C, bh, bw, h, w, window, F32)
    flipped = pos_autograd(d.view(h, w, C).flip(0, 1).reshape(h * w, C), C, bh, bw, h, w, window, F32)
    for r, b, a, f in zip(refs, bounds, a32, flipped):
        assert_inside(a, r, b, f"pos_embed adjoint {(bh, bw, h, w, window)}")
        assert_inside(f.flip(1, 2), r, b, f"pos_embed adjoint from the other corner {(bh, bw, h, w, window)}")
    if (bh, bw) != (h, w) and bh > 1:
        m = BB.hiera_pos_embed_bwd_bound(d.double(), C, bh, bw, h, w, window, A=-0.5)[0][0]
        assert_outside(m, refs[0], bounds[0], "bicubic adjoint with A = -0.5")


# ---------------------------------------------------------------------------------------------------------------------------------
# loss and optimiser
def bce_data(n, seed):
    x = randn(n, seed=seed) * 4
    y = torch.tensor([0.0, 1.0, 0.3])[torch.arange(n) % 3]
    for i, v in enumerate((100.0, -100.0, 0.0, 100.0, -100.0, 0.0)):
        if i < n:
            x[i] = v
    return x, y


@pytest.mark.parametrize("n", [1, 63, 257, 4099])
def test_bce_bound_and_mutants(n):
    x, y = bce_data(n, n)
    for pw in (1.0, 2.5):
        refs, bounds = BB.bce_logits_bound(x.double(), y.double(), pw, 0.75)
        l = F.binary_cross_entropy_with_logits(x, y, pos_weight=torch.tensor(pw), reduction="none")
        xg = x.clone().requires_grad_(True)
        F.binary_cross_entropy_with_logits(xg, y, pos_weight=torch.tensor(pw)).backward()
        assert_inside(0.75 + l.sum() / n, refs[0], bounds[0], f"bce loss n={n} pw={pw}")
        assert_inside(0.75 + l.flip(0).mean(), refs[0], bounds[0], f"bce loss from the other end n={n} pw={pw}")
        assert_inside(xg.grad, refs[1], bounds[1], f"bce gradient n={n} pw={pw}")
        s = torch.sigmoid(x)
        assert_inside(((pw * y + 1 - y) * s - pw * y) / n, refs[1], bounds[1], f"bce gradient order 2 n={n} pw={pw}")
        if pw != 1.0 and n > 2:
            x64, y64 = x.double(), y.double()
            sp = F.softplus(x64)
            assert_outside(0.75 + (y64 * (sp - x64) + pw * (1 - y64) * sp).mean(), refs[0], bounds[0], "bce: pos_weight on the wrong term (loss)")
            s64 = torch.sigmoid(x64)
            assert_outside((y64 * (s64 - 1) + pw * (1 - y64) * s64) / n, refs[1], bounds[1], "bce: pos_weight on the wrong term (gradient)")
        assert_outside(l.double().sum() / n, refs[0], bounds[0], "bce loss overwrites instead of adding")


def adam32(p, g, m, v, lr, b1, b2, eps, step, gscale, wd, order=0, *, no_bc=False, eps_inside=False):
    t = lambda s: torch.tensor(s, dtype=p.dtype)
    gi = g * gscale
    if order == 0:
        m2, v2 = b1 * m + (1 - b1) * gi, b2 * v + (1 - b2) * gi * gi
    else:
        m2, v2 = torch.lerp(gi, m, t(b1)), torch.addcmul(b2 * v, gi, gi, value=1 - b2)
    bc1, bc2 = (1.0, 1.0) if no_bc else (1 - b1 ** step, 1 - b2 ** step)
    if eps_inside:
        den = torch.sqrt(v2 / bc2 + eps)
    else:
        den = torch.sqrt(v2 / bc2) + eps if order == 0 else torch.sqrt(v2) / math.sqrt(bc2) + eps
    upd = lr * (m2 / bc1) / den if order == 0 else (lr / bc1) * m2 / den
    return p * (1 - lr * wd) - upd, m2, v2


@pytest.mark.parametrize("step", [1, 1000])
def test_adam_bound_and_mutants(step):
    n = 257
    p, g, m, v = randn(n, seed=1), randn(n, seed=2) * 0.1, randn(n, seed=3) * 0.05, (randn(n, seed=4) * 0.03) ** 2
    g[0], m[0], v[0] = 0.0, 0.0, 0.0
    g[1], v[1] = 1e-6, 1e-14                                  # sqrt(vhat) comparable with eps
    if step == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    lr, b1, b2, eps = BB.f32(1e-2), BB.f32(0.9), BB.f32(0.999), BB.f32(1e-8)
    for gscale, wd in ((1.0, 0.0), (BB.f32(1 / 128), BB.f32(0.1))):
        for dev in (False, True):
            refs, bounds = BB.adam_bound(p.double(), g.double(), m.double(), v.double(), lr, b1, b2, eps, step, gscale, wd, dev)
            for order in (0, 1):
                got = adam32(p, g, m, v, lr, b1, b2, eps, step, gscale, wd, order)
                for name, gt, r, b in zip("pmv", got, refs, bounds):
                    assert_inside(gt, r, b, f"adam {name} step={step} order={order}")
        a64 = [t.double() for t in (p, g, m, v)]
        if step == 1000:
            assert_outside(adam32(*a64, lr, b1, b2, eps, step, gscale, wd, no_bc=True)[0], refs[0], bounds[0], "adam without bias correction")
        assert_outside(adam32(*a64, lr, b1, b2, BB.f32(1e-3), step, gscale, wd, eps_inside=True)[0],
                       BB.adam_bound(*a64, lr, b1, b2, BB.f32(1e-3), step, gscale, wd)[0][0], BB.adam_bound(*a64, lr, b1, b2, BB.f32(1e-3), step, gscale, wd)[1][0],
                       "adam with eps inside the root")
        assert_outside(adam32(*a64, lr, b1, b2, eps, step, gscale, wd, eps_inside=True)[0][1:2], refs[0][1:2], bounds[0][1:2], "adam with eps inside the root (small v)")


# ---------------------------------------------------------------------------------------------------------------------------------
# routing and masks
def maxpool_bwd_first(x, dy, B, H, W, last=False):
    """dy routed to the first (mutant: last) maximum of each 2x2 window in scan order; x [B*H*W, C]"""
    C = x.shape[1]
    win = x.view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(-1, C, 4)
    mx = win.max(-1, keepdim=True).values
    hit = win == mx
    pos = torch.arange(4).view(1, 1, 4)
    arg = torch.where(hit, pos, torch.full_like(pos, -1 if last else 4))
    arg = arg.max(-1).values if last else arg.min(-1).values
    out = torch.zeros_like(win)
    out.scatter_(2, arg.unsqueeze(-1), dy.view(-1, C, 1))
    return out.view(B, H // 2, W // 2, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B * H * W, C)


def test_maxpool_bwd_routing_reference_and_mutant():
    B, H, W, C = 2, 6, 8, 5
    x = torch.randint(0, 3, (B * H * W, C), generator=torch.Generator().manual_seed(3)).double()      # many ties
    dy = randn(B * (H // 2) * (W // 2), C, seed=4).double()
    xg = x.view(B, H, W, C).permute(0, 3, 1, 2).clone().requires_grad_(True)
    F.max_pool2d(xg, 2).backward(dy.view(B, H // 2, W // 2, C).permute(0, 3, 1, 2))
    ref = xg.grad.permute(0, 2, 3, 1).reshape(-1, C)
    assert torch.equal(maxpool_bwd_first(x, dy, B, H, W), ref), "F.max_pool2d keeps the first maximum"
    assert not torch.equal(maxpool_bwd_first(x, dy, B, H, W, last=True), ref), "mutant survived: maxpool routing to the last maximum"


def test_dropout_bound_and_mutants():
    n = 4096
    x, res = randn(n, seed=1), randn(n, seed=2)
    for p in (0.0, 0.1, 0.999):
        thr = int(min(4294967295.0, float(np.float32(p)) * 4294967296.0))
        keep = torch.from_numpy(BB.dropout_keep_np(12345, np.arange(n) + 77, thr))
        if p == 0.1:
            assert 0.85 < float(keep.float().mean()) < 0.95
        if p == 0.0:
            assert bool(keep.all())
        for r in (None, res):
            ref, bound = BB.dropout_bound(x.double(), keep, p, None if r is None else r.double())
            pf = BB.f32(p)
            y = torch.where(keep, x / (1 - pf), torch.zeros_like(x))
            assert_inside(y if r is None else y + r, ref, bound, f"dropout p={p}")
            y2 = x * keep.float() * (1.0 / (1.0 - pf))
            assert_inside(y2 if r is None else r + y2, ref, bound, f"dropout order 2 p={p}")
            if p == 0.1:
                y3 = torch.where(keep, x, torch.zeros_like(x)).double()
                assert_outside(y3 if r is None else y3 + r.double(), ref, bound, "dropout without the 1 / (1 - p) factor")
    # saturation of the fp16 store
    big = torch.tensor([65504.0, -65504.0], dtype=F64)
    ref, bound = BB.dropout_bound(big, torch.tensor([True, True]), 0.1, None, True, True)
    assert bool((ref.abs() == 65504.0).all())
    assert_outside(torch.tensor([float("inf"), float("-inf")]), ref, bound, "dropout: an fp16 store that overflows to inf")
