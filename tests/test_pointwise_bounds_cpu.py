"""The bounds of tests/pointwise_bounds.py are neither wrong nor slack (CPU): per kernel family, at shapes of the GPU matrix
(tests/test_pointwise_variants_gpu.py), an fp32 torch evaluation in ANOTHER operation order than the float64 reference lies within the bound at
every element, and so does its 16-bit-rounded copy within the 16-bit bound; a fixed list of mutants -- each a mistake a real kernel makes --
lies outside the bound at some element.  If a mutant survives, the bound or the data is too weak: that is what gets fixed, never the list.
Also here: helpers.kernel_key on literal kernel names."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointwise_bounds as PB  # noqa: E402
from helpers import kernel_key  # noqa: E402

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


def gelu32(x):
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def truncate16(x32, dtype):
    """fp32 -> 16 bits by dropping the low significand bits (round toward zero) instead of rounding to nearest"""
    r = x32.to(dtype)
    over = r.float().abs() > x32.abs()
    bits = r.view(torch.int16)
    return torch.where(over, bits - 1, bits).view(dtype)                  # sign-magnitude: one step toward zero


# ---------------------------------------------------------------------------------------------------------------------------------
def test_kernel_key_on_literal_names():
    cases = {
        "void gemm_kernel<128, 32, 4, 1>(GemmParams)": "gemm_kernel<128,32,4,1>",
        "_Z11gemm_kernelILi128ELi32ELi4ELi1EEv10GemmParams": "gemm_kernel<128,32,4,1>",
        "_Z17gemm_wstat_kernelILi4ELi1ELb0ELb1EEv10GemmParams": "gemm_wstat_kernel<4,1,false,true>",
        "void gemm_skinny_kernel<false>(GemmParams)": "gemm_skinny_kernel<false>",
        "_Z16gemm_glds_kernel10GemmParams": "gemm_glds_kernel",
        "_Z15add_cast_kernelIDF16_fDF16_EvPKT_llPKT0_llfPT1_lli": "add_cast_kernel<_Float16,float,_Float16>",
        "void add_cast_kernel<_Float16, float, _Float16>(_Float16 const*, long, long, float const*, long, long, float, _Float16*, long, long, int)":
            "add_cast_kernel<_Float16,float,_Float16>",
        "_Z16layernorm_kernelIfDF16bLi12EEvPKT_lPKfS4_PT0_lliifPS5_l": "layernorm_kernel<float,__bf16,12>",
        "_Z16layernorm_kernelIfu6__bf16Li12EEvPKT_l": "layernorm_kernel<float,__bf16,12>",
        "void layernorm_kernel<float, __bf16, 12>(float const*, long)": "layernorm_kernel<float,__bf16,12>",
        "_Z21pixel_shuffle8_kernelILi64EfLb1EEvPKDF16_PKfPKT0_S4_S4_PS0_iii": "pixel_shuffle8_kernel<64,float,true>",
        "void pixel_shuffle8_kernel<64, float, true>(_Float16 const*, float const*)": "pixel_shuffle8_kernel<64,float,true>",
        "_Z24conv3x3s2_ln_gelu_kernelILi4ELi16EDF16_EvPKT1_PKfS5_S5_S5_PDF16_iiiiff": "conv3x3s2_ln_gelu_kernel<4,16,_Float16>",
        "_Z21space_to_depth_kernelIfEvPKT_PDF16_iiiiii": "space_to_depth_kernel<float>",
        "_Z21upsample2x_add_kernelPfPKfiiii": "upsample2x_add_kernel",
        "_Z3fooILin3EEvv": "foo<-3>",
        "_Z18window_move_kernelILb0EjEvPhlS0_PKhiiiiiiii": "window_move_kernel<false,unsignedint>",
        "void window_move_kernel<false, unsigned int>(unsigned char*, long)": "window_move_kernel<false,unsignedint>",
        # what a demangler without the bf16 mangling makes of the bf16 build's names, where it does not give up
        "void layernorm_kernel<bool _Accum, 12>(bool _Accum const*, long, float const*, float const*, float*, long)": "layernorm_kernel<__bf16,float,12>",
        "void pixel_shuffle8_kernel<32, bool _Accum, bool, E>(bool _Accum const*, float const*)": "pixel_shuffle8_kernel<32,__bf16,true>",
        "void layernorm_bwd_kernel<bool _Accum, int, E>(float const*, long, bool _Accum const*)": "layernorm_bwd_kernel<__bf16,1>",
        "void pixel_shuffle8_kernel<64, float, false>(bool _Accum const*, float const*, float const*)": "pixel_shuffle8_kernel<64,float,false>",
        "_Z21pixel_shuffle8_kernelILi32EDF16bLb0EEvPKDF16bPKfPKT0_S3_S3_PS0_iii": "pixel_shuffle8_kernel<32,__bf16,false>",
    }
    for name, key in cases.items():
        assert kernel_key(name) == key, name


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm
def ln_rows(rows, C, seed):
    x = randn(rows, C, seed=seed) * (0.5 + (torch.arange(rows) % 4).float())[:, None] + 2.0 * ((torch.arange(rows) % 3).float() - 1)[:, None]
    x[1] = 1000.0 + randn(C, seed=seed + 1)                   # mean = 1000 std
    x[2] = 1e-3 * randn(C, seed=seed + 4)                     # var ~ eps
    x[rows - 1] = 2.0                                         # constant
    return x, 1.0 + 0.5 * randn(C, seed=seed + 2), randn(C, seed=seed + 3)


def ln32(x, w, b, eps, act, C_div=None, use_eps=True, one_pass=False):
    """fp32 LayerNorm summing from the other end of the row; the keyword arguments switch the mutants on"""
    C = x.shape[-1]
    mean = x.flip(-1).sum(-1, keepdim=True) / C
    if one_pass:
        var = (x * x).flip(-1).sum(-1, keepdim=True) / C - mean * mean
    else:
        var = ((x - mean) ** 2).flip(-1).sum(-1, keepdim=True) / (C_div or C)
    y = (x - mean) / torch.sqrt(var + (eps if use_eps else 0.0)) * w + b
    return gelu32(y) if act else y


@pytest.mark.parametrize("C", [1, 4, 63, 100, 132, 388, 772, 1023, 1024])
def test_layernorm_bound(C):
    x, w, b = ln_rows(9, C, C)
    for ti in (F32, torch.float16, torch.bfloat16):
        xr = x.to(ti).float()
        for act in (0, 1):
            ref, bound = PB.layernorm_bound(xr.double(), w.double(), b.double(), 1e-6, act)
            y = ln32(xr, w, b, 1e-6, act)
            assert_inside(y, ref, bound, f"layernorm C={C} act={act} in={ti}")
            assert bool((ref[-1] == (PB.gelu64(b.double()) if act else b.double())).all()), "constant row: the reference is the bias"
            for t16, fp16 in T16:
                ref, bound = PB.layernorm_bound(xr.double(), w.double(), b.double(), 1e-6, act, True, fp16)
                assert_inside(y.to(t16), ref, bound, f"layernorm C={C} act={act} in={ti} out={t16}")


def test_layernorm_mutants():
    for C in (4, 100):
        x, w, b = ln_rows(9, C, C)
        x64, w64, b64 = x.double(), w.double(), b.double()
        ref, bound = PB.layernorm_bound(x64, w64, b64, 1e-6)
        assert_outside(ln32(x64, w64, b64, 1e-6, 0, C_div=C - 1), ref, bound, f"variance over C - 1 (C={C})")
        assert_outside(ln32(x64, w64, b64, 1e-6, 0, use_eps=False)[2:3], ref[2:3], bound[2:3], f"eps dropped (C={C})")
        assert_outside(ln32(x, w, b, 1e-6, 0, one_pass=True)[1:2], ref[1:2], bound[1:2], f"one-pass variance on the mean >> std row (C={C})")
        assert_outside(ln32(x64, w64.roll(1), b64.roll(1), 1e-6, 0), ref, bound, f"weight and bias one channel off (C={C})")
        y = ln32(x, w, b, 1e-6, 0)
        for t16, fp16 in T16:
            ref16, bound16 = PB.layernorm_bound(x64, w64, b64, 1e-6, 0, True, fp16)
            assert_outside(truncate16(y, t16), ref16, bound16, f"truncating 16-bit store {t16} (C={C})")


# ---------------------------------------------------------------------------------------------------------------------------------
# add_cast, rope
def test_add_cast_bound_and_mutants():
    a, b = randn(3, 5, 6, seed=1), randn(3, 1, 6, seed=2).expand(3, 5, 6)
    for ta in (F32, torch.float16, torch.bfloat16):
        ar, br = a.to(ta).float(), b.to(ta).float()
        for alpha in (0.75, -2.5, 1.0):
            ref, bound = PB.add_cast_bound(ar.double(), br.double(), alpha)
            y = torch.addcmul(ar, torch.full_like(br, alpha), br)                      # another order / contraction than a + (alpha * b)
            assert_inside(y, ref, bound, f"add_cast alpha={alpha}")
            assert_inside(alpha * br + ar, ref, bound, f"add_cast alpha={alpha}")
            for t16, fp16 in T16:
                ref16, bound16 = PB.add_cast_bound(ar.double(), br.double(), alpha, True, fp16)
                assert_inside(y.to(t16), ref16, bound16, f"add_cast alpha={alpha} out={t16}")
                if ta == F32:                                  # (sums of 16-bit inputs are exact or ties in 16 bits: nothing to truncate)
                    assert_outside(truncate16(y, t16), ref16, bound16, f"add_cast truncating store {t16}")
            if alpha != 1.0:
                assert_outside(alpha * ar.double() + br.double(), ref, bound, "alpha applied to a")
        ref, bound = PB.add_cast_bound(ar.double(), None, 1.0)
        assert bool((bound == 0).all()) and bool((ref == ar.double()).all())


def test_rope_bound_and_mutants():
    for t16, fp16 in T16:
        x = (randn(2, 10, 8, seed=3) * 3).to(t16).float()
        ang = randn(10, 4, seed=4) * 3
        c, s = ang.cos(), ang.sin()
        re, im = x[..., 0::2], x[..., 1::2]
        rr, ri, br, bi = PB.rope_bound(re.double(), im.double(), c.double(), s.double(), fp16)
        yr, yi = torch.addcmul(-(im * s), re, c), torch.addcmul(im * c, re, s)
        assert_inside(yr.to(t16), rr, br, "rope re")
        assert_inside(yi.to(t16), ri, bi, "rope im")
        assert_outside((re * c + im * s).to(t16), rr, br, "rotation by the conjugate")
        assert_outside(truncate16(yr, t16), rr, br, f"rope truncating store {t16}")


# ---------------------------------------------------------------------------------------------------------------------------------
# bilinear, aa_downsample
def bilinear32(x, H, W, half_pixel=True):
    """fp32 bilinear in the lerp form a + l (b - a), horizontal pass first"""
    P, h, w = x.shape
    sy, sx = torch.tensor(h / H, dtype=F32), torch.tensor(w / W, dtype=F32)
    o = 0.5 if half_pixel else 0.0
    fy = ((torch.arange(H, dtype=F32) + o) * sy - o).clamp(min=0)
    fx = ((torch.arange(W, dtype=F32) + o) * sx - o).clamp(min=0)
    y0, x0 = fy.floor().long().clamp(max=h - 1), fx.floor().long().clamp(max=w - 1)
    y1, x1 = (y0 + 1).clamp(max=h - 1), (x0 + 1).clamp(max=w - 1)
    ly, lx = (fy - y0).view(1, H, 1), (fx - x0).view(1, 1, W)
    rows = x[:, :, x0] + (x[:, :, x1] - x[:, :, x0]) * lx.view(1, 1, W)
    return rows[:, y0] + (rows[:, y1] - rows[:, y0]) * ly


BIL = [(3, 16, 24, 50, 97), (2, 7, 5, 7, 5), (2, 32, 32, 12, 20), (2, 5, 6, 11, 18), (2, 8, 8, 16, 32), (1, 1, 1, 3, 4), (1, 64, 64, 513, 514)]


@pytest.mark.parametrize("P,h,w,H,W", BIL)
def test_bilinear_bound_and_mutants(P, h, w, H, W):
    x = randn(P, h, w, seed=h + w)
    ref, bound = PB.bilinear_bound(x.double(), H, W)
    ours = F.interpolate(x.double()[None], size=(H, W), mode="bilinear", align_corners=False)[0]
    assert float((ref - ours).abs().max()) < 1e-12, "the restated reference is F.interpolate"
    assert_inside(bilinear32(x, H, W), ref, bound, f"bilinear {h}x{w}->{H}x{W}")
    assert_inside(F.interpolate(x[None], size=(H, W), mode="bilinear", align_corners=False)[0], ref, bound, "bilinear (torch fp32)")
    if (h, w) != (H, W) and h > 1:
        assert_outside(F.interpolate(x.double()[None], size=(H, W), mode="bilinear", align_corners=True)[0], ref, bound, "align_corners=True")
        assert_outside(bilinear32(x.double(), H, W, half_pixel=False), ref, bound, "half-pixel offset dropped")


@pytest.mark.parametrize("P,H,W,f,s,b", [(2, 8, 12, 1, 1.0, 0.0), (2, 8, 12, 2, 20.0, -10.0), (3, 16, 8, 4, 20.0, -10.0), (1, 4, 4, 4, 1.0, 0.0), (1, 250, 130, 2, 20.0, -10.0)])
def test_aa_downsample_bound_and_mutants(P, H, W, f, s, b):
    x = randn(P, H, W, seed=H + f)
    ref, bound = PB.aa_downsample_bound(x.double(), f, s, b)
    ours = F.interpolate((x.double() * s + b)[None], size=(H // f, W // f), mode="bilinear", antialias=True, align_corners=False)[0]
    assert float((ref - ours).abs().max()) < 1e-12 * max(1.0, float(ref.abs().max())), "the restated reference is F.interpolate(antialias=True)"
    y = torch.einsum("qw,pow->poq", PB.aa_weights(W, f, F32), torch.einsum("oh,phw->pow", PB.aa_weights(H, f, F32), x * s + b))
    assert_inside(y, ref, bound, f"aa_downsample {H}x{W}/{f}")
    assert_inside(F.interpolate((x * s + b)[None], size=(H // f, W // f), mode="bilinear", antialias=True, align_corners=False)[0], ref, bound, "aa (torch fp32)")
    if f > 1 and H // f > 1:
        wy, wx = PB.aa_weights(H, f, F64, renorm=False), PB.aa_weights(W, f, F64, renorm=False)
        assert_outside(torch.einsum("oh,phw,qw->poq", wy, x.double() * s + b, wx), ref, bound, "weights not renormalised at the border")
        interior = torch.einsum("oh,phw,qw->poq", wy, x.double() * s + b, wx)[:, 1:-1, 1:-1]
        assert inside(interior, ref[:, 1:-1, 1:-1], bound[:, 1:-1, 1:-1]) or H // f < 3, "away from the border the weights already sum to one"


# ---------------------------------------------------------------------------------------------------------------------------------
# the fused LayerNorm tails: conv3x3s2_ln_gelu, dwconv7x7_ln, convt2x2_shuffle
def ln2d32(a, w, b):
    mean = a.flip(-1).sum(-1, keepdim=True) / a.shape[-1]
    var = ((a - mean) ** 2).flip(-1).sum(-1, keepdim=True) / a.shape[-1]
    return (a - mean) / torch.sqrt(var + 1e-6) * w + b


def conv_eval(v, w, bias, lw, lb, pad="zero"):
    """conv + LayerNorm2d + GELU in v's precision -> [B * Ho * Wo, Cout]"""
    if pad == "zero":
        acc = F.conv2d(v, w, bias, stride=2, padding=1)
    else:
        acc = F.conv2d(F.pad(v, (1, 1, 1, 1), mode="replicate"), w, bias, stride=2)
    a = acc.permute(0, 2, 3, 1).reshape(-1, w.shape[0])
    return gelu32(ln2d32(a, lw, lb))


@pytest.mark.parametrize("cin", [1, 4, 16])
@pytest.mark.parametrize("B,H,W", [(1, 2, 2), (1, 2, 6), (3, 6, 2), (1, 10, 14), (2, 16, 24)])
def test_conv3x3s2_ln_gelu_bound_and_mutants(cin, B, H, W):
    cout = 4 * cin
    w = randn(cout, cin, 3, 3, seed=cin) * (0.5 / math.sqrt(cin))
    bias, lw, lb = randn(cout, seed=cin + 1), 1.0 + 0.2 * randn(cout, seed=cin + 2), 0.2 * randn(cout, seed=cin + 3)
    x = randn(B, cin, H, W, seed=H * W + cin)
    modes = (0, 1, 2) if cin == 1 else (0,)
    for mode in modes:
        for t16, fp16 in T16:
            xr = x if cin == 1 else x.to(t16).float()
            if mode == 2:
                xr = xr.clone()
                xr.flatten()[0::3] = 0.0                       # exact zeros: "> 0" and ">= 0" differ
            v64, dv = xr.double(), 0.0
            v32 = xr
            if mode == 1:
                v64 = 20.0 * torch.sigmoid(3 * xr.double()) - 10.0
                dv = 20.0 * PB.SIGMOID_ABS + 2 * PB.U * (v64.abs() + 10.0)
                v32 = 20.0 / (1.0 + torch.exp(-3 * xr)) - 10.0
            elif mode == 2:
                v64 = (xr.double() > 0).double() * 20.0 - 10.0
                v32 = v64.float()
            args64 = (w.double(), bias.double(), lw.double(), lb.double())
            ref, bound = PB.conv3x3s2_ln_gelu_bound(v64, dv, *args64, fp16)
            y = conv_eval(v32, w, bias, lw, lb)
            assert_inside(y.to(t16), ref, bound, f"conv3x3s2 cin={cin} mode={mode} {B}x{H}x{W} {t16}")
            if (H, W) == (10, 14):
                assert_outside(conv_eval(v64, w.double().transpose(2, 3), *args64[1:]), ref, bound, "conv taps (ky, kx) transposed")
                assert_outside(conv_eval(v64, *args64, pad="replicate"), ref, bound, "padding replicated instead of zero")
                assert_outside(truncate16(y, t16), ref, bound, f"conv truncating store {t16}")
                if mode == 2:
                    assert_outside(conv_eval((xr.double() >= 0).double() * 20.0 - 10.0, *args64), ref, bound, "mode 2 with >=")


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (1, 3, 5), (2, 7, 7), (1, 5, 23)])
def test_dwconv7x7_ln_bound_and_mutants(B, H, W):
    C = 256
    x, w = randn(B, C, H, W, seed=H * W), randn(C, 1, 7, 7, seed=1) * 0.2
    bias, lw, lb = randn(C, seed=2), 1.0 + 0.2 * randn(C, seed=3), 0.2 * randn(C, seed=4)
    ev = lambda xx, ww, bb, l1, l2: ln2d32(F.conv2d(xx, ww, bb, padding=3, groups=C).permute(0, 2, 3, 1).reshape(-1, C), l1, l2)
    y = ev(x, w, bias, lw, lb)
    for t16, fp16 in T16:
        ref, bound = PB.dwconv7x7_ln_bound(x.double(), w.double(), bias.double(), lw.double(), lb.double(), fp16)
        assert_inside(y.to(t16), ref, bound, f"dwconv7x7_ln {B}x{H}x{W} {t16}")
        if H > 1:
            assert_outside(ev(x.double(), w.double().transpose(2, 3), bias.double(), lw.double(), lb.double()), ref, bound, "dwconv taps transposed")
        assert_outside(ev(x.double(), w.double(), bias.double(), lw.double().roll(1), lb.double().roll(1)), ref, bound, "LayerNorm weight one channel off")


@pytest.mark.parametrize("C,ln", [(64, True), (32, False), (48, True), (16, False), (1, False)])
@pytest.mark.parametrize("B,h,w", [(1, 1, 1), (3, 3, 5)])
def test_pixel_shuffle_bound_and_mutants(C, ln, B, h, w):
    for t16, fp16 in T16:
        g, skip = randn(B * h * w, 4 * C, seed=C).to(t16).float(), randn(B * 4 * h * w, C, seed=C + 1).to(t16).float()
        bias, lw, lb = randn(C, seed=C + 2), 1.0 + 0.2 * randn(C, seed=C + 3), 0.2 * randn(C, seed=C + 4)
        ref, bound = PB.pixel_shuffle_bound(g.double(), bias.double(), skip.double(), lw.double() if ln else None, lb.double() if ln else None, B, h, w, fp16)

        def ev(gg, bb, ss, swap=False):
            v = gg.view(B, h, w, 2, 2, C)
            v = v.permute(0, 1, 4, 2, 3, 5) if swap else v.permute(0, 1, 3, 2, 4, 5)
            v = (ss + bb) + v.reshape(B * 4 * h * w, C)
            return gelu32(ln2d32(v, lw.to(v.dtype), lb.to(v.dtype)) if ln else v)
        assert_inside(ev(g, bias, skip).to(t16), ref, bound, f"pixel shuffle C={C} ln={ln} {t16}")
        assert_outside(ev(g.double(), bias.double(), skip.double(), swap=True), ref, bound, "pixel-shuffle sub-position (ky, kx) swapped")


# ---------------------------------------------------------------------------------------------------------------------------------
def test_hyper_masks_and_prompt_points_bounds():
    for t16, _ in T16:
        hyper, up = randn(3, 8, 32, seed=1), randn(3, 257, 32, seed=2).to(t16).float()
        ref, bound = PB.hyper_masks_bound(hyper.double(), up.double())
        assert_inside(hyper.flip(-1) @ up.flip(-1).transpose(1, 2), ref, bound, "hyper_masks")
        assert_outside(hyper.double().roll(1, -1) @ up.double().transpose(1, 2), ref, bound, "hyper_masks channels one off")
    xy = torch.tensor([[0.0, 0.0], [1023.0, 1023.0], [-7.5, 100.25], [1324.0, 511.0]])
    g = randn(2, 128, seed=3)
    c64 = 2.0 * ((xy.double() + 0.5) / 1024.0) - 1.0
    a64 = 2.0 * math.pi * (c64[:, 0:1] * g[0].double() + c64[:, 1:2] * g[1].double())
    terms = 2.0 * math.pi * ((c64[:, 0:1] * g[0].double()).abs() + (c64[:, 1:2] * g[1].double()).abs())
    c32 = 2.0 * ((xy + 0.5) * (1.0 / 1024.0)) - 1.0
    a32 = (c32[:, 1:2] * g[1] + c32[:, 0:1] * g[0]) * 6.283185307179586
    for fn in (torch.sin, torch.cos):
        ref = fn(a64)
        assert_inside(fn(a32), ref, PB.prompt_points_bound(terms, 0.0, ref), "prompt_points")
        assert_outside(fn(2.0 * math.pi * (c64[:, 0:1] * g[1].double() + c64[:, 1:2] * g[0].double())), ref, PB.prompt_points_bound(terms, 0.0, ref), "x and y rows of the matrix swapped")
