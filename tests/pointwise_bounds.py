"""Error bounds of the row-wise, elementwise and conv-tail kernels (csrc/elementwise.hip, csrc/conv.hip outside the patch embedding), built
like error_bound() of tests/test_gemm_variants_gpu.py: the largest |kernel - float64 reference| a CORRECT fp32 kernel can show, element by
element, from the reference's own intermediates.  No constant here is fitted to what a kernel returns; tests/test_pointwise_bounds_cpu.py
shows that the bounds hold for fp32 evaluations in other operation orders and that a fixed list of real kernel mistakes falls outside them.

Terms (U = 2^-24, the fp32 unit round-off; all tensors float64, inputs already rounded to the kernel's input type):
  * n fp32 operations on a sum: n * U * (sum of the absolute terms) -- the gamma_n bound, any summation order;
  * exact-erf GELU: Lipschitz constant 1.13 on the incoming error + the 5e-5 absolute error csrc/common.h states for its polynomial form
    (the Abramowitz-Stegun form of LayerNorm's epilogue, 1.5e-7 on erf, lies below that for every |x| the tests use);
  * the __expf sigmoid: 1e-6 (a few fp32 ulps of a value <= 1), as in error_bound();
  * fused LayerNorms: the pre-norm error, the error of the mean and the relative error of rstd, amplified by rstd * |ln_w| (ln_tail);
  * bilinear / image_prep: the fp32 error of the source coordinate times the largest step between neighbouring source pixels of the plane
    (an upper bound of the spread of the four neighbours on either side of a cell boundary) + the interpolation's own roundings;
  * prompt_points: the argument round-off U * n * |a| of sin / cos (Lipschitz 1) + one ulp of the function value;
  * a 16-bit store: half an ulp of the output type relative to the value, 2^-11 (fp16) or 2^-8 (bf16), + half the fp16 subnormal spacing.
"""
import math

import torch

U = 2.0 ** -24
GELU_LIP, GELU_ABS, SIGMOID_ABS = 1.13, 5e-5, 1e-6


def store16(ref, e, fp16=True):
    """bound after a round-to-nearest store of the value in the 16-bit operand type"""
    return e + (2.0 ** -11 if fp16 else 2.0 ** -8) * (ref.abs() + e) + (2.0 ** -25 if fp16 else 0.0)


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def ln_stats(a, da, eps):
    """the statistics of ln_tail and their errors: (d, rstd, dd, rel) = a - mean, 1 / sqrt(var + eps), the absolute error of d and the
    relative error of rstd (see ln_tail for the steps)"""
    C = a.shape[-1]
    da = torch.as_tensor(da, dtype=a.dtype, device=a.device).expand_as(a)
    mean = a.mean(-1, keepdim=True)
    d = a - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    dmean = da.mean(-1, keepdim=True) + (C + 1) * U * a.abs().mean(-1, keepdim=True)
    dd = da + dmean + U * d.abs()
    dvar = (2 * d.abs() * dd + dd * dd).mean(-1, keepdim=True) + (C + 3) * U * var
    r = dvar / (var + eps)
    rel = torch.where(r < 0.5, 0.5 * r / (1.0 - r.clamp(max=0.5)), torch.full_like(r, float("inf"))) + 3 * U
    return d, rstd, dd, rel


def ln_tail(a, da, w, b, eps):
    """LayerNorm over the last dim of float64 `a` whose fp32 counterpart carries the absolute error `da` (tensor or 0.0): returns
    (pre, dpre) = the float64 result d * rstd * w + b and its bound.  Steps: mean (C - 1 additions and a division of values of mean size
    mean|a|), d = a - mean, var (C + 3 operations on d^2, first-order in the error of d), rstd = 1 / sqrt(var + eps) (three more
    roundings; relative error r / 2 / (1 - r) with r = dvar / (var + eps), infinite if r >= 0.5), the affine (three roundings)."""
    d, rstd, dd, rel = ln_stats(a, da, eps)
    pre = d * rstd * w + b
    dpre = w.abs() * rstd * (dd + d.abs() * rel) * (1.0 + rel) + 3 * U * (d * rstd * w).abs() + U * pre.abs()
    return pre, dpre


def act_store(pre, dpre, act, out16, fp16=True):
    """(ref, bound) after the optional GELU and the store"""
    ref, e = (gelu64(pre), dpre * GELU_LIP + GELU_ABS) if act == 1 else (pre, dpre)
    return ref, (store16(ref, e, fp16) if out16 else e)


def layernorm_bound(x, w, b, eps, act=0, out16=False, fp16=True):
    """msam2_layernorm / _dual: x [rows, C] (rounded to the input type), fp32 w, b -> (ref, bound)"""
    pre, dpre = ln_tail(x, 0.0, w, b, eps)
    return act_store(pre, dpre, act, out16, fp16)


def add_cast_bound(a, b, alpha, out16=False, fp16=True):
    """out = a + alpha * b: two roundings (product, sum); cast only (b is None): exact in fp32 -> (ref, bound)"""
    if b is None:
        ref, e = a.clone(), torch.zeros_like(a)
    else:
        ref = a + alpha * b
        e = U * (alpha * b).abs() + U * ref.abs()
    return ref, (store16(ref, e, fp16) if out16 else e)


def rope_bound(re, im, c, s, fp16=True):
    """(re + i im)(c + i s) with the kernel's own fp32 table: two products and a sum per component -> (ref_re, ref_im, b_re, b_im)"""
    rr, ri = re * c - im * s, re * s + im * c
    er = 2 * U * ((re * c).abs() + (im * s).abs())
    ei = 2 * U * ((re * s).abs() + (im * c).abs())
    return rr, ri, store16(rr, er, fp16), store16(ri, ei, fp16)


def plane_step(x):
    """largest |difference| between horizontally / vertically adjacent pixels of each plane of x [P, h, w] -> ([P,1,1], [P,1,1])"""
    P = x.shape[0]
    z = x.new_zeros(P)
    sx = (x[:, :, 1:] - x[:, :, :-1]).abs().reshape(P, -1).max(1).values if x.shape[2] > 1 else z
    sy = (x[:, 1:, :] - x[:, :-1, :]).abs().reshape(P, -1).max(1).values if x.shape[1] > 1 else z
    return sx.view(P, 1, 1), sy.view(P, 1, 1)


def bilinear_ref(x, H, W):
    """float64 bilinear resize, align_corners=False, of x [P, h, w] (F.interpolate's rule, written out so that the intermediates exist):
    returns ref [P, H, W] and the source coordinates fy [H], fx [W]"""
    P, h, w = x.shape
    ar = lambda n: torch.arange(n, dtype=torch.float64, device=x.device)
    fy = ((ar(H) + 0.5) * (h / H) - 0.5).clamp(min=0)
    fx = ((ar(W) + 0.5) * (w / W) - 0.5).clamp(min=0)
    y0, x0 = fy.floor().long().clamp(max=h - 1), fx.floor().long().clamp(max=w - 1)
    y1, x1 = (y0 + 1).clamp(max=h - 1), (x0 + 1).clamp(max=w - 1)
    ly, lx = (fy - y0).view(1, H, 1), (fx - x0).view(1, 1, W)
    g = lambda yy, xx: x[:, yy][:, :, xx]
    ref = (1 - ly) * ((1 - lx) * g(y0, x0) + lx * g(y0, x1)) + ly * ((1 - lx) * g(y1, x0) + lx * g(y1, x1))
    return ref, fy, fx


def bilinear_bound(x, H, W, pixel_err=0.0):
    """msam2_bilinear_upsample (and, with pixel_err = U * |pixel|, the resize of image_prep): coordinate f = (X + 0.5) * s - 0.5 with s
    rounded to fp32: three roundings of values <= f + 0.5 -> df = 3 U (f + 0.5); the weight l = f - floor(f) is exact, 1 - l one rounding.
    Bound: df * step (both axes) + 8 roundings of the convex combination, each <= U max|neighbour| -> (ref, bound)"""
    ref, fy, fx = bilinear_ref(x, H, W)
    sx, sy = plane_step(x)
    dfy, dfx = (3 * U * (fy + 0.5)).view(1, H, 1), (3 * U * (fx + 0.5)).view(1, 1, W)
    amax = x.abs().reshape(x.shape[0], -1).max(1).values.view(-1, 1, 1)
    return ref, dfy * sy + dfx * sx + 8 * U * amax + pixel_err


def aa_weights(n_in, f, dtype=torch.float64, device="cpu", renorm=True):
    """[n_in / f, n_in] weights of the anti-aliased triangle filter of half-width f source pixels (separable, renormalised per output)"""
    o = torch.arange(n_in // f, dtype=dtype, device=device).view(-1, 1)
    i = torch.arange(n_in, dtype=dtype, device=device).view(1, -1)
    c = (o + 0.5) * f
    wt = (1.0 - ((i + 0.5 - c) / f).abs()).clamp(min=0)
    return wt / (wt.sum(1, keepdim=True) if renorm else float(f))


def aa_downsample_bound(x, f, in_scale, in_bias):
    """msam2_aa_downsample on x [P, H, W]: v = x * scale + bias (two roundings), weights w = max(0, 1 - |.| / f) / sum (exact dyadic
    numerators for the power-of-two factors; the sum of <= 2 f terms and the division: (2 f + 2) roundings), then 2 f additions per axis:
    n = 2 * (2 f) + 2 * (2 f + 3) + 2 roundings on sum w |v| -> (ref, bound)"""
    P, H, W = x.shape
    v = x * in_scale + in_bias
    wy, wx = aa_weights(H, f, x.dtype, x.device), aa_weights(W, f, x.dtype, x.device)
    ref = torch.einsum("oh,phw,qw->poq", wy, v, wx)
    absv = torch.einsum("oh,phw,qw->poq", wy, (x * in_scale).abs() + abs(in_bias), wx)
    return ref, (8 * f + 8) * U * absv


def conv3x3s2_ln_gelu_bound(v, dv, w, bias, ln_w, ln_b, fp16=True):
    """msam2_conv3x3s2_ln_gelu: v [B, Cin, H, W] float64 is the conv's input AFTER the mask transform, dv its absolute error (0 for modes 0
    and 2, whose values are exact; mscale * SIGMOID_ABS + U |v| for mode 1).  Pre-norm: 9 Cin + 1 operations on |bias| + sum |v w| plus
    sum dv |w|; LayerNorm over Cout with eps 1e-6 (ln_tail), GELU, 16-bit store -> (ref, bound) as [B * Ho * Wo, Cout]"""
    import torch.nn.functional as F
    cout, cin = w.shape[:2]
    acc = F.conv2d(v, w, bias, stride=2, padding=1)
    mag = F.conv2d(v.abs(), w.abs(), bias.abs(), stride=2, padding=1)
    dvt = torch.as_tensor(dv, dtype=v.dtype, device=v.device).expand_as(v)
    dacc = (9 * cin + 1) * U * mag + F.conv2d(dvt, w.abs(), None, stride=2, padding=1)
    nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(-1, cout)
    pre, dpre = ln_tail(nhwc(acc), nhwc(dacc), ln_w, ln_b, 1e-6)
    return act_store(pre, dpre, 1, True, fp16)


def dwconv7x7_ln_bound(x, w, bias, ln_w, ln_b, fp16=True):
    """msam2_dwconv7x7_ln: x [B, C, H, W] float64, w [C, 1, 7, 7]: 50 operations on |bias| + sum |x w|, LayerNorm over C (eps 1e-6), 16-bit
    store -> (ref, bound) as [B * H * W, C]"""
    import torch.nn.functional as F
    C = x.shape[1]
    acc = F.conv2d(x, w, bias, padding=3, groups=C)
    mag = F.conv2d(x.abs(), w.abs(), bias.abs(), padding=3, groups=C)
    nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(-1, C)
    pre, dpre = ln_tail(nhwc(acc), nhwc(50 * U * mag), ln_w, ln_b, 1e-6)
    return act_store(pre, dpre, 0, True, fp16)


def pixel_shuffle_bound(g, bias, skip, ln_w, ln_b, B, h, w, fp16=True):
    """msam2_convt2x2_shuffle*: g [B*h*w, 4 C] (rounded to 16 bits), skip [B*4hw, C]: v = g(tok, sub) + bias + skip (two roundings), optional
    LayerNorm over C (eps 1e-6), GELU, 16-bit store -> (ref, bound) as [B * 4hw, C]"""
    C = bias.numel()
    gs = g.view(B, h, w, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B * 4 * h * w, C)
    v = gs + bias + skip
    dv = 2 * U * (gs.abs() + bias.abs() + skip.abs())
    if ln_w is not None:
        v, dv = ln_tail(v, dv, ln_w, ln_b, 1e-6)
    return act_store(v, dv, 1, True, fp16)


def hyper_masks_bound(hyper, up):
    """masks[n, k, p] = sum_c hyper[n, k, c] up[n, p, c]: C products and C additions in fp32 -> (ref, bound)"""
    C = hyper.shape[-1]
    ref = hyper @ up.transpose(1, 2)
    return ref, 2 * C * U * (hyper.abs() @ up.abs().transpose(1, 2))


def prompt_points_bound(a_terms, a, val):
    """sin / cos(a), a = 2 pi (cx g0 + cy g1): the argument carries ~8 roundings (coordinate normalisation, two products, the sum, 2 pi)
    of values <= a_terms = 2 pi (|cx g0| + |cy g1|) -> 8 U a_terms (Lipschitz 1), + 2 ulps of the value for sinf / cosf, + one rounding
    of the sum with the label embedding (val = the float64 output) -> bound"""
    return 8 * U * a_terms + 2 * U + U * val.abs() + 0 * a
