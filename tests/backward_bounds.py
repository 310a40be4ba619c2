"""Error bounds of the training-side pointwise and row kernels (csrc/backward.hip outside the GEMMs and the attention), in the style and with
the terms of tests/pointwise_bounds.py: the largest |kernel - float64 reference| a CORRECT fp32 kernel can show, element by element, from
the reference's own intermediates.  No constant here is fitted to what a kernel returns; tests/test_backward_bounds_cpu.py shows that fp32
evaluations in other operation orders lie inside the bounds and that a fixed list of real kernel mistakes falls outside them.

Further terms (U = 2^-24; all tensors float64, inputs already rounded to the kernel's input types):
  * a sum of n terms in ANY order (lane partials, LDS folds, atomics): n * U * (sum of the absolute terms) + the per-term errors;
  * Phi(x) of the GELU derivative: GELU_CDF_ABS for the clamped polynomial of csrc/common.h (measured against math.erf on the CPU by
    tests/test_backward_bounds_cpu.py -- its coefficients were fitted to the error of x Phi(x), not of Phi), 4 U for erff();
  * the hardware exp2 / __expf of a value <= 1: EXP_ABS, the SIGMOID_ABS of pointwise_bounds, + the round-off of its argument,
    U * |argument| * value per rounding;
  * resize adjoints: the fp32 error of the source coordinate, 3 U (|f| + 0.5), times the Lipschitz constant of the tap weight in the
    coordinate, on every tap that can carry weight, times |g|; + n * U * sum |w g|.
"""
import math

import numpy as np
import torch

from pointwise_bounds import SIGMOID_ABS, U, ln_stats, ln_tail, store16  # noqa: F401

EXP_ABS = SIGMOID_ABS
GELU_CDF_ABS = 6.6e-5      # max |Phi_poly - Phi| over [-10, 10]: 6.52e-5 at |x| = 0.443 in float64 and in the fp32 fma chain (the CPU file holds it to 5 %)
ERFF_ABS = 4 * U           # 0.5 * (1 + erff(x / sqrt 2)): erff within 2 ulps of a value <= 1, the argument's rounding (slope <= 0.4), the sum
INV_SQRT_2PI = 0.3989422804014327
OP16_MAX = 65504.0


def sum_bound(n, abs_terms_sum, per_term=0.0):
    """error of a sum of n fp32 terms in any order"""
    return n * U * abs_terms_sum + per_term


# ---------------------------------------------------------------------------------------------------------------------------------
def layernorm_bwd_bound(x, dy, gamma, eps, add=None, dgamma0=None, dbeta0=None):
    """msam2_layernorm_bwd: x [rows, C] fp32, dy rounded to its type, gamma fp32 -> ((dx, dgamma, dbeta), (b_dx, b_dgamma, b_dbeta)).
    xhat and rstd carry ln_tail's errors (dxh, rel); g = dy gamma one rounding; the row means m1 = mean(g), m2 = mean(g xhat): C + 1
    operations each; inner = g - m1 - xhat m2: a product and two subtractions; dx = rstd inner (+ add): one rounding each.
    dgamma / dbeta: rows + 1 terms (the value already there is one of them) in any order."""
    rows, C = x.shape
    one, zero = torch.ones(C, dtype=x.dtype, device=x.device), torch.zeros(C, dtype=x.dtype, device=x.device)
    xh, dxh = ln_tail(x, 0.0, one, zero, eps)
    _, rstd, _, rel = ln_stats(x, 0.0, eps)
    g = dy * gamma
    dg = U * g.abs()
    m1 = g.mean(-1, keepdim=True)
    dm1 = dg.mean(-1, keepdim=True) + (C + 1) * U * g.abs().mean(-1, keepdim=True)
    gx = g * xh
    dgx = g.abs() * dxh + dg * xh.abs() + dg * dxh + U * gx.abs()
    m2 = gx.mean(-1, keepdim=True)
    dm2 = dgx.mean(-1, keepdim=True) + (C + 1) * U * gx.abs().mean(-1, keepdim=True)
    inner = g - m1 - xh * m2
    dinner = dg + dm1 + xh.abs() * dm2 + dxh * m2.abs() + dxh * dm2 + U * (xh * m2).abs() + 2 * U * (g.abs() + m1.abs() + (xh * m2).abs())
    dx = rstd * inner
    ddx = rstd * dinner * (1.0 + rel) + rstd * inner.abs() * rel + U * dx.abs()
    if add is not None:
        dx = dx + add
        ddx = ddx + U * dx.abs()
    g0 = torch.zeros(C, dtype=x.dtype, device=x.device) if dgamma0 is None else dgamma0
    b0 = torch.zeros(C, dtype=x.dtype, device=x.device) if dbeta0 is None else dbeta0
    t = dy * xh
    dgamma = g0 + t.sum(0)
    b_dgamma = sum_bound(rows + 1, g0.abs() + t.abs().sum(0), (dy.abs() * dxh + U * t.abs()).sum(0))
    dbeta = b0 + dy.sum(0)
    b_dbeta = sum_bound(rows + 1, b0.abs() + dy.abs().sum(0))
    return (dx, dgamma, dbeta), (ddx, b_dgamma, b_dbeta)


# ---------------------------------------------------------------------------------------------------------------------------------
def phi64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    return phi64(x) + x * INV_SQRT_2PI * torch.exp(-0.5 * x * x)


def act_bwd_bound(pre, dy, act, poly, fp16=True):
    """msam2_act_bwd: out = dy * act'(pre) stored in 16 bits (saturating in the fp16 build).  GELU' = Phi(x) + x phi(x): Phi within
    GELU_CDF_ABS (poly: the vector kernel) or ERFF_ABS (the scalar kernel); x phi(x): the exponential's argument -x^2 / 2 carries two
    roundings, the exponential EXP_ABS, two products; the sum and the product with dy one rounding each.  ReLU' is exact."""
    if act == 2:
        ref = dy * (pre > 0).to(dy.dtype)
        e = torch.zeros_like(ref)
    else:
        arg = 0.5 * pre * pre
        xphi = pre * INV_SQRT_2PI * torch.exp(-arg)
        d = phi64(pre) + xphi
        dd = (GELU_CDF_ABS if poly else ERFF_ABS) + pre.abs() * INV_SQRT_2PI * EXP_ABS + (2 * arg + 3) * U * xphi.abs() + U * d.abs()
        ref = dy * d
        e = dy.abs() * dd + U * ref.abs()
    if fp16:
        ref = ref.clamp(-OP16_MAX, OP16_MAX)                 # f2op saturates; clamping moves kernel and reference towards each other
    return ref, store16(ref, e, fp16)


# ---------------------------------------------------------------------------------------------------------------------------------
LOG2E = 1.4426950408889634


def softmax_rows_bound(s, scale, fp16=True):
    """msam2_softmax_rows: t = s * sl2 - max * sl2 with sl2 = fl(scale * log2 e) (the host's product: relative error 2 U): four roundings
    of values <= |s sl2| + |m|; e = exp2(t) <= 1: EXP_ABS + ln 2 * dt * e; l = sum e: cols terms; p = e * (1 / l): two roundings; the store"""
    cols = s.shape[-1]
    a = s * (scale * LOG2E)
    m = a.max(-1, keepdim=True).values
    t = a - m
    e = torch.exp2(t)
    dt = 4 * U * (a.abs() + m.abs())
    de = EXP_ABS + math.log(2.0) * dt * e * torch.exp2(dt)
    l = e.sum(-1, keepdim=True)
    dl = sum_bound(cols, l, de.sum(-1, keepdim=True))
    p = e / l
    dp = de / (l - dl) + p * dl / (l - dl) + 2 * U * p
    return p, store16(p, dp, fp16)


def softmax_bwd_rows_bound(p, dp, scale, fp16=True):
    """msam2_softmax_bwd_rows: acc = sum p dp (cols + 1 operations), ds = scale * p * (dp - acc): a difference and two products; the store"""
    cols = p.shape[-1]
    pd = p * dp
    acc = pd.sum(-1, keepdim=True)
    dacc = sum_bound(cols + 1, pd.abs().sum(-1, keepdim=True))
    ref = scale * p * (dp - acc)
    e = (scale * p).abs() * (dacc + U * (dp - acc).abs()) + 2 * U * ref.abs()
    return ref, store16(ref, e, fp16)


# ---------------------------------------------------------------------------------------------------------------------------------
def convt_sub(g, B, h, w, C):
    """g [B*h*w, 4 C] -> [B*4hw, C]: pixel (b, Y, X) takes token (b, Y/2, X/2), sub-block (Y & 1) * 2 + (X & 1)"""
    return g.view(B, h, w, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B * 4 * h * w, C)


def convt_unsub(z, B, h, w, C):
    """the inverse gather: [B*4hw, C] -> [B*h*w, 4 C]"""
    return z.view(B, h, 2, w, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B * h * w, 4 * C)


def convt2x2_gather_bound(g, bias, skip, B, h, w):
    """z = g(tok, sub) + bias + skip in fp32: two roundings"""
    C = bias.numel()
    gs = convt_sub(g, B, h, w, C)
    ref = gs + bias + (skip if skip is not None else 0.0)
    return ref, 2 * U * (gs.abs() + bias.abs() + (skip.abs() if skip is not None else 0.0))


# ---------------------------------------------------------------------------------------------------------------------------------
def dw_taps(w):
    """taps [49, C] -> conv2d weight [C, 1, 7, 7]"""
    return w.t().reshape(-1, 1, 7, 7)


def dwconv7x7_bound(x, w, bias, flip):
    """msam2_dwconv7x7: x [B, C, H, W], taps w [49, C]: 50 operations on |bias| + sum |x w|.  flip: correlation with the flipped kernel"""
    import torch.nn.functional as F
    C = x.shape[1]
    k = dw_taps(w)
    if flip:
        k = k.flip(2, 3)
    ref = F.conv2d(x, k, bias, padding=3, groups=C)
    mag = F.conv2d(x.abs(), k.abs(), None if bias is None else bias.abs(), padding=3, groups=C)
    return ref, 50 * U * mag


def dwconv7x7_wgrad_bound(x, dy, dw0):
    """msam2_dwconv7x7_wgrad: dw[tap][c] = dw0 + sum over the B H W pixels of dy[p] x[p + offset(tap)] -> [49, C]: npix + 1 terms, any order"""
    B, C, H, W = x.shape
    xp = torch.nn.functional.pad(x, (3, 3, 3, 3))
    ref, mag = dw0.clone(), dw0.abs()
    for ky in range(7):
        for kx in range(7):
            t = dy * xp[:, :, ky:ky + H, kx:kx + W]
            ref[ky * 7 + kx] += t.sum((0, 2, 3))
            mag[ky * 7 + kx] += t.abs().sum((0, 2, 3))
    return ref, sum_bound(B * H * W + 1, mag)


def col2im3x3s2_bound(dcols, B, H, W, C):
    """msam2_col2im3x3s2: dcols [B*(H/2)*(W/2), 9 C] (columns (ky, kx, c)) -> dx [B*H*W, C], at most four terms per pixel"""
    import torch.nn.functional as F
    Ho, Wo = H // 2, W // 2
    cols = dcols.view(B, Ho * Wo, 9, C).permute(0, 3, 2, 1).reshape(B, C * 9, Ho * Wo)
    fold = lambda t: F.fold(t, (H, W), kernel_size=3, stride=2, padding=1).permute(0, 2, 3, 1).reshape(B * H * W, C)
    return fold(cols), 3 * U * fold(cols.abs())


# ---------------------------------------------------------------------------------------------------------------------------------
def _hat_matrix(n_out, n_src, dtype, device):
    """[n_out, n_src] bilinear (align_corners = False) weights of pointwise_bounds.bilinear_ref along one axis, and the bound of their fp32
    counterparts: the coordinate carries 3 U (f + 0.5), the hat function has slope 1, 1 - l one more rounding; every source the clamped
    taps can reach within that error may carry it"""
    o = torch.arange(n_out, dtype=dtype, device=device)
    f = ((o + 0.5) * (n_src / n_out) - 0.5).clamp(min=0)
    i0 = f.floor().long().clamp(max=n_src - 1)
    i1 = (i0 + 1).clamp(max=n_src - 1)
    l = f - i0
    Wm = torch.zeros(n_out, n_src, dtype=dtype, device=device)
    Wm.scatter_add_(1, i0.view(-1, 1), (1 - l).view(-1, 1))
    Wm.scatter_add_(1, i1.view(-1, 1), l.view(-1, 1))
    df = 3 * U * (f + 0.5) + U
    src = torch.arange(n_src, dtype=dtype, device=device).view(1, -1)
    near = (src - f.view(-1, 1)).abs() <= 1.0 + df.view(-1, 1)
    near |= (src == n_src - 1) & (f.view(-1, 1) >= n_src - 1)                # beyond the last source: both taps clamp onto it
    return Wm, torch.where(near, df.view(-1, 1).expand_as(Wm), torch.zeros_like(Wm))


def bilinear_bwd_bound(g, h, w):
    """msam2_bilinear_upsample_bwd: g [P, H, W] -> dx [P, h, w] = Wy^T g Wx; weight errors on both axes, then one product and one addition
    per visited output and axis: n = (taps per source along y) + (along x) + 2 operations on sum |wy wx g|"""
    P, H, W = g.shape
    Wy, dWy = _hat_matrix(H, h, g.dtype, g.device)
    Wx, dWx = _hat_matrix(W, w, g.dtype, g.device)
    ref = torch.einsum("Yy,pYX,Xx->pyx", Wy, g, Wx)
    ag = g.abs()
    n = int((Wy != 0).sum(0).max()) + int((Wx != 0).sum(0).max()) + 2
    bound = (torch.einsum("Yy,pYX,Xx->pyx", dWy, ag, Wx) + torch.einsum("Yy,pYX,Xx->pyx", Wy, ag, dWx) + torch.einsum("Yy,pYX,Xx->pyx", dWy, ag, dWx)
             + n * U * torch.einsum("Yy,pYX,Xx->pyx", Wy, ag, Wx))
    return ref, bound


def _cubic_matrix(n_out, n_src, dtype, device, A=-0.75):
    """[n_out, n_src] clamped 4-tap bicubic (align_corners = False, torch's A = -0.75) weights along one axis and the bound of their fp32
    counterparts: the tap polynomials have slope <= 1.5 in the coordinate (error 3 U (|f| + 0.5)), their own evaluation ~8 roundings of
    values <= 3; a clamped border source can collect all four taps"""
    o = torch.arange(n_out, dtype=dtype, device=device)
    f = (o + 0.5) * (n_src / n_out) - 0.5
    i0 = f.floor()
    t = f - i0
    c1 = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1
    c2 = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    taps = [c2(t + 1), c1(t), c1(1 - t), c2(2 - t)]
    Wm = torch.zeros(n_out, n_src, dtype=dtype, device=device)
    dW = torch.zeros(n_out, n_src, dtype=dtype, device=device)
    dw = 1.5 * (3 * U * (f.abs() + 0.5)) + 24 * U
    for a in range(4):
        idx = (i0.long() - 1 + a).clamp(0, n_src - 1).view(-1, 1)
        Wm.scatter_add_(1, idx, taps[a].view(-1, 1))
    for a in range(-1, 5):                                   # one tap further on either side: the floor may fall the other way in fp32
        idx = (i0.long() - 1 + a).clamp(0, n_src - 1).view(-1, 1)
        dW.scatter_add_(1, idx, dw.view(-1, 1))
    return Wm, dW


def hiera_pos_embed_bwd_bound(d_table, C, bh, bw, h, w, window, A=-0.75):
    """msam2_hiera_pos_embed_bwd: d_table [h*w, C] -> (d_pos_embed [C, bh, bw], d_window [C, window, window]) and their bounds.  The resize
    adjoint runs as two passes of w and h terms; the window sum has (h / window)(w / window) terms."""
    g = d_table.view(h, w, C)
    Wy, dWy = _cubic_matrix(h, bh, g.dtype, g.device, A)
    Wx, dWx = _cubic_matrix(w, bw, g.dtype, g.device, A)
    ein = lambda a, t, b: torch.einsum("Yy,YXc,Xx->cyx", a, t, b)
    ag = g.abs()
    ref = ein(Wy, g, Wx)
    bound = ein(dWy, ag, Wx.abs()) + ein(Wy.abs(), ag, dWx) + ein(dWy, ag, dWx) + (h + w + 4) * U * ein(Wy.abs(), ag, Wx.abs())
    tiles = g.view(h // window, window, w // window, window, C)
    dwin = tiles.sum((0, 2)).permute(2, 0, 1)
    bwin = sum_bound((h // window) * (w // window), tiles.abs().sum((0, 2)).permute(2, 0, 1))
    return (ref, dwin), (bound, bwin)


# ---------------------------------------------------------------------------------------------------------------------------------
def bce_logits_bound(x, y, pos_weight, loss0=0.0):
    """msam2_bce_logits -> ((loss, dx), (b_loss, b_dx)).  softplus(v) = max(v, 0) + log1p(exp(-|v|)): __expf within EXP_ABS of a value
    <= 1, log1pf (slope <= 1) within 2 ulps of a value <= log 2, the sum one rounding; softplus(-v) = softplus(v) - v one more.  Each term
    pw t sp(-v) + (1 - t) sp(v): four products / differences and a sum.  The loss: n + 3 operations (the value already there, 1 / n, the
    product) in any order.  The gradient: sigmoid within SIGMOID_ABS, then (s - 1), the products, the sum, 1 / n."""
    n = x.numel()
    sp_pos = x.clamp(min=0) + torch.log1p(torch.exp(-x.abs()))
    sp_neg = sp_pos - x
    d_pos = EXP_ABS + 4 * U * math.log(2.0) + U * sp_pos
    d_neg = d_pos + U * sp_neg.abs() + U * sp_pos
    a, b = pos_weight * y, 1.0 - y
    term = a * sp_neg + b * sp_pos
    dterm = a.abs() * d_neg + b.abs() * d_pos + 4 * U * ((a * sp_neg).abs() + (b * sp_pos).abs())
    loss = loss0 + term.sum() / n
    b_loss = sum_bound(n + 3, abs(loss0) + term.abs().sum() / n, dterm.sum() / n)
    s = torch.sigmoid(x)
    dx = (a * (s - 1.0) + b * s) / n
    b_dx = ((a.abs() + b.abs()) * SIGMOID_ABS + 6 * U * ((a * (s - 1.0)).abs() + (b * s).abs())) / n
    return (loss, dx), (b_loss, b_dx)


def f32(v):
    """the value a float argument of a C entry has after its conversion to fp32"""
    return float(torch.tensor(v, dtype=torch.float32))


def adam_bound(p, g, m, v, lr, b1, b2, eps, step, gscale=1.0, wd=0.0, device_pow=False):
    """msam2_adam_step / _multi on float64 copies of the fp32 state (lr, b1, b2, eps, gscale, wd as the fp32 values the entry receives)
    -> ((p', m', v'), (b_p, b_m, b_v)).  The chain of roundings: gi = g gscale; m' = b1 m + (1 - b1) gi (four); v' = b2 v + (1 - b2) gi^2
    (five); the bias corrections 1 - b^t: powf within 2 ulps on the host, on the device exp2(t log2 b) with a 4-ulp logarithm, its
    product and the exponential; mhat = m' / bc1, vhat = v' / bc2, sqrt, + eps, the quotient, lr, p decay - update."""
    gi = g * gscale
    m2 = b1 * m + (1 - b1) * gi
    dm = 5 * U * ((b1 * m).abs() + ((1 - b1) * gi).abs())
    v2 = b2 * v + (1 - b2) * gi * gi
    dv = 7 * U * ((b2 * v).abs() + (1 - b2) * gi * gi)

    def bc(b):
        pw = b ** step
        arg = step * abs(math.log2(b))
        dpw = pw * (math.log(2.0) * (4 * U * arg + U * arg) * 2 + 4 * U) if device_pow else 2 * U * pw
        return 1.0 - pw, dpw + U * (1.0 - pw)
    bc1, dbc1 = bc(b1)
    bc2, dbc2 = bc(b2)
    mh = m2 / bc1
    dmh = dm / (bc1 - dbc1) + mh.abs() * (dbc1 / (bc1 - dbc1) + U)
    vh = v2 / bc2
    dvh = dv / (bc2 - dbc2) + vh * (dbc2 / (bc2 - dbc2) + U)
    rt = torch.sqrt(vh)
    drt = torch.sqrt(vh + dvh) - rt + U * rt
    den = rt + eps
    dden = drt + U * den
    upd = lr * mh / den
    den_lo = (den - dden).clamp(min=1e-300)
    dupd = lr * (dmh / den_lo + mh.abs() * dden / (den * den_lo)) + 3 * U * upd.abs()
    decay = 1.0 - lr * wd
    p2 = p * decay - upd
    dp = dupd + 3 * U * (p * decay).abs() + U * p2.abs()
    return (p2, m2, v2), (dp, dm, dv)


# ---------------------------------------------------------------------------------------------------------------------------------
def dropout_bound(x, keep, p, res=None, out16=False, fp16=True):
    """msam2_dropout: y = keep ? x * fl(1 / (1 - p)) : 0 (+ res) with p the fp32 value the entry receives: 1 - p is rounded at the size of 1
    (relative error U / (1 - p)), then the reciprocal and the product, one rounding each; p = 0 multiplies by exactly 1; the sum with
    the residual one rounding.  The 16-bit store saturates in the fp16 build."""
    ik = 1.0 / (1.0 - f32(p))
    v = torch.where(keep, x * ik, torch.zeros_like(x))
    e = (0.0 if p == 0 else U * ik + 2 * U) * v.abs()
    if res is not None:
        v = v + res
        e = e + U * v.abs()
    if not out16:
        return v, e
    if fp16:
        v = v.clamp(-OP16_MAX, OP16_MAX)
    return v, store16(v, e, fp16)


def dropout_keep_np(seed, idx, thr):
    """numpy uint64 restatement of dropout_keep (csrc/common.h): splitmix64 of seed + idx * golden, upper half >= thr"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + idx.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return (z >> np.uint64(32)) >= np.uint64(thr)


def dropout_thr(p):
    """the 32-bit threshold msam2_dropout derives from its fp32 argument p"""
    return int(min(4294967295.0, f32(p) * 4294967296.0))
