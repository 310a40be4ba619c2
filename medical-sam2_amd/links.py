"""What the three drivers of the explicit backward share: `training.py` (the 2-D step: calibrates once, then runs frozen scales inside a
captured graph), `training_3d.py` (BPTT over a tape) and `autograd.py` (torch.autograd.Function wrappers), the last two eager with
one host read per link.  Every 16-bit backward operand runs under a power-of-two scale and is un-scaled in fp32; the rules that pick
those scales -- and with them whether an operand saturates or flushes to zero -- are stated here once."""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from . import backward as bwd
from .ops import F32


def pow2_scale(amax: float) -> float:
    """the power of two that brings max|gradient| = amax into (2^-4, 2^-3]; 1 for a zero or non-finite maximum"""
    return 2.0 ** (-3 - math.ceil(math.log2(amax))) if amax > 0 and math.isfinite(amax) else 1.0


def amax_of(t: torch.Tensor) -> float:
    """max|t| -- ONE HOST READ: for the eager drivers and a calibrating call only, never on a path that a captured step takes"""
    return float(t.detach().abs().max().item())


def pow2_scale_of(t: torch.Tensor) -> float:
    """`pow2_scale` of max|t| (one host read, see `amax_of`)"""
    return pow2_scale(amax_of(t))


def bce_loss_scale(n_loss: int, pos_weight: float, upsampled: bool) -> float:
    """Fixed loss scale of the mean BCE over n_loss elements.  |dloss/dlogit| <= max(pos_weight, 1) / n is ~1e-6 at 1024^2 -- below the
    16-bit operand's normal range (fp16: 6e-5).  A power of two that depends on no data (so the step stays capturable) brings the largest
    entry to 2^-4; the backward is linear in d_masks and the update kernel multiplies the gradients by the inverse.
    upsampled (the loss on one mask at the video resolution): the up-sampling adjoint sums ~16 elements per low-res pixel, 2^-4 more
    keeps that sum <= 2^0."""
    return 2.0 ** (math.floor(math.log2(n_loss / max(float(pos_weight), 1.0))) - 4 - (4 if upsampled else 0))


def accumulate(dst: Dict[str, torch.Tensor], src: Dict[str, torch.Tensor], factor: float = 1.0) -> None:
    """dst[k] = dst[k] + src[k] * factor in fp32 (in this order; a key new to dst takes src[k] * factor)"""
    for k, v in src.items():
        g = v.to(F32)
        if factor != 1.0:
            g = g * factor
        dst[k] = dst[k] + g if k in dst else g


def decoder_link(args: tuple, d_masks: Optional[torch.Tensor], d_tokens: Optional[torch.Tensor], backward=bwd.mask_decoder_backward):
    """The mask decoder's backward under its two upstream gradients: d_masks [B, nm, 4h, 4w] on the mask logits and d_tokens [B, nm, C] on
    the mask tokens (the object-pointer path), either may be None.  args = (dec, src, pe, sparse, f0, f1, B, h, w) as for `backward`.
    One scale s_d for both, chosen from the MASK gradient: it is the one that enters as a 16-bit GEMM operand right away (d_masks against
    the up-scaled features), and a mean-reduced BCE gradient scaled by anything much larger's maximum would land in fp16's subnormals.
    The token gradient is added in fp32 to the hyper-network path's result before anything is rounded, so it only has to stay inside the
    16-bit RANGE: if it would not (a_t * s_d > 1024), the two are back-propagated separately under their own scales and recombined in
    fp32 -- the decoder backward is linear.
    Returns None when both gradients are absent or all zero (nothing to do), else (d_src, d_sparse, {parameter: gradient}, aux with
    "d_feat_s0" / "d_feat_s1", s_d), everything still carrying s_d.  Host reads: max|d_masks|, max|d_tokens| and one per scale."""
    dec, src, B, h, w = args[0], args[1], args[6], args[7], args[8]
    a_m = amax_of(d_masks) if d_masks is not None else 0.0
    a_t = amax_of(d_tokens) if d_tokens is not None else 0.0
    if a_m == 0.0 and a_t == 0.0:
        return None
    dm = d_masks.to(F32).contiguous() if a_m > 0 else torch.zeros(B, dec.num_mask_tokens, 4 * h, 4 * w, dtype=F32, device=src.device)
    dt = d_tokens.to(F32).contiguous() if a_t > 0 else None
    s_d = pow2_scale_of(dm) if a_m > 0 else pow2_scale_of(dt)
    aux: dict = {}
    if a_m > 0 and a_t * s_d > 1024.0:
        d_src, d_sparse, g = backward(*args, dm * s_d, aux=aux)
        s_t = pow2_scale_of(dt)
        aux2: dict = {}
        d_src2, d_sparse2, g2 = backward(*args, torch.zeros_like(dm), aux=aux2, d_mask_tokens=dt * s_t)
        r = s_d / s_t
        d_src, d_sparse = d_src + d_src2 * r, d_sparse + d_sparse2 * r
        accumulate(g, g2, r)
        accumulate(aux, aux2, r)
    else:
        d_src, d_sparse, g = backward(*args, dm * s_d, aux=aux, d_mask_tokens=None if dt is None else dt * s_d)
    return d_src, d_sparse, g, aux, s_d
