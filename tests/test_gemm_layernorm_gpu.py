"""gemm_rowln_kernel (GPU): a residual-stream GEMM of Hiera stage 3 with the LayerNorm that follows it in its epilogue
(ops.gemm_residual_layernorm), against float64, against the two launches it replaces, and at module level.

Bounds.  C32: error_bound() of tests/test_gemm_variants_gpu.py for an fp32 output with bias and fp32 residual (K fp32 additions).  Against
the product path (ops.gemm with an fp32 residual at M = 256, where gemm_launch takes the LDS-DMA kernels the step runs) and against
ops.layernorm on the fused kernel's own fp32 rows: the same bits -- the kernel accumulates k in their order and restates their arithmetic.
"""
import os as _os
import sys as _sys

import pytest
import torch

_sys.path.insert(0, _os.path.dirname(_os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

from helpers import Canvas, nan_padded, op16_is_fp16, same_bits, within  # noqa: E402
from test_gemm_variants_gpu import error_bound  # noqa: E402

DEV = "cuda"
N = 384
EPS = 1e-6
# (M, K): one tile with fewer k-steps than the ring is deep; the prefetch-distance boundary; a single live row; three full tiles and one of
# 8 rows; the product K of proj and of fc2 at the smallest M where gemm_launch takes the DMA kernels; a ragged tile behind nine full ones
CASES = [(64, 64), (64, 128), (1, 384), (200, 384), (256, 384), (256, 1536), (64 * 9 + 33, 1536)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import medical_sam2_amd.ops as ops_mod
    return ops_mod


_INPUTS = {}


def inputs(ops, M, K):
    """(a, w, bias, r, gamma, beta) of a case on the device, built once: seeded randn; the residual rows carry an offset and a scale spread
    over two decades, so that a row's mean and variance matter"""
    if (M, K) not in _INPUTS:
        g = torch.Generator().manual_seed(1000 * K + M)
        a = torch.randn(M, K, generator=g).to(ops.OP16)
        w = (torch.randn(N, K, generator=g) * K ** -0.5).to(ops.OP16)
        bias = torch.randn(N, generator=g) * 0.5
        scale = 10.0 ** (torch.rand(M, 1, generator=g) * 2 - 1)
        r = torch.randn(M, N, generator=g) * scale + torch.randn(M, 1, generator=g) * 3
        gamma = torch.randn(N, generator=g)
        beta = torch.randn(N, generator=g)
        _INPUTS[(M, K)] = tuple(t.to(DEV) for t in (a, w, bias, r, gamma, beta))
    return _INPUTS[(M, K)]


def fused_in_canvases(ops, M, K):
    """the op on operands inside NaN-filled buffers (lda > K, ldr > N) with outputs inside sentinel-filled ones (ldc, ldy > N)"""
    a, w, bias, r, gamma, beta = inputs(ops, M, K)
    av = nan_padded(M, K, K + 8, ops.OP16, a)
    rv = nan_padded(M, N, N + 4, torch.float32, r)
    c, y = Canvas(M, N, torch.float32), Canvas(M, N, ops.OP16)
    ops.gemm_residual_layernorm(av, w, bias, rv, gamma, beta, EPS, out=c.view, out16=y.view)
    return c, y


@pytest.mark.parametrize("M,K", CASES)
def test_fused_vs_float64_and_standalone_layernorm(ops, M, K):
    assert ops.gemm_residual_layernorm_supported(N, K)
    a, w, bias, r, gamma, beta = inputs(ops, M, K)
    c, y = fused_in_canvases(ops, M, K)
    assert c.sentinels_intact() and y.sentinels_intact(), "wrote outside an output view (padding columns, or rows past M)"
    c32, y16 = c.view.contiguous(), y.view.contiguous()
    assert bool(torch.isfinite(c32).all()) and bool(torch.isfinite(y16.float()).all()), "operand padding (NaN) reached an output"
    a64, w64 = a.double(), w.double()
    pre = a64 @ w64.t() + bias.double()
    ref = pre + r.double()
    bound = error_bound(a64.abs() @ w64.abs().t(), K, pre, ref, fp16=op16_is_fp16())
    err = (c32.double() - ref).abs()
    print(f"C32 {M}x{N}x{K}: max |err| {err.max().item():.3e}, {(err / bound).max().item():.3f} of the bound")
    within(c32, ref, bound, f"C32 {M}x{N}x{K} against float64")
    alone = ops.layernorm(c32, gamma, beta, EPS)
    ne = int((alone.view(torch.int16) != y16.view(torch.int16)).sum())
    print(f"Y16 {M}x{N}x{K}: {ne} of {y16.numel()} elements differ from ops.layernorm on the same rows")
    same_bits(y16, alone, f"Y16 {M}x{N}x{K} against the stand-alone LayerNorm kernel")
    c2, y2 = fused_in_canvases(ops, M, K)
    assert torch.equal(c.bits(), c2.bits()) and torch.equal(y.bits(), y2.bits()), "two launches differ"


@pytest.mark.parametrize("K", [384, 1536])
def test_c32_has_the_bits_of_the_product_path(ops, K):
    M = 256
    a, w, bias, r, gamma, beta = inputs(ops, M, K)
    c32, _ = ops.gemm_residual_layernorm(a, w, bias, r, gamma, beta, EPS)
    old = ops.gemm(a, w, bias, residual=r, out_dtype=torch.float32)
    print(f"C32 {M}x{N}x{K} vs ops.gemm: max |diff| {(c32 - old).abs().max().item():.3e}")
    same_bits(c32, old, f"C32 {M}x{N}x{K} against ops.gemm with an fp32 residual")


def test_supported_and_refusals(ops):
    assert ops.gemm_residual_layernorm_supported(384, 384) and ops.gemm_residual_layernorm_supported(384, 1536)
    for n, k in [(256, 384), (768, 384), (384, 96)]:
        assert not ops.gemm_residual_layernorm_supported(n, k)
        a = torch.zeros(64, k, dtype=ops.OP16, device=DEV)
        w = torch.zeros(n, k, dtype=ops.OP16, device=DEV)
        v = torch.zeros(n, device=DEV)
        with pytest.raises((ValueError, RuntimeError)):
            ops.gemm_residual_layernorm(a, w, v, torch.zeros(64, n, device=DEV), v, v, EPS)


def _chain(blocks, t, B, H, W):
    """the two blocks as Hiera.forward chains them: block 0 is handed block 1's norm1, block 1 the rows block 0's fc2 left for it"""
    from medical_sam2_amd.modeling.common import v_f32
    b0, b1 = blocks
    nn1 = (v_f32(b1._wc, "n1w", b1.norm1.weight), v_f32(b1._wc, "n1b", b1.norm1.bias), 1e-6)
    with torch.no_grad():
        t1, h, w = b0.run(t, B, H, W, fused_gemm_ln=True, next_norm=nn1)
        xn, b0.next_xn = b0.next_xn, None
        return b1.run(t1, B, h, w, fused_gemm_ln=True, xn=xn)[0], xn


def test_two_block_chain_fused_vs_switched_off(ops, monkeypatch):
    """a window block and a global block of dim 384 at 16 x 16 tokens (M = 256: the product path's DMA GEMM kernels): same fp32 tokens"""
    import medical_sam2_amd.modeling.encoder as enc
    from medical_sam2_amd.modeling.encoder import MultiScaleBlock
    torch.manual_seed(3)
    blocks = [MultiScaleBlock(dim=384, dim_out=384, num_heads=4, window_size=ws).to(DEV).eval() for ws in (8, 0)]
    for b in blocks:                                            # LayerNorms that do something
        for ln in (b.norm1, b.norm2):
            torch.nn.init.normal_(ln.weight, 1.0, 0.3)
            torch.nn.init.normal_(ln.bias, 0.0, 0.3)
    B, H, W = 1, 16, 16
    t = torch.randn(B * H * W, 384, generator=torch.Generator().manual_seed(5)).to(DEV)
    calls = []
    real = ops.gemm_residual_layernorm
    monkeypatch.setattr(ops, "gemm_residual_layernorm", lambda *a, **k: (calls.append(a[0].shape[1]), real(*a, **k))[1])
    monkeypatch.setattr(enc, "_FUSED_GEMM_LN", False)
    off, xn_off = _chain(blocks, t, B, H, W)
    assert not calls and xn_off is None
    monkeypatch.setattr(enc, "_FUSED_GEMM_LN", True)
    monkeypatch.setattr(enc, "_FUSED_GEMM_LN_K", frozenset((384, 1536)))
    on, xn_on = _chain(blocks, t, B, H, W)
    assert calls == [384, 1536, 384] and xn_on is not None      # proj and fc2 of block 0, proj of block 1 (nobody follows its fc2)
    print(f"chain, fused vs switched off: max |diff| {(on - off).abs().max().item():.3e}")
    same_bits(on, off, "two-block chain, fused vs switched off")
    del calls[:]
    with torch.no_grad():                                       # the training forward's call form never asks
        plain = blocks[1].run(blocks[0].run(t, B, H, W)[0], B, H, W)[0]
    assert not calls
    same_bits(plain, off, "two-block chain, plain call form")
