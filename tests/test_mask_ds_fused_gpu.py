"""conv3x3s2_mfma_kernel (GPU): a stage of the mask down-sampler as one implicit-GEMM kernel with bias + LayerNorm2d + GELU in its epilogue
(ops.conv3x3s2_mfma_ln_gelu), against the three launches it replaces, against float64, and at module level.

Against ops.im2col3x3s2 -> ops.gemm(out_dtype=F32) -> ops.layernorm(act=GELU) on the same tensors: the same bits -- the kernel accumulates k
in the order of the GEMM kernel that serves the shape (gemm_skinny_kernel's four partial sums at M <= 32 and K % 16 == 0 included) and
restates layernorm_kernel's arithmetic.  Against float64: the bound the three-launch path has, error_bound() of
tests/test_gemm_variants_gpu.py for the fp32 pre-norm map (K fp32 additions and the bias) carried through pointwise_bounds.ln_tail and the
GELU + 16-bit store of layernorm_bound -- a sanity check on the shared path, not a new tolerance.
"""
import os as _os
import sys as _sys

import pytest
import torch
import torch.nn.functional as F

_sys.path.insert(0, _os.path.dirname(_os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

import pointwise_bounds as PB  # noqa: E402
from helpers import Canvas, nan_guarded, op16_is_fp16, same_bits, within  # noqa: E402
from test_gemm_variants_gpu import error_bound  # noqa: E402

DEV = "cuda"
EPS = 1e-6
# (B, H, W, Cin): one output pixel, every border tap; non-square, fewer pixels than one wave block; batch seam, ragged (30 pixels, K = 144:
# the GEMM of the three launches is the skinny kernel); 306 pixels, a ragged block behind full ones; K = 576, 36 k-steps; several workgroups
CASES = [(1, 2, 2, 4), (1, 4, 6, 4), (2, 6, 10, 16), (2, 18, 34, 16), (3, 16, 16, 64), (1, 64, 64, 4)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import medical_sam2_amd.ops as ops_mod
    return ops_mod


_INPUTS = {}


def inputs(ops, B, H, W, cin):
    """(x NHWC 16-bit, conv weight fp32 [cout, cin, 3, 3] rounded to 16 bits, packed weight, bias, gamma, beta) on the device, built once:
    seeded; the input carries an offset and a per-pixel scale so that a row's mean and variance matter"""
    key = (B, H, W, cin)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(100000 * cin + 1000 * H + 10 * W + B)
        cout = 4 * cin
        x = (torch.randn(B, H, W, cin, generator=g) * (0.5 + torch.rand(B, H, W, 1, generator=g)) + 0.3).to(ops.OP16)
        w = (torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5).to(ops.OP16)
        ld = (9 * cin + 7) // 8 * 8
        wp = torch.zeros(cout, ld, dtype=ops.OP16)
        wp[:, :9 * cin] = w.permute(0, 2, 3, 1).reshape(cout, -1)
        bias = torch.randn(cout, generator=g) * 0.5
        gamma = 1.0 + 0.3 * torch.randn(cout, generator=g)
        beta = 0.3 * torch.randn(cout, generator=g)
        _INPUTS[key] = tuple(t.to(DEV) for t in (x, w.float(), wp, bias, gamma, beta))
    return _INPUTS[key]


def three_launches(ops, x, B, H, W, wp, bias, gamma, beta):
    cols = ops.im2col3x3s2(x.reshape(B * H * W, -1), B, H, W)
    g = ops.gemm(cols, wp, bias, out_dtype=torch.float32)
    return ops.layernorm(g, gamma, beta, EPS, act=ops.ACT_GELU)


def fused_in_canvas(ops, B, H, W, cin):
    """the op on an input inside NaN guards with its output inside a sentinel canvas"""
    x, _, wp, bias, gamma, beta = inputs(ops, B, H, W, cin)
    xv = nan_guarded(x)
    y = Canvas(B * (H // 2) * (W // 2), 4 * cin, ops.OP16)
    ops.conv3x3s2_mfma_ln_gelu(xv.reshape(B * H * W, cin), B, H, W, wp, bias, gamma, beta, EPS, out=y.view)
    return y


@pytest.mark.parametrize("B,H,W,cin", CASES)
def test_fused_vs_three_launches_and_float64(ops, B, H, W, cin):
    cout = 4 * cin
    assert ops.conv3x3s2_mfma_ln_gelu_supported(cin, cout)
    x, w, wp, bias, gamma, beta = inputs(ops, B, H, W, cin)
    y = fused_in_canvas(ops, B, H, W, cin)
    assert y.sentinels_intact(), "wrote outside the output view (padding columns, or rows past the last pixel)"
    y16 = y.view.contiguous()
    assert bool(torch.isfinite(y16.float()).all()), "a NaN guard around the input reached the output (a tap outside the tensor)"
    old = three_launches(ops, x, B, H, W, wp, bias, gamma, beta)
    ne = int((old.view(torch.int16) != y16.view(torch.int16)).sum())
    print(f"{B}x{H}x{W}x{cin}: {ne} of {y16.numel()} elements differ from im2col + gemm + layernorm")
    same_bits(y16, old, f"{B}x{H}x{W}x{cin} against im2col + gemm + layernorm")
    y2 = fused_in_canvas(ops, B, H, W, cin)
    assert torch.equal(y.bits(), y2.bits()), "two launches differ"
    # float64 restatement from the operand-rounded inputs
    x64 = x.double().permute(0, 3, 1, 2)
    nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(-1, cout)
    pre = nhwc(F.conv2d(x64, w.double(), bias.double(), stride=2, padding=1))
    S = nhwc(F.conv2d(x64.abs(), w.double().abs(), None, stride=2, padding=1))
    dpre = error_bound(S, (9 * cin + 7) // 8 * 8, pre, pre, fp16=op16_is_fp16())
    pre2, dpre2 = PB.ln_tail(pre, dpre, gamma.double(), beta.double(), EPS)
    ref, bound = PB.act_store(pre2, dpre2, 1, True, op16_is_fp16())
    err = (y16.double() - ref).abs()
    print(f"{B}x{H}x{W}x{cin}: max |err| {err.max().item():.3e}, {(err / bound).max().item():.3f} of the bound")
    within(y16, ref, bound, f"{B}x{H}x{W}x{cin} against float64")


@pytest.mark.parametrize("B,H,W,cin", [(4, 512, 512, 4), (4, 256, 256, 16), (4, 128, 128, 64)])
def test_benchmark_sizes_same_bits(ops, B, H, W, cin):
    """The stages at the benchmark's sizes (4.2 million outputs each; stage 4's GEMM is the LDS-DMA kernel there), bits only.  A LayerNorm
    or GELU whose multiplies and adds are fused otherwise than layernorm_kernel's moves an fp32 value by an ulp, which reaches the 16-bit
    output once in 2^13 (fp16) or 2^16 (bf16) elements: the small cases above cannot see that, these can."""
    cout = 4 * cin
    g = torch.Generator(device=DEV).manual_seed(cin)
    r = lambda *s: torch.randn(*s, generator=g, device=DEV)
    x = (r(B * H * W, cin) * (0.5 + torch.rand(B * H * W, 1, generator=g, device=DEV)) + 0.3).to(ops.OP16)
    ld = (9 * cin + 7) // 8 * 8
    wp = torch.zeros(cout, ld, dtype=ops.OP16, device=DEV)
    wp[:, :9 * cin] = (r(cout, 9 * cin) * (9 * cin) ** -0.5).to(ops.OP16)
    bias, gamma, beta = r(cout) * 0.5, 1.0 + 0.3 * r(cout), 0.3 * r(cout)
    new = ops.conv3x3s2_mfma_ln_gelu(x, B, H, W, wp, bias, gamma, beta, EPS)
    old = three_launches(ops, x, B, H, W, wp, bias, gamma, beta)
    ne = int((old.view(torch.int16) != new.view(torch.int16)).sum())
    print(f"{B}x{H}x{W}x{cin}: {ne} of {new.numel()} elements differ from im2col + gemm + layernorm")
    same_bits(new, old, f"{B}x{H}x{W}x{cin} against im2col + gemm + layernorm")


def test_supported_and_refusals(ops):
    for cin, cout in [(4, 16), (16, 64), (64, 256)]:
        assert ops.conv3x3s2_mfma_ln_gelu_supported(cin, cout)
    for cin, cout in [(4, 8), (8, 32), (16, 32), (32, 128), (64, 64), (128, 512)]:
        assert not ops.conv3x3s2_mfma_ln_gelu_supported(cin, cout)
        x = torch.zeros(4 * 4, cin, dtype=ops.OP16, device=DEV)
        wp = torch.zeros(cout, (9 * cin + 7) // 8 * 8, dtype=ops.OP16, device=DEV)
        v = torch.zeros(cout, device=DEV)
        with pytest.raises((ValueError, RuntimeError)):
            ops.conv3x3s2_mfma_ln_gelu(x, 1, 4, 4, wp, v, v, v, EPS)


def test_mask_down_sampler_fused_vs_switched_off(ops, monkeypatch):
    """MaskDownSampler.run on a seeded 1 x 1 x 64 x 64 mask: stages 2-4 (256, 64 and 16 output pixels) as one kernel each and as their
    three launches give the same fp32 tokens"""
    import medical_sam2_amd.modeling.memory as mem
    torch.manual_seed(11)
    ds = mem.MaskDownSampler(embed_dim=256, kernel_size=3, stride=2, padding=1, total_stride=16).to(DEV).eval()
    for m in ds.encoder:                                        # LayerNorms that do something
        if isinstance(m, mem.LayerNorm2d):
            torch.nn.init.normal_(m.weight, 1.0, 0.3)
            torch.nn.init.normal_(m.bias, 0.0, 0.3)
    mask = (torch.randn(1, 1, 64, 64, generator=torch.Generator().manual_seed(12)) * 4).to(DEV)
    calls = []
    real = ops.conv3x3s2_mfma_ln_gelu
    monkeypatch.setattr(ops, "conv3x3s2_mfma_ln_gelu", lambda *a, **k: (calls.append(a[4].shape[0]), real(*a, **k))[1])
    with torch.no_grad():
        monkeypatch.setattr(mem, "_FUSED_MASK_DS", False)
        off = ds.run(mask, 1, 1.0, 0.0)
        assert not calls
        monkeypatch.setattr(mem, "_FUSED_MASK_DS", True)
        monkeypatch.setattr(mem, "_FUSED_MASK_DS_STAGES", frozenset((2, 3, 4)))
        on = ds.run(mask, 1, 1.0, 0.0)
    assert calls == [16, 64, 256]
    print(f"mask down-sampler, fused vs switched off: max |diff| {(on - off).abs().max().item():.3e}")
    same_bits(on, off, "MaskDownSampler.run, fused vs switched off")
