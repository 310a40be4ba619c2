"""mlp_rowln_kernel (GPU): the MLP of a Hiera stage-3 block, its residual add and the next LayerNorm as one kernel (ops.mlp_residual_layernorm)
against the two launches it replaces on the same operands: ops.gemm(act=GELU) -> ops.gemm_residual_layernorm (fc1 launched with at least
256 rows, so that it runs the kernels of the step: fc1_as_the_step_runs_it).

Every comparison with the launches is same_bits: the kernel takes k ascending in 16-wide MFMA steps in both GEMMs, rounds the hidden
activations to the operand type where fc1's store does, and restates the row kernel's epilogue.  Shapes: M = 1 (a lone row),
65 (one row in a second tile), 200 (three full tiles and one of 8 rows); H = 128 (one chunk), 256 (the chunk-to-chunk hand-over of the ring
and the hidden image), 1536 (the product's).
"""
import os as _os
import subprocess
import sys as _sys

import pytest
import torch

_sys.path.insert(0, _os.path.dirname(_os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

from helpers import ROOT, Canvas, btol, nan_padded, same_bits  # noqa: E402

DEV = "cuda"
N = 384
EPS = 1e-6
MS = (1, 65, 200)
HS = (128, 256, 1536)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import medical_sam2_amd.ops as ops_mod
    return ops_mod


_INPUTS = {}


def inputs(ops, M, H):
    """(a, w1, b1, w2, b2, r, gamma, beta) of a case on the device, built once: seeded randn; the residual rows carry an offset and a scale
    spread over two decades (tests/test_memattn_tail_gpu.py), so that a row's mean and variance matter"""
    if (M, H) not in _INPUTS:
        g = torch.Generator().manual_seed(9000 * H + M)
        a = torch.randn(M, N, generator=g).to(ops.OP16)
        w1 = (torch.randn(H, N, generator=g) * N ** -0.5).to(ops.OP16)
        b1 = torch.randn(H, generator=g) * 0.5
        w2 = (torch.randn(N, H, generator=g) * H ** -0.5).to(ops.OP16)
        b2 = torch.randn(N, generator=g) * 0.5
        scale = 10.0 ** (torch.rand(M, 1, generator=g) * 2 - 1)
        r = torch.randn(M, N, generator=g) * scale + torch.randn(M, 1, generator=g) * 3
        gamma = torch.randn(N, generator=g)
        beta = torch.randn(N, generator=g)
        _INPUTS[(M, H)] = tuple(t.to(DEV) for t in (a, w1, b1, w2, b2, r, gamma, beta))
    return _INPUTS[(M, H)]


_REF = {}


def fc1_as_the_step_runs_it(ops, a, w1, b1):
    """ops.gemm(act=GELU) on the rows of a, launched with at least 256 rows (zero rows appended, their outputs dropped): from 256 rows upward
    gemm_launch takes the LDS-DMA kernels the step runs, which sum k ascending in 16-wide MFMA steps; below, it takes kernels with another
    summation order (M <= 32: gemm_skinny_kernel splits K over four waves), whose hidden activations differ from the product's by an ulp of
    the 16-bit type here and there.  A GEMM's rows are independent, so the appended rows change nothing in the rows compared
    (tests/test_gemm_layernorm_gpu.py compares at M = 256 for the same reason)."""
    M = a.shape[0]
    if M >= 256:
        return ops.gemm(a, w1, b1, act=ops.ACT_GELU)
    ap = torch.zeros(256, a.shape[1], dtype=a.dtype, device=a.device)
    ap[:M] = a
    return ops.gemm(ap, w1, b1, act=ops.ACT_GELU)[:M]


def two_launches(ops, M, H, with_bias=True):
    """(c32, y16) of the product's two launches, computed once per case and left unchanged"""
    key = (M, H, with_bias)
    if key not in _REF:
        a, w1, b1, w2, b2, r, gamma, beta = inputs(ops, M, H)
        hid = fc1_as_the_step_runs_it(ops, a, w1, b1 if with_bias else None)
        _REF[key] = ops.gemm_residual_layernorm(hid, w2, b2 if with_bias else None, r, gamma, beta, EPS)
    return _REF[key]


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("H", HS)
def test_has_the_bits_of_the_two_launches(ops, H, M, with_bias):
    """operands inside NaN-filled buffers with leading dimensions larger than the row, outputs inside sentinel-filled canvases"""
    assert ops.mlp_residual_layernorm_supported(N, H)
    a, w1, b1, w2, b2, r, gamma, beta = inputs(ops, M, H)
    av = nan_padded(M, N, N + 8, ops.OP16, a)               # lda > N
    w1v = nan_padded(H, N, N + 8, ops.OP16, w1)             # ldw1 > N
    w2v = nan_padded(N, H, H + 16, ops.OP16, w2)            # ldw2 > H
    rv = nan_padded(M, N, N + 4, torch.float32, r)          # ldr > N
    c, y = Canvas(M, N, torch.float32), Canvas(M, N, ops.OP16)   # ldc, ldy > N
    ops.mlp_residual_layernorm(av, w1v, b1 if with_bias else None, w2v, b2 if with_bias else None, rv, gamma, beta, EPS, out=c.view, out16=y.view)
    assert c.sentinels_intact() and y.sentinels_intact(), "wrote outside an output view (padding columns, or rows past M)"
    c_ref, y_ref = two_launches(ops, M, H, with_bias)
    c32, y16 = c.view.contiguous(), y.view.contiguous()
    print(f"mlp_rowln {M}x{N}x{H} bias={with_bias}: max |C32 - launches| {(c32 - c_ref).abs().max().item():.3e}, "
          f"{int((y16.view(torch.int16) != y_ref.view(torch.int16)).sum())} of {y16.numel()} Y16 elements differ")
    same_bits(c32, c_ref, f"C32 {M}x{N}x{H} against gemm(GELU) -> gemm_residual_layernorm")
    same_bits(y16, y_ref, f"Y16 {M}x{N}x{H} against gemm(GELU) -> gemm_residual_layernorm")


def test_product_shape_has_the_bits_of_the_kernels_the_step_runs(ops):
    """B = 4: 16384 rows, where ops.gemm takes gemm_wstat_kernel and every CU owns one tile (the W prefetch's 32 workgroups per XCD)"""
    M, H = 16384, 1536
    a, w1, b1, w2, b2, r, gamma, beta = inputs(ops, M, H)
    c, y = ops.mlp_residual_layernorm(a, w1, b1, w2, b2, r, gamma, beta, EPS)
    c_ref, y_ref = ops.gemm_residual_layernorm(ops.gemm(a, w1, b1, act=ops.ACT_GELU), w2, b2, r, gamma, beta, EPS)
    print(f"mlp_rowln {M}x{N}x{H}: max |C32 - launches| {(c - c_ref).abs().max().item():.3e}, "
          f"{int((y.view(torch.int16) != y_ref.view(torch.int16)).sum())} of {y.numel()} Y16 elements differ")
    same_bits(c, c_ref, f"C32 {M}x{N}x{H} against gemm(GELU) -> gemm_residual_layernorm")
    same_bits(y, y_ref, f"Y16 {M}x{N}x{H} against gemm(GELU) -> gemm_residual_layernorm")
    del _INPUTS[(M, H)]


def test_second_stream_and_graph_replay(ops):
    M, H = 200, 256
    a, w1, b1, w2, b2, r, gamma, beta = inputs(ops, M, H)
    c_ref, y_ref = two_launches(ops, M, H)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c, y = ops.mlp_residual_layernorm(a, w1, b1, w2, b2, r, gamma, beta, EPS)
    s.synchronize()
    same_bits(c, c_ref, "C32 on a second stream")
    same_bits(y, y_ref, "Y16 on a second stream")
    c, y = torch.zeros_like(c_ref), torch.zeros_like(y_ref)
    ops.mlp_residual_layernorm(a, w1, b1, w2, b2, r, gamma, beta, EPS, out=c, out16=y)   # the kernel's LDS limit is raised outside the capture
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        ops.mlp_residual_layernorm(a, w1, b1, w2, b2, r, gamma, beta, EPS, out=c, out16=y)
    for i in range(2):
        c.zero_()
        y.zero_()
        gr.replay()
        torch.cuda.synchronize()
        same_bits(c, c_ref, f"C32, graph replay {i}")
        same_bits(y, y_ref, f"Y16, graph replay {i}")


def test_against_fp32_restatement(ops):
    """sanity against torch in fp32 on the same 16-bit weights, at test_ln_mlp_residual_fused's bound for the fused MLP against its oracle
    (tests/test_kernels_gpu.py: atol btol(6e-3), rtol btol(4e-3)): two 16-bit roundings, the input rows and the hidden activations"""
    M, H = 200, 1536
    a, w1, b1, w2, b2, r, gamma, beta = inputs(ops, M, H)
    c, y = ops.mlp_residual_layernorm(a, w1, b1, w2, b2, r, gamma, beta, EPS)
    hid = torch.nn.functional.gelu(a.float() @ w1.float().t() + b1)
    ref = hid @ w2.float().t() + b2 + r
    err, lim = (c - ref).abs(), btol(6e-3) + btol(4e-3) * ref.abs()
    print(f"C32 against fp32 torch: max |err| {err.max().item():.3e}, {(err / lim).max().item():.3f} of the bound")
    assert bool((err <= lim).all()), f"C32 against fp32 torch: max err {err.max().item():.4g}, {int((err > lim).sum())} bad of {err.numel()}"
    alone = ops.layernorm(c, gamma, beta, EPS)
    same_bits(y, alone, "Y16 against ops.layernorm on the kernel's own rows")


def test_supported_and_refusals(ops):
    assert all(ops.mlp_residual_layernorm_supported(N, h) for h in HS)
    M = 65
    a, w1, b1, w2, b2, r, gamma, beta = inputs(ops, M, 128)
    z = lambda *s: torch.zeros(*s, dtype=ops.OP16, device=DEV)
    with pytest.raises(ValueError, match=r"N = 384, H = 192 is not built \(N = 384 with H % 128 == 0\)"):
        ops.mlp_residual_layernorm(a, z(192, N), None, z(N, 192), None, r, gamma, beta, EPS)
    with pytest.raises(ValueError, match=r"N = 256, H = 1024 is not built"):
        ops.mlp_residual_layernorm(z(M, 256), z(1024, 256), None, z(256, 1024), None, torch.zeros(M, 256, device=DEV), gamma[:256].contiguous(),
                                   beta[:256].contiguous(), EPS)
    with pytest.raises(ValueError, match=r"mlp_residual_layernorm shapes"):
        ops.mlp_residual_layernorm(a, w1, b1, z(N, 256), b2, r, gamma, beta, EPS)
    with pytest.raises(RuntimeError, match=r"mlp_residual_layernorm: A, W1, W2, b1, b2, R32, C32, ln_w, ln_b must be 16-byte aligned"):
        ops.mlp_residual_layernorm(a, w1, torch.zeros(129, device=DEV)[1:], w2, b2, r, gamma, beta, EPS)
    with pytest.raises(RuntimeError, match=r"mlp_residual_layernorm: lda, ldw1, ldw2 must be multiples of 8"):
        ops.mlp_residual_layernorm(z(M, N + 4)[:, :N], w1, b1, w2, b2, r, gamma, beta, EPS)


# ---- the trunk: the switch is read when the module is imported, so each setting runs in a fresh child process
CHILD = r"""
import sys, torch
sys.path.insert(0, {root!r})
import medical_sam2_amd.ops as ops
from medical_sam2_amd.modeling.encoder import Hiera
torch.set_grad_enabled(False)
torch.manual_seed(21)
trunk = Hiera(embed_dim=96, num_heads=1, stages=(1, 1, 3, 1), global_att_blocks=(3,), window_spec=(8, 4, 14, 7))
for mod in trunk.modules():                                  # LayerNorms that do something
    if isinstance(mod, torch.nn.LayerNorm):
        torch.nn.init.normal_(mod.weight, 1.0, 0.3)
        torch.nn.init.normal_(mod.bias, 0.0, 0.3)
trunk = trunk.cuda().eval()
calls = []
real = ops.mlp_residual_layernorm
ops.mlp_residual_layernorm = lambda *a, **k: (calls.append((a[0].shape[0], a[1].shape[0])), real(*a, **k))[1]
x = torch.randn(1, 3, {side}, {side}, generator=torch.Generator().manual_seed(22)).cuda()
outs = trunk(x)
torch.cuda.synchronize()
torch.save(dict(outs=[o.float().cpu() for o in outs], calls=calls), {path!r})
"""
SIDE = 544     # stage 3 is 34 x 34 = 1156 tokens: eighteen 64-row tiles and one of 4 rows, above the dispatch's token gate


def _trunk_child(tmp_path, name, env_extra):
    path = str(tmp_path / f"{name}.pt")
    env = dict(_os.environ)
    env.pop("MSAM2_NO_FUSED_MLP_LN", None)
    env.update(env_extra)
    proc = subprocess.run([_sys.executable, "-c", CHILD.format(root=ROOT, side=SIDE, path=path)], env=env, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    return torch.load(path)


def test_trunk_fused_vs_switched_off(ops, tmp_path):
    on = _trunk_child(tmp_path, "on", {})
    off = _trunk_child(tmp_path, "off", {"MSAM2_NO_FUSED_MLP_LN": "1"})
    assert off["calls"] == [] and on["calls"] == [(1156, 1536)] * 3, (on["calls"], off["calls"])   # the three dim-384 blocks, one launch each
    assert len(on["outs"]) == len(off["outs"]) > 0
    for i, (p, q) in enumerate(zip(on["outs"], off["outs"])):
        assert bool(torch.isfinite(p).all())
        print(f"trunk output {i} {tuple(p.shape)}: max |diff| {(p - q).abs().max().item():.3e}")
        same_bits(p, q, f"trunk output {i}, fused MLP against MSAM2_NO_FUSED_MLP_LN=1")
