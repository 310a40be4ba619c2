"""The tails of a memory-attention layer as one gemm_rowln_kernel each (GPU): ops.gemm_residual_layernorm at N = 256 and
ops.gemm_merged_residual_layernorm (split-KV merge -> out-projection + residual -> LayerNorm), against the launches they replace, and
MemoryAttention.forward with the fusion against MSAM2_NO_FUSED_MEMATTN_TAIL=1.

Every comparison is for equal bits: the kernel takes k in the GEMM kernels' order and restates attn_merge_kernel's and layernorm_kernel's
arithmetic in their order.  The references are the product's own launches on the same operands: ops.attention_merge,
ops.gemm with an fp32 residual, ops.layernorm.
"""
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

from helpers import ROOT, Canvas, nan_padded, same_bits  # noqa: E402

DEV = "cuda"
N = 256
EPS = 1e-5
MS = (200, 65)            # three full 64-row tiles and one of 8 rows; one row in the second tile


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import medical_sam2_amd.ops as ops_mod
    return ops_mod


_ROWS = {}


def row_side(ops, M, K):
    """(w, bias, r, gamma, beta) of a case on the device, built once: the residual rows carry an offset and a scale spread over two decades"""
    if (M, K) not in _ROWS:
        g = torch.Generator().manual_seed(7000 * K + M)
        w = (torch.randn(N, K, generator=g) * K ** -0.5).to(ops.OP16)
        bias = torch.randn(N, generator=g) * 0.5
        scale = 10.0 ** (torch.rand(M, 1, generator=g) * 2 - 1)
        r = torch.randn(M, N, generator=g) * scale + torch.randn(M, 1, generator=g) * 3
        gamma = torch.randn(N, generator=g)
        beta = torch.randn(N, generator=g)
        _ROWS[(M, K)] = tuple(t.to(DEV) for t in (w, bias, r, gamma, beta))
    return _ROWS[(M, K)]


def reference(ops, a, w, bias, r, gamma, beta):
    """the two launches: ops.gemm with an fp32 residual, ops.layernorm on its rows"""
    c = ops.gemm(a, w, bias, residual=r, out_dtype=torch.float32)
    return c, ops.layernorm(c, gamma, beta, EPS)


# ---- plain-A form at N = 256
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("K", [64, 256, 2048])
def test_plain_form_has_the_bits_of_gemm_and_layernorm(ops, K, M, with_bias):
    assert ops.gemm_residual_layernorm_supported(N, K)
    w, bias, r, gamma, beta = row_side(ops, M, K)
    bias = bias if with_bias else None
    a = torch.randn(M, K, generator=torch.Generator().manual_seed(K + M)).to(ops.OP16).to(DEV)
    av = nan_padded(M, K, K + 8, ops.OP16, a)               # lda > K
    rv = nan_padded(M, N, N + 4, torch.float32, r)          # ldr > N
    c, y = Canvas(M, N, torch.float32), Canvas(M, N, ops.OP16)   # ldc, ldy > N
    ops.gemm_residual_layernorm(av, w, bias, rv, gamma, beta, EPS, out=c.view, out16=y.view)
    assert c.sentinels_intact() and y.sentinels_intact(), "wrote outside an output view (padding columns, or rows past M)"
    c_ref, y_ref = reference(ops, a, w, bias, r, gamma, beta)
    print(f"plain {M}x{N}x{K} bias={with_bias}: max |C32 - gemm| {(c.view - c_ref).abs().max().item():.3e}, "
          f"{int((y.view.contiguous().view(torch.int16) != y_ref.view(torch.int16)).sum())} Y16 elements differ")
    same_bits(c.view.contiguous(), c_ref, f"C32 {M}x{N}x{K} against ops.gemm with an fp32 residual")
    same_bits(y.view.contiguous(), y_ref, f"Y16 {M}x{N}x{K} against ops.layernorm on those rows")


# ---- merged form
GUARD = 256


def fabricated_workspace(ops, M, D, splits):
    """A split-KV workspace in the attention ABI's layout -- [splits][M][D] 16-bit partials, then [splits][M][2] fp32 (max, sum) -- inside
    guard bytes.  Random partials and pairs with sum > 0; split 1 is empty (max = -inf, sum = 0) on every row; on rows 0, 7 and M - 1 all
    splits but the last are empty.  The partials of empty splits are NaN: nothing may read them into a result.  Returns (buffer, view)."""
    g = torch.Generator().manual_seed(100 * D + 10 * splits + M)
    part = torch.randn(splits, M, D, generator=g)
    mx = torch.randn(splits, M, generator=g) * 3
    sm = torch.rand(splits, M, generator=g) * 5 + 0.1
    empty = torch.zeros(splits, M, dtype=torch.bool)
    empty[1, :] = True
    if splits > 2:
        for row in (0, 7, M - 1):
            empty[:, row] = True
            empty[splits - 1, row] = False
    mx[empty] = float("-inf")
    sm[empty] = 0.0
    part[empty] = float("nan")
    pb = part.to(ops.OP16).contiguous().view(torch.uint8).flatten()
    mb = torch.stack([mx, sm], -1).contiguous().view(torch.uint8).flatten()
    body = torch.cat([pb, mb])
    assert body.numel() == ops.lib().msam2_attention_workspace_bytes(1, 1, M, D, splits)
    buf = torch.full((GUARD + body.numel() + GUARD,), 0xA5, dtype=torch.uint8)
    buf[GUARD:GUARD + body.numel()] = body
    buf = buf.to(DEV)
    return buf, buf[GUARD:GUARD + body.numel()]


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("splits", [2, 4, 8])
@pytest.mark.parametrize("D", [64, 256])
def test_merged_form_has_the_bits_of_merge_gemm_layernorm(ops, D, splits, M):
    assert ops.gemm_merged_residual_layernorm_supported(N, D, splits)
    w, bias, r, gamma, beta = row_side(ops, M, D)
    buf, ws = fabricated_workspace(ops, M, D, splits)
    before = buf.clone()
    rv = nan_padded(M, N, N + 4, torch.float32, r)
    c, y = Canvas(M, N, torch.float32), Canvas(M, N, ops.OP16)
    ops.gemm_merged_residual_layernorm(ws, splits, D, w, bias, rv, gamma, beta, EPS, out=c.view, out16=y.view)
    assert torch.equal(buf, before), "the workspace or its guard bytes changed"
    assert c.sentinels_intact() and y.sentinels_intact(), "wrote outside an output view"
    Lk = splits * 32 * 8                                     # enough key tiles that the effective split count is `splits`
    assert ops.attention_effective_splits(Lk, splits) == splits
    o = torch.empty(1, M, 1, D, dtype=ops.OP16, device=DEV).permute(0, 2, 1, 3)
    ops.attention_merge(o, Lk, splits, ws.clone())
    a = o.permute(0, 2, 1, 3).reshape(M, D)
    assert bool(torch.isfinite(a.float()).all()), "the reference merge read an empty split"
    c_ref, y_ref = reference(ops, a, w, bias, r, gamma, beta)
    print(f"merged D={D} splits={splits} M={M}: max |C32 - launches| {(c.view - c_ref).abs().max().item():.3e}, "
          f"{int((y.view.contiguous().view(torch.int16) != y_ref.view(torch.int16)).sum())} Y16 elements differ")
    same_bits(c.view.contiguous(), c_ref, f"C32, D={D} splits={splits} M={M}, against attention_merge -> gemm")
    same_bits(y.view.contiguous(), y_ref, f"Y16, D={D} splits={splits} M={M}, against layernorm on those rows")


def test_refusals(ops):
    M, D = 65, 64
    w, bias, r, gamma, beta = row_side(ops, M, D)
    _, ws = fabricated_workspace(ops, M, D, 8)
    big = torch.zeros(ws.numel() * 2 + 64, dtype=torch.uint8, device=DEV)
    call = lambda ws_, s, d, w_: ops.gemm_merged_residual_layernorm(ws_, s, d, w_, bias, r, gamma, beta, EPS)
    assert not ops.gemm_merged_residual_layernorm_supported(N, D, 9) and not ops.gemm_merged_residual_layernorm_supported(N, D, 1)
    assert not ops.gemm_merged_residual_layernorm_supported(N, 128, 4) and not ops.gemm_merged_residual_layernorm_supported(384, D, 4)
    with pytest.raises(RuntimeError, match=r"gemm_merged_residual_layernorm: splits=9 outside \[2, 8\]"):
        call(big, 9, D, w)
    with pytest.raises(RuntimeError, match=r"gemm_merged_residual_layernorm: splits=1 outside \[2, 8\]"):
        call(big, 1, D, w)
    with pytest.raises(RuntimeError, match=r"gemm_merged_residual_layernorm: D=128 is not built \(64, 256\)"):
        call(big, 4, 128, torch.zeros(N, 128, dtype=ops.OP16, device=DEV))
    with pytest.raises(RuntimeError, match=r"gemm_merged_residual_layernorm: workspace too small \(\d+ of \d+ bytes\)"):
        call(ws[:-16], 8, D, w)
    with pytest.raises(RuntimeError, match=r"gemm_merged_residual_layernorm: workspace, W, bias, R32, C32, ln_w, ln_b must be 16-byte aligned"):
        call(big[8:], 8, D, w)
    assert not ops.gemm_residual_layernorm_supported(N, 128)
    with pytest.raises((ValueError, RuntimeError), match=r"N = 256, K = 128 is not built"):
        ops.gemm_residual_layernorm(torch.zeros(M, 128, dtype=ops.OP16, device=DEV), torch.zeros(N, 128, dtype=ops.OP16, device=DEV), bias, r,
                                    gamma, beta, EPS)


# ---- whole module, eval mode: the switch is read when the module is imported, so each setting runs in a fresh child process
L_SIDE, NK = 32, 2048
CHILD = r"""
import sys, torch
sys.path.insert(0, {root!r})
import medical_sam2_amd.ops as ops
import medical_sam2_amd.modeling.memory as mem
from medical_sam2_amd.modeling.common import attn_splits
torch.set_grad_enabled(False)
torch.manual_seed(11)
rope = lambda **kw: mem.RoPEAttention(rope_theta=10000.0, feat_sizes=[32, 32], embedding_dim=256, num_heads=1, downsample_rate=1, dropout=0.1, **kw)
layer = mem.MemoryAttentionLayer(activation="relu", dim_feedforward=2048, dropout=0.1, pos_enc_at_attn=False, self_attention=rope(), d_model=256,
                                 pos_enc_at_cross_attn_keys=True, pos_enc_at_cross_attn_queries=False,
                                 cross_attention=rope(rope_k_repeat=True, kv_in_dim=64))
m = mem.MemoryAttention(d_model=256, pos_enc_at_input=True, layer=layer, num_layers=4)
for mod in m.modules():                                      # LayerNorms that do something
    if isinstance(mod, torch.nn.LayerNorm):
        torch.nn.init.normal_(mod.weight, 1.0, 0.3)
        torch.nn.init.normal_(mod.bias, 0.0, 0.3)
m = m.cuda().eval()
L, NK = {L}, {NK}
g = torch.Generator().manual_seed(12)
curr, pos = torch.randn(L, 1, 256, generator=g).cuda(), torch.randn(L, 1, 256, generator=g).cuda()
memory, mpos = torch.randn(NK, 1, 64, generator=g).cuda(), torch.randn(NK, 1, 64, generator=g).cuda()
calls = {{"merged": 0, "plain": 0}}
real_m, real_p = ops.gemm_merged_residual_layernorm, ops.gemm_residual_layernorm
ops.gemm_merged_residual_layernorm = lambda *a, **k: (calls.__setitem__("merged", calls["merged"] + 1), real_m(*a, **k))[1]
ops.gemm_residual_layernorm = lambda *a, **k: (calls.__setitem__("plain", calls["plain"] + 1), real_p(*a, **k))[1]
full = m(curr, memory, pos, mpos, num_obj_ptr_tokens=0)
# 9 key tiles of the capacity's 64: the kernels' split -> tile map (ceil(9 / splits) tiles each) leaves the last splits without a key
short = m(curr, memory, pos, mpos, num_obj_ptr_tokens=0, key_count=torch.tensor(288, dtype=torch.int32, device="cuda"))
torch.cuda.synchronize()
torch.save({{"full": full.cpu(), "short": short.cpu(), "calls": calls, "op16": str(ops.OP16),
            "splits": (ops.attention_effective_splits(L, attn_splits(1, 1, L, L)), ops.attention_effective_splits(NK, attn_splits(1, 1, L, NK)))}}, sys.argv[1])
"""


@pytest.fixture(scope="module")
def module_runs(ops, tmp_path_factory):
    """MemoryAttention.forward (4 layers, L = 1024 queries, 2048 memory rows, B = 1) in two child processes: as dispatched, and switched off"""
    d = tmp_path_factory.mktemp("memattn_tail")
    script = d / "child.py"
    script.write_text(CHILD.format(root=ROOT, L=L_SIDE * L_SIDE, NK=NK))
    out = {}
    for name, extra in (("on", {}), ("off", {"MSAM2_NO_FUSED_MEMATTN_TAIL": "1"})):
        env = {k: v for k, v in os.environ.items() if k not in ("MSAM2_NO_FUSED_MEMATTN_TAIL", "MSAM2_FUSED_MEMATTN_TAIL_PARTS")}
        env.update(extra, PYTHONUNBUFFERED="1")
        r = subprocess.run([sys.executable, str(script), str(d / f"{name}.pt")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        out[name] = torch.load(d / f"{name}.pt")
    return out


def test_module_takes_the_fused_tails_and_the_switch_brings_the_launches_back(ops, module_runs):
    on, off = module_runs["on"], module_runs["off"]
    assert on["op16"] == off["op16"] == str(ops.OP16)
    sa, ca = on["splits"]
    assert 2 <= sa <= 8 and 2 <= ca <= 8, f"both attentions must merge at this size: {sa}, {ca}"
    # two forwards of four layers, a self- and a cross-attention tail each (linear2 + norm1 is off the default list)
    assert on["calls"]["merged"] == 2 * 4 * 2, on["calls"]
    assert off["calls"] == {"merged": 0, "plain": 0}, off["calls"]


def test_module_output_equals_the_switched_off_path(module_runs):
    on, off = module_runs["on"], module_runs["off"]
    print(f"full bank: max |on - off| {(on['full'] - off['full']).abs().max().item():.3e}")
    assert bool(torch.isfinite(on["full"]).all())
    same_bits(on["full"], off["full"], "MemoryAttention.forward, fused tails vs MSAM2_NO_FUSED_MEMATTN_TAIL=1")


def test_module_output_with_empty_splits_equals_the_switched_off_path(module_runs):
    on, off = module_runs["on"], module_runs["off"]
    print(f"key_count = 288 of 2048: max |on - off| {(on['short'] - off['short']).abs().max().item():.3e}")
    assert bool(torch.isfinite(on["short"]).all())
    same_bits(on["short"], off["short"], "MemoryAttention.forward with a padded bank (empty splits), fused vs switched off")
    assert not torch.equal(on["short"], on["full"])


def test_same_file_on_the_bf16_library(ops):
    """the operand type is a property of the loaded library: the tests of this file once more in a child process on libmsam2_hip_bf16.so"""
    if os.environ.get("MSAM2_LIB_PATH"):
        assert str(ops.OP16).endswith(os.environ.get("MSAM2_EXPECT_OP16", "")), ops.OP16
        return                                              # this IS a run on a chosen library
    lib = os.path.join(ROOT, "medical-sam2_amd", "libmsam2_hip_bf16.so")
    assert os.path.exists(lib), "libmsam2_hip_bf16.so is built by __graft_entry__.build()"
    env = dict(os.environ, MSAM2_LIB_PATH=lib, MSAM2_EXPECT_OP16="bfloat16", PYTHONUNBUFFERED="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-30:])
    print(tail)
    assert r.returncode == 0 and " passed" in tail and "failed" not in tail, tail
