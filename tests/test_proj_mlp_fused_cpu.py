"""The proj + MLP fusion of Hiera stages 1-2 without a GPU: the W1 input permutation's formula, and MultiScaleBlock.run's dispatch rule with
the ops stubbed (taken only on the inference trunk's request, per shape, never by the training forwards)."""
import pytest
import torch

import medical_sam2_amd.modeling.encoder as enc
import medical_sam2_amd.ops as ops
from medical_sam2_amd.modeling.encoder import MultiScaleBlock


@pytest.mark.parametrize("dim", [96, 192])
def test_w1_order_is_a_32_block_permutation_and_equals_w2s(dim):
    src = ops.mlp_fused_w1_order(dim)
    for b in range(dim // 32):                                  # a permutation inside every 32-block
        assert sorted(src[32 * b:32 * b + 32].tolist()) == list(range(32 * b, 32 * b + 32))
    # the accumulator's register order: lane half h, register e of d-block d holds channel 32 d + 8 (e >> 2) + 4 h + (e & 3); registers
    # 0-7 / 8-15 are k-steps 2 d / 2 d + 1, whose operand position is 16 (k-step) + 8 h + j
    for d in range(dim // 32):
        for h in range(2):
            for e in range(16):
                pos = 16 * (2 * d + (e >> 3)) + 8 * h + (e & 7)
                assert src[pos] == 32 * d + 8 * (e >> 2) + 4 * h + (e & 3)
    # W2's hidden permutation (mlp_fused_permute_kernel's formula, restated): the same map per 32-block
    for pos in range(dim):
        q = pos & 31
        s, hh, j = q >> 4, (q >> 3) & 1, q & 7
        assert src[pos] == (pos >> 5) * 32 + 16 * s + 8 * (j >> 2) + 4 * hh + (j & 3)


def _block(monkeypatch, dim=96, dim_out=96, heads=1, hw=32, supported=(96, 192), act=torch.nn.GELU):
    """a block whose kernels are stubs that record the launches"""
    calls = []
    blk = MultiScaleBlock(dim=dim, dim_out=dim_out, num_heads=heads, window_size=8, act_layer=act)
    T = hw * hw
    rec = lambda name, ret: (lambda *a, **k: (calls.append(name), ret(*a, **k))[1])
    monkeypatch.setattr(enc.ops, "layernorm", rec("layernorm", lambda t, *a, **k: torch.zeros(t.shape)))
    monkeypatch.setattr(enc.ops, "window_qkv_attention_supported", lambda *a: True)
    monkeypatch.setattr(enc.ops, "window_qkv_attention", rec("attn", lambda xn, w, *a, **k: torch.zeros(xn.shape[0], w.shape[0] // 3)))
    monkeypatch.setattr(enc.ops, "gemm_qkv_pool2x2", None)
    monkeypatch.setattr(enc.ops, "gemm", rec("gemm", lambda a, w, b=None, **k: torch.zeros(a.shape[0], w.shape[0])))
    monkeypatch.setattr(enc.ops, "window_attention", rec("attn", lambda qkv, *a, **k: torch.zeros(qkv.shape[0], qkv.shape[1] // 3)))
    monkeypatch.setattr(enc.ops, "ln_mlp_residual_supported", lambda d: d in (96, 192))
    monkeypatch.setattr(enc.ops, "ln_mlp_residual", rec("mlp", lambda t, *a, also16=False, **k: (t, "o16") if also16 else t))
    monkeypatch.setattr(enc.ops, "mlp_fused_permute_w1", lambda w: w)
    monkeypatch.setattr(enc.ops, "mlp_fused_permute_w2", lambda w: w)
    monkeypatch.setattr(enc.ops, "proj_ln_mlp_residual_supported", lambda d: d in supported)
    monkeypatch.setattr(enc.ops, "proj_ln_mlp_residual",
                        rec("proj_mlp", lambda o, wp, bp, res, *a, also16=False, next_ln=None:
                            (res, "o16" if also16 else None, "xn" if next_ln is not None else None)))
    monkeypatch.setattr(enc.ops, "gemm_residual_layernorm_supported", lambda N, K: False)
    monkeypatch.setattr(enc, "w_bf16", lambda wc, key, p: p)
    monkeypatch.setattr(enc, "v_f32", lambda wc, key, p: p)
    monkeypatch.setattr(enc, "_FUSED_PROJ_MLP", True)
    monkeypatch.setattr(enc, "_FUSED_QKV_ATTN", True)
    monkeypatch.setattr(enc, "_FUSED_PROJ_MLP_DIMS", frozenset((96, 192)))
    monkeypatch.setattr(enc, "_FUSED_PROJ_MLP_NEXT_LN_DIMS", frozenset((96, 192)))
    run = lambda **k: (calls.clear(), blk.run(torch.zeros(T, dim), 1, hw, hw, **k), list(calls))[2]
    return blk, run


TODAY = ["layernorm", "attn", "gemm", "mlp"]
NN = ("w", "b", 1e-6)


def test_taken_only_on_request(monkeypatch):
    blk, run = _block(monkeypatch)
    assert run() == ["layernorm", "gemm", "attn", "gemm", "mlp"]   # the training forwards' call form: every launch they have today
    assert run(fused_qkv_attn=True) == TODAY
    assert run(fused_gemm_ln=True) == ["layernorm", "gemm", "attn", "gemm", "mlp"]   # only behind the one-kernel attention
    monkeypatch.setattr(enc, "_FUSED_QKV_ATTN", False)          # MSAM2_NO_FUSED_QKV_ATTN=1 brings the whole block back to the training forward's bits
    assert run(fused_qkv_attn=True, fused_gemm_ln=True) == ["layernorm", "gemm", "attn", "gemm", "mlp"]
    monkeypatch.setattr(enc, "_FUSED_QKV_ATTN", True)
    assert run(fused_qkv_attn=True, fused_gemm_ln=True) == ["layernorm", "attn", "proj_mlp"]
    assert blk.next_xn is None and blk.out16 is None
    assert run(fused_qkv_attn=True, fused_gemm_ln=True, emit16=True, next_norm=NN) == ["layernorm", "attn", "proj_mlp"]
    assert blk.next_xn == "xn" and blk.out16 == "o16"
    assert run(fused_qkv_attn=True, fused_gemm_ln=True, xn=torch.zeros(1024, 96)) == ["attn", "proj_mlp"]   # norm1 rows handed in: no LayerNorm launch either


def test_switches(monkeypatch):
    blk, run = _block(monkeypatch)
    on = dict(fused_qkv_attn=True, fused_gemm_ln=True, next_norm=NN)
    monkeypatch.setattr(enc, "_FUSED_PROJ_MLP", False)          # MSAM2_NO_FUSED_PROJ_MLP=1: today's launches
    assert run(**on) == TODAY and blk.next_xn is None
    monkeypatch.setattr(enc, "_FUSED_PROJ_MLP", True)
    monkeypatch.setattr(enc, "_FUSED_PROJ_MLP_DIMS", frozenset((192,)))   # the per-shape list
    assert run(**on) == TODAY and blk.next_xn is None
    monkeypatch.setattr(enc, "_FUSED_PROJ_MLP_DIMS", frozenset((96,)))
    monkeypatch.setattr(enc, "_FUSED_PROJ_MLP_NEXT_LN_DIMS", frozenset())  # the norm1 rows' own list: the kernel is taken, the rows are not asked for
    assert run(**on) == ["layernorm", "attn", "proj_mlp"] and blk.next_xn is None


def test_refused_forms(monkeypatch):
    on = dict(fused_qkv_attn=True, fused_gemm_ln=True, next_norm=NN)
    blk, run = _block(monkeypatch, supported=())                # the library's gate
    assert run(**on) == TODAY
    blk, run = _block(monkeypatch, act=torch.nn.ReLU)           # a non-GELU MLP has no one-kernel form
    assert "proj_mlp" not in run(**on) and "mlp" not in run(**on)
    blk, run = _block(monkeypatch, hw=16)                       # fewer than 1024 tokens per slice: no one-kernel MLP, so nothing to fold into
    assert "proj_mlp" not in run(**on)
    assert not enc._proj_mlp_dispatched(96, 128) and enc._proj_mlp_dispatched(96, 96)   # a padded head width: the proj is not square


def test_rule_never_looks_at_the_batch(monkeypatch):
    import inspect
    src = inspect.getsource(enc._proj_mlp_dispatched)
    assert "B" not in src.split('"""')[2]
    import medical_sam2_amd.backward as bwd
    import medical_sam2_amd.backward_encoder as be
    for mod in (bwd, be):                                       # the saved forwards never name the fused call
        assert "proj_ln_mlp_residual" not in inspect.getsource(mod)
