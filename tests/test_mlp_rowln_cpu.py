"""The one-kernel stage-3 MLP (ops.mlp_residual_layernorm), host side: what is built, what the wrapper refuses, how MLP.run dispatches it, and
a restatement of the kernel's chunk / stage schedule (csrc/mlp_rowln.hip) showing that every accumulator takes k ascending."""
import inspect

import pytest
import torch

import medical_sam2_amd.modeling.encoder as enc
import medical_sam2_amd.ops as ops
from medical_sam2_amd.modeling.encoder import MLP


def test_supported_queries():
    assert all(ops.mlp_residual_layernorm_supported(384, h) for h in (128, 256, 1536, 2048))
    assert not any(ops.mlp_residual_layernorm_supported(n, h) for n, h in ((384, 0), (384, 64), (384, 192), (384, 1600), (256, 2048), (96, 384),
                                                                           (192, 768), (768, 3072)))


def test_wrapper_refusals():
    M, N, H = 8, 384, 128
    z = lambda *s: torch.zeros(*s, dtype=ops.OP16)
    f = lambda *s: torch.zeros(*s)
    a, w1, w2, r, v = z(M, N), z(H, N), z(N, H), f(M, N), f(N)
    with pytest.raises(ValueError, match=r"mlp_residual_layernorm shapes \(8, 384\) x \(128, 384\) x \(384, 256\)"):
        ops.mlp_residual_layernorm(a, w1, None, z(N, 256), None, r, v, v, 1e-6)
    with pytest.raises(ValueError, match=r"operands: 16-bit, reduction dimension contiguous"):
        ops.mlp_residual_layernorm(a.float(), w1, None, w2, None, r, v, v, 1e-6)
    with pytest.raises(ValueError, match=r"operands: 16-bit, reduction dimension contiguous"):
        ops.mlp_residual_layernorm(a, z(N, H).t(), None, w2, None, r, v, v, 1e-6)
    with pytest.raises(ValueError, match=r"N = 384, H = 192 is not built \(N = 384 with H % 128 == 0\)"):
        ops.mlp_residual_layernorm(a, z(192, N), None, z(N, 192), None, r, v, v, 1e-6)
    with pytest.raises(ValueError, match=r"N = 256, H = 1024 is not built"):
        ops.mlp_residual_layernorm(z(M, 256), z(1024, 256), None, z(256, 1024), None, f(M, 256), f(256), f(256), 1e-6)
    with pytest.raises(ValueError, match=r"residual must be fp32 \[M, N\]"):
        ops.mlp_residual_layernorm(a, w1, None, w2, None, f(M + 1, N), v, v, 1e-6)
    with pytest.raises(ValueError, match=r"b1 is fp32 \[H\]; b2, ln_w, ln_b are fp32 \[N\]"):
        ops.mlp_residual_layernorm(a, w1, f(N), w2, None, r, v, v, 1e-6)
    with pytest.raises(ValueError, match=r"out is fp32 \[M, N\], out16 16-bit \[M, N\], rows contiguous"):
        ops.mlp_residual_layernorm(a, w1, None, w2, None, r, v, v, 1e-6, out=f(M, N), out16=f(M, N))


def _mlp(monkeypatch, supported=True):
    calls = []
    monkeypatch.setattr(enc.ops, "gemm", lambda h, w, b, **k: (calls.append(("gemm", w.shape[1])), torch.zeros(h.shape[0], w.shape[0]))[1])
    monkeypatch.setattr(enc.ops, "gemm_residual_layernorm",
                        lambda h, w, b, r, lw, lb, eps: (calls.append(("fused", w.shape[1])), (torch.zeros_like(r), "y16"))[1])
    monkeypatch.setattr(enc.ops, "mlp_residual_layernorm",
                        lambda h, w1, b1, w2, b2, r, lw, lb, eps: (calls.append(("mlp", w1.shape[0])), (torch.zeros_like(r), "y16"))[1])
    monkeypatch.setattr(enc.ops, "gemm_residual_layernorm_supported", lambda N, K: N == 384 and K % 64 == 0)
    monkeypatch.setattr(enc.ops, "mlp_residual_layernorm_supported", lambda N, H: supported and N == 384 and H % 128 == 0)
    monkeypatch.setattr(enc, "w_bf16", lambda wc, key, p: p)
    monkeypatch.setattr(enc, "v_f32", lambda wc, key, p: p)
    monkeypatch.setattr(enc, "_FUSED_GEMM_LN", True)
    monkeypatch.setattr(enc, "_FUSED_GEMM_LN_K", frozenset((384, 1536)))
    monkeypatch.setattr(enc, "_FUSED_MLP_LN", True)
    return calls


def test_mlp_run_dispatch(monkeypatch):
    calls = _mlp(monkeypatch)
    pair = [("gemm", 384), ("fused", 1536)]
    mlp = MLP(384, 1536, 384, num_layers=2, activation=torch.nn.GELU)
    x, r, ln = torch.zeros(4, 384), torch.zeros(4, 384), ("w", "b", 1e-6)
    t, y = mlp.run(x, residual=r, ln=ln, one_kernel=True)
    assert y == "y16" and calls == [("mlp", 1536)]
    del calls[:]
    t, y = mlp.run(x, residual=r, ln=ln)                          # a caller that does not ask keeps the pair
    assert y == "y16" and calls == pair
    del calls[:]
    out = mlp.run(x, residual=r, one_kernel=True)                 # no LayerNorm handed in: the two GEMMs
    assert isinstance(out, torch.Tensor) and calls == [("gemm", 384), ("gemm", 1536)]
    del calls[:]
    monkeypatch.setattr(enc, "_FUSED_MLP_LN", False)              # MSAM2_NO_FUSED_MLP_LN=1
    t, y = mlp.run(x, residual=r, ln=ln, one_kernel=True)
    assert y == "y16" and calls == pair
    del calls[:]
    monkeypatch.setattr(enc, "_FUSED_MLP_LN", True)
    monkeypatch.setattr(enc, "_FUSED_GEMM_LN", False)             # without the row kernels there is no fused form at all
    t, y = mlp.run(x, residual=r, ln=ln, one_kernel=True)
    assert y is None and calls == [("gemm", 384), ("gemm", 1536)]
    del calls[:]
    monkeypatch.setattr(enc, "_FUSED_GEMM_LN", True)
    for other in (MLP(384, 1536, 384, num_layers=2, activation=torch.nn.ReLU), MLP(384, 1536, 384, num_layers=3, activation=torch.nn.GELU),
                  MLP(384, 1536, 384, num_layers=2, activation=torch.nn.GELU, sigmoid_output=True)):
        other.run(x, residual=r, ln=ln, one_kernel=True)
        assert not any(c[0] == "mlp" for c in calls)


def test_unsupported_shape_keeps_the_pair(monkeypatch):
    calls = _mlp(monkeypatch, supported=False)
    mlp = MLP(384, 1536, 384, num_layers=2, activation=torch.nn.GELU)
    t, y = mlp.run(torch.zeros(4, 384), residual=torch.zeros(4, 384), ln=("w", "b", 1e-6), one_kernel=True)
    assert y == "y16" and calls == [("gemm", 384), ("fused", 1536)]


def test_gate_never_sees_the_batch():
    assert list(inspect.signature(enc._mlp_ln_dispatched).parameters) == ["N", "H"]
    src = inspect.getsource(enc.MultiScaleBlock.run)
    assert "one_kernel=Hq * Wq >= _FUSED_MLP_LN_MIN_TOKENS" in src    # tokens per slice, not rows of the batch


def test_training_forwards_never_ask():
    import medical_sam2_amd.backward as bwd
    import medical_sam2_amd.backward_encoder as be
    for mod in (bwd, be):
        assert "one_kernel" not in inspect.getsource(mod) and "mlp_residual_layernorm" not in inspect.getsource(mod)


# ---- the schedule of mlp_rowln_kernel, restated: stage s = 4 c + t of chunk c goes through ring buffer t & 1
def schedule(H, N=384):
    """[(stage, buffer, kind, rows, k range)] in issue order, and per accumulator the k ranges it consumes in order"""
    stages, fc1_k, fc2_k = [], {}, []
    for c in range(H // 128):
        for t in range(4):
            s = 4 * c + t
            if t < 2:
                k = (t * N // 2, (t + 1) * N // 2)
                stages.append((s, t & 1, "W1", (128 * c, 128 * c + 128), k))
                for kl in range(3):                               # three 64-k images, four 16-wide MFMA steps each
                    for ks in range(4):
                        k0 = k[0] + 64 * kl + 16 * ks
                        fc1_k.setdefault(c, []).append((k0, k0 + 16))
            else:
                k = (128 * c + 64 * (t - 2), 128 * c + 64 * (t - 1))
                stages.append((s, t & 1, "W2", (0, N), k))
                for ks in range(4):
                    fc2_k.append((k[0] + 16 * ks, k[0] + 16 * ks + 16))
    return stages, fc1_k, fc2_k


@pytest.mark.parametrize("H", [128, 256, 1536])
def test_schedule_takes_k_ascending(H):
    stages, fc1_k, fc2_k = schedule(H)
    assert len(stages) == 4 * H // 128 and [s[0] for s in stages] == list(range(len(stages)))
    assert all(a[1] != b[1] for a, b in zip(stages, stages[1:])), "consecutive stages share a ring buffer"
    for c, ks in fc1_k.items():                                   # a chunk's fc1 accumulator: k = 0 .. 383 in 24 ascending 16-wide steps
        assert ks == [(16 * i, 16 * i + 16) for i in range(24)]
    assert fc2_k == [(16 * i, 16 * i + 16) for i in range(H // 16)]   # each C accumulator: the hidden index ascending, as at K = H
    # the hidden image of chunk c is written behind stage 4 c + 1 and read in stages 4 c + 2, 4 c + 3: two barriers (stages 4 c + 4,
    # 4 c + 5) lie between its last read and the next chunk's stores
    for c in range(H // 128 - 1):
        last_read, next_write = 4 * c + 3, 4 * (c + 1) + 1
        assert next_write - last_read == 2
    # every W1 element and every W2 element is streamed exactly once per workgroup
    w1 = sum((r[1] - r[0]) * (k[1] - k[0]) for _, _, kind, r, k in stages if kind == "W1")
    w2 = sum((r[1] - r[0]) * (k[1] - k[0]) for _, _, kind, r, k in stages if kind == "W2")
    assert w1 == H * 384 and w2 == 384 * H
