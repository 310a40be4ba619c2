"""Python plumbing of the GEMM + LayerNorm fusion with the op stubbed (no GPU): Hiera.forward hands block i the next block's norm1 and hands
the rows block i's fc2 left to block i + 1; MLP.run dispatches per shape; the training forwards never request the fused path."""
import torch

import medical_sam2_amd.modeling.encoder as enc
from medical_sam2_amd.modeling.encoder import Hiera, MLP, MultiScaleBlock


def _trunk(monkeypatch):
    """a small Hiera whose blocks record how they were called instead of running kernels"""
    trunk = Hiera(embed_dim=96, num_heads=1, stages=(1, 1, 3, 1), global_att_blocks=(3,), window_spec=(8, 4, 14, 7))
    log = []

    def fake_run(self, t, B, H, W, emit16=False, fused_qkv_attn=False, fused_gemm_ln=False, xn=None, next_norm=None):
        i = list(trunk.blocks).index(self)
        log.append(dict(i=i, fused_gemm_ln=fused_gemm_ln, xn=xn, next_norm=next_norm))
        self.out16 = None
        self.next_xn = ("rows for block", i + 1) if fused_gemm_ln and next_norm is not None else None
        if self.q_stride:
            H, W = H // 2, W // 2
        return torch.zeros(B * H * W, self.dim_out), H, W

    monkeypatch.setattr(MultiScaleBlock, "run", fake_run)
    monkeypatch.setattr(trunk.patch_embed, "tokens", lambda x, pos=None: torch.zeros(x.shape[0] * (x.shape[-1] // 4) ** 2, 96))
    monkeypatch.setattr(trunk, "_pos_tokens", lambda h, w: None)
    monkeypatch.setattr(enc, "v_f32", lambda wc, key, p: p)
    return trunk, log


def test_trunk_hands_norm1_forward_and_rows_on(monkeypatch):
    trunk, log = _trunk(monkeypatch)
    trunk(torch.zeros(1, 3, 64, 64))
    dims = [(b.dim, b.dim_out) for b in trunk.blocks]
    assert dims == [(96, 96), (96, 192), (192, 384), (384, 384), (384, 384), (384, 768)]
    assert log[0]["xn"] is None
    for e in log:
        i = e["i"]
        assert e["fused_gemm_ln"]
        if i + 1 < len(dims):                                   # every block is offered the next block's norm1 (its input width matches)
            w, b, eps = e["next_norm"]
            assert w is trunk.blocks[i + 1].norm1.weight and b is trunk.blocks[i + 1].norm1.bias and eps == 1e-6
        else:
            assert e["next_norm"] is None
        if i > 0:                                               # and receives what the block before it left, nothing else
            assert e["xn"] == ("rows for block", i)
    assert all(b.next_xn is None for b in trunk.blocks), "a block kept a reference to the rows it handed on"


def test_training_forwards_never_request_it(monkeypatch):
    trunk, log = _trunk(monkeypatch)
    with enc.two_launch_qkv_attention():                        # frozen_forward_image: every training driver's encoder forward
        trunk(torch.zeros(1, 3, 64, 64))
    assert log and all(not e["fused_gemm_ln"] and e["next_norm"] is None and e["xn"] is None for e in log)
    import inspect
    import medical_sam2_amd.backward as bwd
    import medical_sam2_amd.backward_encoder as be
    for mod in (bwd, be):                                       # the saved forwards call blk.run / mlp.run in their plain form
        src = inspect.getsource(mod)
        assert "fused_gemm_ln" not in src and "next_norm" not in src and "ln=" not in src.replace("_ln=", "")


def _mlp(monkeypatch, supported=True):
    calls = []
    monkeypatch.setattr(enc.ops, "gemm", lambda h, w, b, **k: (calls.append(("gemm", w.shape[1])), torch.zeros(h.shape[0], w.shape[0]))[1])
    monkeypatch.setattr(enc.ops, "gemm_residual_layernorm",
                        lambda h, w, b, r, lw, lb, eps: (calls.append(("fused", w.shape[1])), (torch.zeros_like(r), "y16"))[1])
    monkeypatch.setattr(enc.ops, "gemm_residual_layernorm_supported", lambda N, K: supported and N == 384 and K % 64 == 0)
    monkeypatch.setattr(enc, "w_bf16", lambda wc, key, p: p)
    monkeypatch.setattr(enc, "v_f32", lambda wc, key, p: p)
    return MLP(384, 1536, 384, num_layers=2, activation=torch.nn.GELU), calls


def test_mlp_run_dispatch(monkeypatch):
    mlp, calls = _mlp(monkeypatch)
    x, r, ln = torch.zeros(4, 384), torch.zeros(4, 384), ("w", "b", 1e-6)
    monkeypatch.setattr(enc, "_FUSED_GEMM_LN", True)
    monkeypatch.setattr(enc, "_FUSED_GEMM_LN_K", frozenset((384, 1536)))
    out = mlp.run(x, residual=r)                                # no LayerNorm handed in: a tensor, the two GEMMs
    assert isinstance(out, torch.Tensor) and calls == [("gemm", 384), ("gemm", 1536)]
    del calls[:]
    t, y = mlp.run(x, residual=r, ln=ln)
    assert y == "y16" and calls == [("gemm", 384), ("fused", 1536)]
    del calls[:]
    monkeypatch.setattr(enc, "_FUSED_GEMM_LN_K", frozenset((384,)))   # the per-shape switch: fc2's K is not dispatched
    t, y = mlp.run(x, residual=r, ln=ln)
    assert y is None and calls == [("gemm", 384), ("gemm", 1536)]
    del calls[:]
    monkeypatch.setattr(enc, "_FUSED_GEMM_LN_K", frozenset((384, 1536)))
    monkeypatch.setattr(enc, "_FUSED_GEMM_LN", False)           # the module switch
    t, y = mlp.run(x, residual=r, ln=ln)
    assert y is None and calls == [("gemm", 384), ("gemm", 1536)]


def test_mlp_run_unsupported_width_keeps_the_gemm(monkeypatch):
    mlp, calls = _mlp(monkeypatch, supported=False)
    monkeypatch.setattr(enc, "_FUSED_GEMM_LN", True)
    t, y = mlp.run(torch.zeros(4, 384), residual=torch.zeros(4, 384), ln=("w", "b", 1e-6))
    assert y is None and calls == [("gemm", 384), ("gemm", 1536)]
