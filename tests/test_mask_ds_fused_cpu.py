"""Python plumbing of the mask down-sampler's one-kernel stages with the ops stubbed (no GPU): the stage list, the per-stage dispatch in
MaskDownSampler.run, the module switch, and a width the kernel is not built for."""
import pytest
import torch

import medical_sam2_amd.modeling.memory as mem


def test_stage_list_parsing():
    assert mem._stage_list("2,3,4") == frozenset((2, 3, 4))
    assert mem._stage_list(" 4 , 2,") == frozenset((2, 4))
    assert mem._stage_list("") == frozenset()
    with pytest.raises(ValueError):
        mem._stage_list("2;3")
    assert mem._FUSED_MASK_DS_STAGES <= frozenset((2, 3, 4))


def _sampler(monkeypatch, supported=lambda cin, cout: (cin, cout) in ((4, 16), (16, 64), (64, 256))):
    """a MaskDownSampler whose ops record how they were called instead of running kernels"""
    calls = []
    ds = mem.MaskDownSampler(embed_dim=256, kernel_size=3, stride=2, padding=1, total_stride=16)

    def conv1(h, n, H, W, *a):
        calls.append(("stage1", 4))
        return torch.zeros(n * (H // 2) * (W // 2), 4)

    def im2col(h, n, H, W):
        calls.append(("im2col", h.shape[1]))
        return torch.zeros(n * (H // 2) * (W // 2), (9 * h.shape[1] + 7) // 8 * 8)

    def gemm(a, w, b, **k):
        calls.append(("gemm", w.shape[0]))
        assert a.shape[1] == w.shape[1], "the packed weight serves the patch matrix"
        return torch.zeros(a.shape[0], w.shape[0])

    def layernorm(g, w, b, eps, act=0):
        calls.append(("ln", g.shape[1]))
        assert act == mem.ops.ACT_GELU
        return g

    def fused(h, n, H, W, w, b, lw, lb, eps):
        calls.append(("fused", w.shape[0]))
        assert w.shape[1] == (9 * h.shape[1] + 7) // 8 * 8 and eps == 1e-6
        return torch.zeros(n * (H // 2) * (W // 2), w.shape[0])

    monkeypatch.setattr(mem.ops, "conv3x3s2_ln_gelu", conv1)
    monkeypatch.setattr(mem.ops, "im2col3x3s2", im2col)
    monkeypatch.setattr(mem.ops, "gemm", gemm)
    monkeypatch.setattr(mem.ops, "layernorm", layernorm)
    monkeypatch.setattr(mem.ops, "conv3x3s2_mfma_ln_gelu", fused)
    monkeypatch.setattr(mem.ops, "conv3x3s2_mfma_ln_gelu_supported", supported)
    monkeypatch.setattr(mem, "OP16", torch.float32)             # the packed weight is built on the host here
    monkeypatch.setattr(mem, "v_f32", lambda wc, key, p: p)
    monkeypatch.setattr(mem, "w_bf16", lambda wc, key, p: p.detach().reshape(p.shape[0], -1))
    return ds, calls


THREE = lambda c: [("im2col", c // 4), ("gemm", c), ("ln", c)]
PROJ = [("gemm", 256)]


def _run(ds):
    with torch.no_grad():
        out = ds.run(torch.zeros(1, 1, 64, 64), 1, 1.0, 0.0)
    assert out.shape == (16, 256)


def test_per_stage_dispatch(monkeypatch):
    ds, calls = _sampler(monkeypatch)
    monkeypatch.setattr(mem, "_FUSED_MASK_DS", True)
    monkeypatch.setattr(mem, "_FUSED_MASK_DS_STAGES", frozenset((2, 3, 4)))
    _run(ds)
    assert calls == [("stage1", 4), ("fused", 16), ("fused", 64), ("fused", 256)] + PROJ
    del calls[:]
    monkeypatch.setattr(mem, "_FUSED_MASK_DS_STAGES", frozenset((2, 4)))   # the per-stage switch: stage 3 keeps its three launches
    _run(ds)
    assert calls == [("stage1", 4), ("fused", 16)] + THREE(64) + [("fused", 256)] + PROJ
    del calls[:]
    monkeypatch.setattr(mem, "_FUSED_MASK_DS_STAGES", frozenset())
    _run(ds)
    assert calls == [("stage1", 4)] + THREE(16) + THREE(64) + THREE(256) + PROJ


def test_module_switch(monkeypatch):
    ds, calls = _sampler(monkeypatch)
    monkeypatch.setattr(mem, "_FUSED_MASK_DS", False)
    monkeypatch.setattr(mem, "_FUSED_MASK_DS_STAGES", frozenset((2, 3, 4)))
    _run(ds)
    assert calls == [("stage1", 4)] + THREE(16) + THREE(64) + THREE(256) + PROJ


def test_unsupported_width_keeps_the_three_launches(monkeypatch):
    ds, calls = _sampler(monkeypatch, supported=lambda cin, cout: cin != 16)
    monkeypatch.setattr(mem, "_FUSED_MASK_DS", True)
    monkeypatch.setattr(mem, "_FUSED_MASK_DS_STAGES", frozenset((2, 3, 4)))
    _run(ds)
    assert calls == [("stage1", 4), ("fused", 16)] + THREE(64) + [("fused", 256)] + PROJ
