"""The memory attention's fused tails, host side: the gate that decides how a tail runs (modeling.memory._tail_form), and the merge rule of
the kernel's "merged" A source restated in torch (tests/memattn_restate.py) on the workspace layout, against a plain softmax recombination."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import memattn_restate as R  # noqa: E402


@pytest.fixture()
def mem(monkeypatch):
    import medical_sam2_amd.modeling.memory as m
    monkeypatch.setattr(m, "_FUSED_TAIL", True)
    monkeypatch.setattr(m, "_FUSED_TAIL_PARTS", frozenset(("sa", "ca", "ffn")))
    return m


# part, N, K, effective splits, kv split, training -> form
GATE = [
    ("sa", 256, 256, 4, False, False, "merged"),
    ("sa", 256, 256, 2, False, False, "merged"),
    ("sa", 256, 256, 8, False, False, "merged"),
    ("sa", 256, 256, 9, False, False, ""),            # more partials than the kernel loads up front: the merge launch stays
    ("sa", 256, 256, 16, False, False, ""),
    ("sa", 256, 256, 1, False, False, "plain"),       # nothing to merge
    ("sa", 256, 256, 4, True, False, "merged"),       # the cross-GPU key split splits the memory bank's keys, not the self-attention's
    ("sa", 256, 256, 4, False, True, ""),             # train mode keeps its launches
    ("sa", 256, 128, 4, False, False, ""),            # a head dim that is not built
    ("sa", 384, 256, 4, False, False, ""),            # a width that is not built
    ("ca", 256, 64, 4, False, False, "merged"),
    ("ca", 256, 64, 8, False, False, "merged"),
    ("ca", 256, 64, 1, False, False, "plain"),
    ("ca", 256, 64, 4, True, False, ""),              # partial + exchange + merge stay
    ("ca", 256, 64, 1, True, False, ""),
    ("ca", 256, 64, 4, False, True, ""),
    ("ca", 256, 64, 12, False, False, ""),
    ("ffn", 256, 2048, 1, False, False, "plain"),
    ("ffn", 256, 2048, 1, True, False, "plain"),
    ("ffn", 256, 2048, 1, False, True, ""),
    ("ffn", 256, 1024, 1, False, False, ""),          # a reduction length that is not built at this width
    ("ffn", 384, 1536, 1, False, False, "plain"),
]


@pytest.mark.parametrize("part,N,K,splits,kv,train,want", GATE)
def test_gate(mem, part, N, K, splits, kv, train, want):
    assert mem._tail_form(part, N, K, splits, kv, train) == want


def test_gate_switches(mem, monkeypatch):
    assert mem._tail_form("sa", 256, 256, 4, False, False) == "merged"
    monkeypatch.setattr(mem, "_FUSED_TAIL_PARTS", frozenset(("sa", "ca")))            # the part list: ffn taken off
    assert mem._tail_form("ffn", 256, 2048, 1, False, False) == ""
    assert mem._tail_form("ca", 256, 64, 4, False, False) == "merged"
    monkeypatch.setattr(mem, "_FUSED_TAIL_PARTS", frozenset())
    assert all(mem._tail_form(p, 256, k, 4, False, False) == "" for p, k in (("sa", 256), ("ca", 64), ("ffn", 2048)))
    monkeypatch.setattr(mem, "_FUSED_TAIL_PARTS", frozenset(("sa", "ca", "ffn")))
    monkeypatch.setattr(mem, "_FUSED_TAIL", False)                                       # MSAM2_NO_FUSED_MEMATTN_TAIL=1
    assert all(mem._tail_form(p, 256, k, 4, False, False) == "" for p, k in (("sa", 256), ("ca", 64), ("ffn", 2048)))


def test_gate_never_sees_the_batch(mem):
    import inspect
    assert list(inspect.signature(mem._tail_form).parameters) == ["part", "N", "K", "splits", "kv_split", "training"]


def test_supported_queries():
    import medical_sam2_amd.ops as ops
    assert all(ops.gemm_residual_layernorm_supported(256, k) for k in (64, 256, 2048))
    assert all(ops.gemm_residual_layernorm_supported(384, k) for k in (64, 384, 1536))
    assert not any(ops.gemm_residual_layernorm_supported(n, k) for n, k in ((256, 384), (256, 96), (256, 0), (128, 64), (768, 384), (384, 96)))
    assert all(ops.gemm_merged_residual_layernorm_supported(256, d, s) for d in (64, 256) for s in range(2, 9))
    assert not any(ops.gemm_merged_residual_layernorm_supported(n, d, s) for n, d, s in ((256, 64, 1), (256, 64, 9), (256, 128, 4), (384, 64, 4)))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("D,splits,rows", [(64, 2, 65), (64, 8, 200), (256, 4, 65), (256, 5, 33)])
def test_merge_rule_on_the_workspace_layout(D, splits, rows, dtype):
    """the restated rule against softmax weights over the splits' log-sum-exps: a wrong row or split stride of either region, or a wrong
    rule for empty splits, moves whole rows.  Bound: the inputs are exact in both; the restatement accumulates in fp32 (a few 1e-7 relative)
    and rounds to the 16-bit type once: half an ulp of that type, 2^-11 (fp16) / 2^-8 (bf16) relative, plus the fp32 slack"""
    g = torch.Generator().manual_seed(D + splits + rows)
    part = torch.randn(splits, rows, D, generator=g).to(dtype)
    mx = torch.randn(splits, rows, generator=g) * 3
    sm = torch.rand(splits, rows, generator=g) * 5 + 0.1
    empty = torch.zeros(splits, rows, dtype=torch.bool)
    empty[1, :] = True                                       # one split empty on every row
    if splits > 2:
        empty[:, [0, 7, rows - 1]] = True                    # on a few rows all but one
        empty[splits - 1, [0, 7, rows - 1]] = False
    mx[empty], sm[empty] = float("-inf"), 0.0
    part[empty] = float("nan")                               # what an empty split leaves must not be read into a result
    ws = R.pack_workspace(part, mx, sm)
    assert ws.numel() == splits * rows * (D * 2 + 8)         # msam2_attention_workspace_bytes(1, 1, rows, D, splits)
    p2, pairs = R.unpack_workspace(ws, rows, D, splits, dtype)
    assert torch.equal(p2.view(torch.int16), part.view(torch.int16)) and torch.equal(pairs[:, :, 0], mx) and torch.equal(pairs[:, :, 1], sm)
    got = R.merged_rows(ws, rows, D, splits, dtype)
    lse = mx.double() * 0.6931471805599453 + sm.double().log()           # natural-log sum-exp of each split; -inf where it is empty
    wts = torch.softmax(lse, 0)
    ref = (wts[:, :, None] * torch.nan_to_num(part.double(), nan=0.0)).sum(0)
    assert bool(torch.isfinite(got.float()).all())
    rel = 2.0 ** (-11 if dtype == torch.float16 else -8)
    bound = ref.abs() * (rel + 1e-6) + 1e-7
    assert bool(((got.double() - ref).abs() <= bound).all()), float(((got.double() - ref).abs() - bound).max())
    only = [0, 7, rows - 1] if splits > 2 else []
    for r in only:                                           # a single live split: its row, whatever its weight
        assert torch.equal(got[r].view(torch.int16), part[splits - 1, r].view(torch.int16))
