"""The token-side block kernels of the two-way decoder without a GPU: the C entries refuse what their kernels cannot take (fake pointers: a
refused call launches nothing), the truth table of msam2_decoder_tokens_supported, and the Python gate (taken only on the inference
decoder's request, for the one configuration that is built, never with MSAM2_NO_FUSED_DEC_TOKENS=1)."""
import ctypes

import pytest
import torch

import medical_sam2_amd.modeling.sam_heads as sh
import medical_sam2_amd.ops as ops
from medical_sam2_amd import _lib

ERR_ARG = -1          # MSAM2_ERR_ARG: a call that got past its argument checks fails too without a GPU, with MSAM2_ERR_LAUNCH (-2)


def _ptr():
    buf = ctypes.create_string_buffer(4096)
    return buf, (ctypes.addressof(buf) + 15) & ~15


def _self(L, p, **k):
    a = dict(queries=p, query_pe=p, skip=0, w_qkv=p, b_qkv=p, w_out=p, b_out=p, ln_w=p, ln_b=p, w_cq=p, b_cq=p, out=p, qp=p, B=4, T=8, C=256, heads=8)
    a.update(k)
    return L.msam2_decoder_tokens_self(a["queries"], a["query_pe"], a["skip"], a["w_qkv"], a["b_qkv"], a["w_out"], a["b_out"], a["ln_w"], a["ln_b"],
                                       1e-5, a["w_cq"], a["b_cq"], a["out"], a["qp"], a["B"], a["T"], a["C"], a["heads"], None)


def _mlp(L, p, **k):
    a = dict(o=p, o_part=None, splits=0, queries=p, w_out=p, b_out=p, ln2_w=p, ln2_b=p, w1=p, b1=p, w2=p, b2=p, ln3_w=p, ln3_b=p, query_pe=p, w_kv=p, b_kv=p, w_fq=None,
             b_fq=None, mid=p, out=p, kv=p, qp_final=None, ws=p, ws_bytes=1 << 20, B=4, T=8, C=256, heads=8, hidden=2048)
    a.update(k)
    return L.msam2_decoder_tokens_mlp(a["o"], a["o_part"], a["splits"], a["queries"], a["w_out"], a["b_out"], a["ln2_w"], a["ln2_b"], 1e-5, a["w1"], a["b1"], a["w2"], a["b2"],
                                      a["ln3_w"], a["ln3_b"], 1e-5, a["query_pe"], a["w_kv"], a["b_kv"], a["w_fq"], a["b_fq"], a["mid"], a["out"],
                                      a["kv"], a["qp_final"], a["ws"], a["ws_bytes"], a["B"], a["T"], a["C"], a["heads"], a["hidden"], None)


def _tail(L, p, **k):
    a = dict(o=p, o_part=None, splits=0, queries=p, w_out=p, b_out=p, ln_w=p, ln_b=p, out=p, B=4, T=8, C=256, heads=8)
    a.update(k)
    return L.msam2_decoder_tokens_tail(a["o"], a["o_part"], a["splits"], a["queries"], a["w_out"], a["b_out"], a["ln_w"], a["ln_b"], 1e-5, a["out"], a["B"], a["T"], a["C"],
                                       a["heads"], None)


def _ks(L, p, **k):
    a = dict(q=p, k=p, v=p, part=p, q_bs=1024, q_ts=128, k_bs=384 * 4096, k_ts=384, B=4, H=8, Lq=8, Lk=4096, D=16, splits=4)
    a.update(k)
    return L.msam2_attention_fewq_keysplit(a["q"], a["q_bs"], a["q_ts"], a["k"], a["k_bs"], a["k_ts"], a["v"], a["k_bs"], a["k_ts"], a["part"], a["B"],
                                           a["H"], a["Lq"], a["Lk"], a["D"], a["splits"], 0.25, None)


def test_refusals_of_the_c_entries():
    L = _lib.lib()
    keep, p = _ptr()
    cases = {
        "decoder_tokens_self: null queries": lambda: _self(L, p, queries=None),
        "decoder_tokens_self: null query_pe": lambda: _self(L, p, query_pe=None),
        "decoder_tokens_self: null w_cq": lambda: _self(L, p, w_cq=None),
        "decoder_tokens_self: null qp": lambda: _self(L, p, qp=None),
        "decoder_tokens_self: queries misaligned": lambda: _self(L, p, queries=p + 4),
        "decoder_tokens_self: w_qkv misaligned": lambda: _self(L, p, w_qkv=p + 8),
        "decoder_tokens_self: qp misaligned": lambda: _self(L, p, qp=p + 2),
        "decoder_tokens_self: R = 33": lambda: _self(L, p, B=3, T=11),
        "decoder_tokens_self: R = 40": lambda: _self(L, p, B=5, T=8),
        "decoder_tokens_self: T = 17": lambda: _self(L, p, B=1, T=17),
        "decoder_tokens_self: T = 0": lambda: _self(L, p, T=0),
        "decoder_tokens_self: B = 0": lambda: _self(L, p, B=0),
        "decoder_tokens_self: C": lambda: _self(L, p, C=128),
        "decoder_tokens_self: heads": lambda: _self(L, p, heads=4),
        "decoder_tokens_mlp: null o": lambda: _mlp(L, p, o=None),
        "decoder_tokens_mlp: null w2": lambda: _mlp(L, p, w2=None),
        "decoder_tokens_mlp: o and partials": lambda: _mlp(L, p, o_part=p, splits=4),
        "decoder_tokens_mlp: 9 splits": lambda: _mlp(L, p, o=None, o_part=p, splits=9),
        "decoder_tokens_mlp: 0 splits": lambda: _mlp(L, p, o=None, o_part=p, splits=0),
        "decoder_tokens_mlp: null workspace": lambda: _mlp(L, p, ws=None),
        "decoder_tokens_mlp: w_fq without b_fq": lambda: _mlp(L, p, w_fq=p, qp_final=p),
        "decoder_tokens_mlp: w_fq without qp_final": lambda: _mlp(L, p, w_fq=p, b_fq=p),
        "decoder_tokens_mlp: o misaligned": lambda: _mlp(L, p, o=p + 8),
        "decoder_tokens_mlp: b1 misaligned": lambda: _mlp(L, p, b1=p + 4),
        "decoder_tokens_mlp: workspace misaligned": lambda: _mlp(L, p, ws=p + 8),
        "decoder_tokens_mlp: kv misaligned": lambda: _mlp(L, p, kv=p + 2),
        "decoder_tokens_mlp: workspace too small": lambda: _mlp(L, p, ws_bytes=16 * 32 * 256 * 4 - 1),
        "decoder_tokens_mlp: R = 36": lambda: _mlp(L, p, B=4, T=9),
        "decoder_tokens_mlp: T = 17": lambda: _mlp(L, p, B=1, T=17),
        "decoder_tokens_mlp: hidden": lambda: _mlp(L, p, hidden=1024),
        "decoder_tokens_mlp: C": lambda: _mlp(L, p, C=384),
        "decoder_tokens_tail: null o": lambda: _tail(L, p, o=None),
        "decoder_tokens_tail: null out": lambda: _tail(L, p, out=None),
        "decoder_tokens_tail: o and partials": lambda: _tail(L, p, o_part=p, splits=4),
        "decoder_tokens_tail: 9 splits": lambda: _tail(L, p, o=None, o_part=p, splits=9),
        "attention_fewq_keysplit: null part": lambda: _ks(L, p, part=None),
        "attention_fewq_keysplit: D": lambda: _ks(L, p, D=32),
        "attention_fewq_keysplit: Lq": lambda: _ks(L, p, Lq=33),
        "attention_fewq_keysplit: Lk": lambda: _ks(L, p, Lk=4097),
        "attention_fewq_keysplit: splits": lambda: _ks(L, p, splits=9),
        "attention_fewq_keysplit: stride": lambda: _ks(L, p, k_ts=12),
        "attention_fewq_keysplit: k misaligned": lambda: _ks(L, p, k=p + 8),
        "decoder_tokens_tail: w_out misaligned": lambda: _tail(L, p, w_out=p + 8),
        "decoder_tokens_tail: ln_b misaligned": lambda: _tail(L, p, ln_b=p + 8),
        "decoder_tokens_tail: R = 34": lambda: _tail(L, p, B=2, T=17),
        "decoder_tokens_tail: T = 32": lambda: _tail(L, p, B=1, T=32),
        "decoder_tokens_tail: heads": lambda: _tail(L, p, heads=16),
    }
    for what, call in cases.items():
        rc = call()
        msg = L.msam2_last_error().decode()
        assert rc == ERR_ARG, (what, rc, msg)
        assert what.split(":")[0] in msg, (what, msg)
    del keep


def test_workspace_size():
    L = _lib.lib()
    assert L.msam2_decoder_tokens_workspace_bytes(4, 8) == 16 * 32 * 256 * 4      # one fp32 [R, 256] partial per 128 hidden units
    assert L.msam2_decoder_tokens_workspace_bytes(1, 7) == 16 * 7 * 256 * 4
    assert L.msam2_decoder_tokens_workspace_bytes(5, 8) == 0 and L.msam2_decoder_tokens_workspace_bytes(1, 17) == 0


def test_split_count_fills_the_chip():
    L = _lib.lib()
    assert [L.msam2_attention_fewq_keysplit_splits(B, 8) for B in (1, 2, 4, 5, 8, 16, 32, 64)] == [8, 8, 4, 3, 2, 1, 1, 1]
    assert L.msam2_attention_fewq_keysplit_splits(0, 8) == 1


def test_truth_table_of_the_gate():
    ok = dict(C=256, heads=8, self_dim=256, cross_dim=128, hidden=2048, layers=2, act=ops.ACT_RELU, B=4, T=8)
    f = lambda **k: ops.decoder_tokens_supported(*{**ok, **k}.values())
    assert f()
    for B, T in [(1, 1), (1, 7), (1, 16), (2, 16), (4, 8), (3, 9), (5, 6), (32, 1)]:
        assert f(B=B, T=T), (B, T)
    for B, T in [(1, 17), (3, 11), (5, 7), (33, 1), (0, 8), (4, 0), (-1, 8), (2, 32)]:
        assert not f(B=B, T=T), (B, T)
    for k in [dict(C=128), dict(C=384), dict(heads=4), dict(heads=16), dict(self_dim=128), dict(cross_dim=256), dict(cross_dim=64),
              dict(hidden=1024), dict(hidden=4096), dict(layers=3), dict(layers=1), dict(act=ops.ACT_GELU), dict(act=ops.ACT_NONE)]:
        assert not f(**k), k


def _block(**k):
    a = dict(embedding_dim=256, num_heads=8, mlp_dim=2048)
    a.update(k)
    return sh.TwoWayAttentionBlock(**a)


def test_python_gate(monkeypatch):
    monkeypatch.delenv("MSAM2_NO_FUSED_DEC_TOKENS", raising=False)
    blk = _block()
    assert blk.tokens_fused(4, 8, True) and blk.tokens_fused(2, 16, True) and blk.tokens_fused(1, 7, True)
    assert not blk.tokens_fused(4, 8, False)                                     # the training forwards' call form
    assert not blk.tokens_fused(5, 8, True) and not blk.tokens_fused(3, 11, True)   # R > 32
    assert not blk.tokens_fused(1, 17, True)                                     # T > 16
    assert not _block(activation=torch.nn.GELU).tokens_fused(4, 8, True)         # a non-ReLU MLP
    three = _block()
    three.mlp = sh.MLP(256, 2048, 256, num_layers=3, activation=torch.nn.ReLU)
    assert not three.tokens_fused(4, 8, True)                                    # a 3-layer MLP
    assert not _block(mlp_dim=1024).tokens_fused(4, 8, True)
    assert not _block(attention_downsample_rate=1).tokens_fused(4, 8, True)
    assert not _block(num_heads=4).tokens_fused(4, 8, True)
    monkeypatch.setenv("MSAM2_NO_FUSED_DEC_TOKENS", "1")                         # the A/B switch, read per call
    assert not blk.tokens_fused(4, 8, True)
    monkeypatch.setenv("MSAM2_NO_FUSED_DEC_TOKENS", "0")
    assert blk.tokens_fused(4, 8, True)


class _Old(Exception):
    pass


def test_run_takes_the_block_kernels_only_behind_the_gate(monkeypatch):
    """`run` with the kernels stubbed: the fused form behind the gate, today's first launch (ops.gemm_tokens) everywhere else"""
    monkeypatch.delenv("MSAM2_NO_FUSED_DEC_TOKENS", raising=False)

    def old(*a, **k):
        raise _Old()
    monkeypatch.setattr(sh.ops, "gemm_tokens", old)
    monkeypatch.setattr(sh.ops, "add_cast", old)
    monkeypatch.setattr(sh, "to_bf16", old)
    monkeypatch.setattr(sh.TwoWayAttentionBlock, "_run_tokens_fused", lambda self, *a: "fused")

    def run(blk, B, T, **k):
        z = torch.zeros(B * T, 256)
        try:
            return blk.run(z, torch.zeros(B * 16, 256), z, torch.zeros(16, 256), B, T, 16, **k)
        except _Old:
            return "old"
    blk = _block()
    assert run(blk, 4, 8, fused_tokens=True) == "fused"
    assert run(blk, 4, 8) == "old" and run(blk, 4, 8, fused_tokens=False) == "old"
    assert run(blk, 5, 8, fused_tokens=True) == "old"                            # R > 32
    assert run(_block(activation=torch.nn.GELU), 4, 8, fused_tokens=True) == "old"
    monkeypatch.setenv("MSAM2_NO_FUSED_DEC_TOKENS", "1")
    assert run(blk, 4, 8, fused_tokens=True) == "old"


def test_only_the_inference_decoder_asks_for_it():
    import inspect
    import medical_sam2_amd.autograd as ag
    import medical_sam2_amd.backward as bwd
    import medical_sam2_amd.training as tr
    import medical_sam2_amd.training_3d as tr3
    for mod in (ag, bwd, tr, tr3):                                   # the training forwards and the backward's recomputation keep their launches
        src = inspect.getsource(mod)
        assert "fused_tokens" not in src and "decoder_tokens" not in src, mod.__name__
    sig = inspect.signature(sh.MaskDecoder.predict_masks_tokens)
    assert sig.parameters["fused_tokens"].default is False
    assert inspect.signature(sh.TwoWayTransformer.run).parameters["fused_tokens"].default is False
    assert inspect.signature(sh.TwoWayAttentionBlock.run).parameters["fused_tokens"].default is False
