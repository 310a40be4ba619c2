"""torch-tensor front end of the C-ABI (include/msam2_hip.h): every function extracts raw device pointers, sizes and
strides and calls libmsam2_hip.so on torch's current HIP stream.  PyTorch provides memory and streams only.

Layout conventions: activations are token-major ("NHWC") ``[rows, C]`` with C contiguous; bf16 for MFMA operands,
fp32 for residual streams / logits.  Weights follow nn.Linear (``[out, in]``).
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Tuple

import torch

from ._lib import check, lib

# 16-bit MFMA operand dtype of the loaded library: fp16 by default, bf16 when built with -DMSAM2_OPERAND_BF16
OP16 = torch.float16 if lib().msam2_operand_is_fp16() else torch.bfloat16

F32 = torch.float32
ACT_NONE, ACT_GELU, ACT_RELU, ACT_SIGMOID = 0, 1, 2, 3


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _is_bf16(t: torch.Tensor) -> int:
    """1 for the library's 16-bit operand dtype (OP16), 0 for fp32."""
    if t.dtype == OP16:
        return 1
    if t.dtype == F32:
        return 0
    raise TypeError(f"expected {OP16} or fp32 tensor, got {t.dtype}")


def _req(cond: bool, msg: str):
    if not cond:
        raise ValueError(msg)


# ---------------------------------------------------------------------------------------------------------------------
def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *, act: int = ACT_NONE,
         colscale: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, res_mod: int = 0,
         out_dtype: torch.dtype = OP16, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[M,N] = residual + colscale * act(a[M,K] @ w[N,K]^T + bias).  a, w bf16; bias/colscale fp32."""
    _req(a.dim() == 2 and w.dim() == 2 and a.shape[1] == w.shape[1], f"gemm shapes {tuple(a.shape)} x {tuple(w.shape)}")
    _req(a.dtype == OP16 and w.dtype == OP16, "gemm operands must be 16-bit (ops.OP16)")
    _req(a.stride(1) == 1 and w.stride(1) == 1, "gemm operands must be K-contiguous")
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=out_dtype, device=a.device)
    _req(out.stride(1) == 1 and out.shape == (M, N), "gemm out must be [M,N] row-major")
    if residual is not None:
        _req(residual.dim() == 2 and residual.stride(1) == 1 and residual.shape[1] == N, "gemm residual must be [*,N]")
    check(lib().msam2_gemm(_p(a), a.stride(0), _p(w), w.stride(0), _p(bias), _p(colscale), _p(residual),
                                residual.stride(0) if residual is not None else 0,
                                _is_bf16(residual) if residual is not None else 0, res_mod, _p(out), out.stride(0),
                                _is_bf16(out), M, N, K, act, _stream()))
    return out


def gemm_tokens(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *, addend: Optional[torch.Tensor] = None,
                add_cols: int = 0, act: int = ACT_NONE, residual: Optional[torch.Tensor] = None, out_dtype: torch.dtype = OP16) -> torch.Tensor:
    """out[M,N] = residual + act((a [+ addend on columns < add_cols]) @ w^T + bias) for M <= 32 fp32 token rows (a, addend fp32
    [M,K] row-major, w 16-bit [N,K]); add_cols must be a multiple of 32 (or >= N for all columns)."""
    _req(a.dim() == 2 and a.dtype == F32 and a.stride(1) == 1 and a.shape[0] <= 32, "gemm_tokens: a must be fp32 [M<=32, K]")
    _req(w.dtype == OP16 and w.stride(1) == 1 and w.shape[1] == a.shape[1], "gemm_tokens: w must be 16-bit [N, K]")
    if addend is not None:
        _req(addend.dtype == F32 and addend.shape == a.shape and addend.stride(1) == 1 and addend.stride(0) == a.stride(0),
             "gemm_tokens: addend must match a")
    M, K = a.shape
    N = w.shape[0]
    out = torch.empty(M, N, dtype=out_dtype, device=a.device)
    if residual is not None:
        _req(residual.dtype == F32 and residual.shape == (M, N) and residual.stride(1) == 1, "gemm_tokens: residual must be fp32 [M,N]")
    check(lib().msam2_gemm_tokens(_p(a), a.stride(0), _p(addend), add_cols if addend is not None else 0, _p(w), w.stride(0), _p(bias),
                                  _p(residual), residual.stride(0) if residual is not None else 0, _p(out), out.stride(0), _is_bf16(out),
                                  M, N, K, act, _stream()))
    return out


def decoder_tokens_supported(C: int, heads: int, self_dim: int, cross_dim: int, mlp_hidden: int, mlp_layers: int, mlp_act: int,
                             B: int, T: int) -> bool:
    """True when the `decoder_tokens_*` block kernels are built for this two-way block and B images of T tokens."""
    return bool(lib().msam2_decoder_tokens_supported(C, heads, self_dim, cross_dim, mlp_hidden, mlp_layers, mlp_act, B, T))


def _dec_rows(name: str, t: torch.Tensor, rows: int, cols: int, dtype: torch.dtype):
    _req(t.dtype == dtype and t.shape == (rows, cols) and t.is_contiguous(), f"{name} must be a contiguous {dtype} [{rows}, {cols}]")


def attention_fewq_keysplit(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, splits: Optional[int] = None):
    """Tokens -> image attention of the two-way decoder (head dim 16, q [B, Lq <= 32, C], k / v [B, Lk <= 4096, C], 16-bit) with every (batch,
    head)'s keys split over `splits` workgroups (default: enough to fill the chip).  Returns (fp32 partials [B*heads*splits, Lq, 18], splits) for
    `decoder_tokens_mlp` / `decoder_tokens_tail`, which merge them; nothing is normalised here."""
    B, Lq, C = q.shape
    Lk = k.shape[1]
    for t in (q, k, v):
        _req(t.dtype == OP16 and t.stride(2) == 1, "attention_fewq_keysplit tensors must be 16-bit (ops.OP16), channel-contiguous")
    if splits is None:
        splits = int(lib().msam2_attention_fewq_keysplit_splits(B, heads))
    part = torch.empty(B * heads * splits, Lq, 18, dtype=F32, device=q.device)
    check(lib().msam2_attention_fewq_keysplit(_p(q), q.stride(0), q.stride(1), _p(k), k.stride(0), k.stride(1), _p(v), v.stride(0), v.stride(1),
                                              _p(part), B, heads, Lq, Lk, C // heads, splits, 1.0 / math.sqrt(C // heads), _stream()))
    return part, splits


def _dec_attn_out(name: str, o, R: int, T: int, C: int, heads: int):
    """the attention output a token kernel takes: 16-bit rows [R, C/2] -> (o, None, 0); (partials, splits) of `attention_fewq_keysplit` -> (None, partials, splits)"""
    if isinstance(o, tuple):
        part, splits = o
        _req(part.dtype == F32 and part.is_contiguous() and part.shape == ((R // T) * heads * splits, T, 18), f"{name}: partials must be fp32 [B*heads*splits, T, 18]")
        return None, part, splits
    _dec_rows(f"{name}: o", o, R, C // 2, OP16)
    return o, None, 0


def decoder_tokens_self(queries: torch.Tensor, query_pe: torch.Tensor, skip_first_layer_pe: bool, w_qkv: torch.Tensor, b_qkv: torch.Tensor,
                        w_out: torch.Tensor, b_out: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor, eps: float, w_cq: torch.Tensor,
                        b_cq: torch.Tensor, B: int, T: int, heads: int):
    """Self-attention half of a two-way block on the token rows (fp32 [B*T, C]) as one launch: returns (queries after norm1, fp32;
    the tokens -> image query projection of queries + query_pe, 16-bit [B*T, C/2])."""
    R, C = B * T, queries.shape[1]
    _dec_rows("decoder_tokens_self: queries", queries, R, C, F32)
    _dec_rows("decoder_tokens_self: query_pe", query_pe, R, C, F32)
    _dec_rows("decoder_tokens_self: w_qkv", w_qkv, 3 * C, C, OP16)
    _dec_rows("decoder_tokens_self: w_out", w_out, C, C, OP16)
    _dec_rows("decoder_tokens_self: w_cq", w_cq, C // 2, C, OP16)
    for v, n in ((b_qkv, 3 * C), (b_out, C), (ln_w, C), (ln_b, C), (b_cq, C // 2)):
        _req(v.dtype == F32 and v.is_contiguous() and v.numel() == n, "decoder_tokens_self: biases and LayerNorm vectors are fp32, contiguous")
    out = torch.empty(R, C, dtype=F32, device=queries.device)
    qp = torch.empty(R, C // 2, dtype=OP16, device=queries.device)
    check(lib().msam2_decoder_tokens_self(_p(queries), _p(query_pe), int(bool(skip_first_layer_pe)), _p(w_qkv), _p(b_qkv), _p(w_out), _p(b_out),
                                          _p(ln_w), _p(ln_b), eps, _p(w_cq), _p(b_cq), _p(out), _p(qp), B, T, C, heads, _stream()))
    return out, qp


def decoder_tokens_mlp(o, queries: torch.Tensor, w_out: torch.Tensor, b_out: torch.Tensor, ln2_w: torch.Tensor, ln2_b: torch.Tensor,
                       eps2: float, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, ln3_w: torch.Tensor,
                       ln3_b: torch.Tensor, eps3: float, query_pe: torch.Tensor, w_kv: torch.Tensor, b_kv: torch.Tensor, B: int, T: int,
                       heads: int, w_fq: Optional[torch.Tensor] = None, b_fq: Optional[torch.Tensor] = None):
    """MLP half of a two-way block on the token rows as two launches: o (16-bit [B*T, C/2], the tokens -> image attention's output, or the
    (partials, splits) pair of `attention_fewq_keysplit`) ->
    (queries after norm3, fp32; the image -> token k | v projection, 16-bit [B*T, C]; with w_fq / b_fq the final attention's query
    projection, 16-bit [B*T, C/2], else None).  The workspace of the fc2 partials is allocated per call."""
    R, C = B * T, queries.shape[1]
    hidden = w1.shape[0]
    o, o_part, splits = _dec_attn_out("decoder_tokens_mlp", o, R, T, C, heads)
    _dec_rows("decoder_tokens_mlp: queries", queries, R, C, F32)
    _dec_rows("decoder_tokens_mlp: query_pe", query_pe, R, C, F32)
    _dec_rows("decoder_tokens_mlp: w_out", w_out, C, C // 2, OP16)
    _dec_rows("decoder_tokens_mlp: w1", w1, hidden, C, OP16)
    _dec_rows("decoder_tokens_mlp: w2", w2, C, hidden, OP16)
    _dec_rows("decoder_tokens_mlp: w_kv", w_kv, C, C, OP16)
    vecs = [(b_out, C), (ln2_w, C), (ln2_b, C), (b1, hidden), (b2, C), (ln3_w, C), (ln3_b, C), (b_kv, C)]
    _req((w_fq is None) == (b_fq is None), "decoder_tokens_mlp: w_fq and b_fq come together")
    if w_fq is not None:
        _dec_rows("decoder_tokens_mlp: w_fq", w_fq, C // 2, C, OP16)
        vecs.append((b_fq, C // 2))
    for v, n in vecs:
        _req(v.dtype == F32 and v.is_contiguous() and v.numel() == n, "decoder_tokens_mlp: biases and LayerNorm vectors are fp32, contiguous")
    dev = queries.device
    mid = torch.empty(R, C, dtype=F32, device=dev)
    out = torch.empty(R, C, dtype=F32, device=dev)
    kv = torch.empty(R, C, dtype=OP16, device=dev)
    qp = torch.empty(R, C // 2, dtype=OP16, device=dev) if w_fq is not None else None
    nbytes = max(int(lib().msam2_decoder_tokens_workspace_bytes(B, T)), 16)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(lib().msam2_decoder_tokens_mlp(_p(o), _p(o_part), splits, _p(queries), _p(w_out), _p(b_out), _p(ln2_w), _p(ln2_b), eps2, _p(w1), _p(b1), _p(w2), _p(b2),
                                         _p(ln3_w), _p(ln3_b), eps3, _p(query_pe), _p(w_kv), _p(b_kv), _p(w_fq), _p(b_fq), _p(mid), _p(out),
                                         _p(kv), _p(qp), _p(ws), nbytes, B, T, C, heads, hidden, _stream()))
    return out, kv, qp


def decoder_tokens_tail(o, queries: torch.Tensor, w_out: torch.Tensor, b_out: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor,
                        eps: float, B: int, T: int, heads: int) -> torch.Tensor:
    """End of the two-way transformer on the token rows: LayerNorm(queries + o @ w_out^T + b_out), fp32 [B*T, C], one launch; o as
    `decoder_tokens_mlp` takes it."""
    R, C = B * T, queries.shape[1]
    o, o_part, splits = _dec_attn_out("decoder_tokens_tail", o, R, T, C, heads)
    _dec_rows("decoder_tokens_tail: queries", queries, R, C, F32)
    _dec_rows("decoder_tokens_tail: w_out", w_out, C, C // 2, OP16)
    for v in (b_out, ln_w, ln_b):
        _req(v.dtype == F32 and v.is_contiguous() and v.numel() == C, "decoder_tokens_tail: bias and LayerNorm vectors are fp32 [C], contiguous")
    out = torch.empty(R, C, dtype=F32, device=queries.device)
    check(lib().msam2_decoder_tokens_tail(_p(o), _p(o_part), splits, _p(queries), _p(w_out), _p(b_out), _p(ln_w), _p(ln_b), eps, _p(out), B, T, C, heads, _stream()))
    return out


def gemm_pool2x2(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], B: int, H: int, W: int) -> torch.Tensor:
    """fp32 [B*(H/2)*(W/2), N] = maxpool2x2(a @ w^T + bias) over the [B,H,W] token image a [B*H*W, K] (16-bit, K-contiguous)."""
    _req(a.dim() == 2 and w.dim() == 2 and a.shape[1] == w.shape[1] and a.shape[0] == B * H * W, "gemm_pool2x2 shapes")
    _req(a.dtype == OP16 and w.dtype == OP16 and a.stride(1) == 1 and w.stride(1) == 1, "gemm_pool2x2 operands: 16-bit, K-contiguous")
    N, K = w.shape
    out = torch.empty(B * (H // 2) * (W // 2), N, dtype=F32, device=a.device)
    check(lib().msam2_gemm_pool2x2(_p(a), a.stride(0), _p(w), w.stride(0), _p(bias), _p(out), out.stride(0), B, H, W, N, K, _stream()))
    return out


def gemm_qkv_pool2x2(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], B: int, H: int, W: int, q_cols: int):
    """Fused qkv projection of a q-pooling block: returns (qkv 16-bit [B*H*W, N] whose columns >= q_cols hold k | v in image order --
    the q columns are left unwritten --, q_pooled 16-bit [B*(H/2)*(W/2), q_cols] = maxpool2x2 of the q columns)."""
    _req(a.dim() == 2 and w.dim() == 2 and a.shape[1] == w.shape[1] and a.shape[0] == B * H * W, "gemm_qkv_pool2x2 shapes")
    _req(a.dtype == OP16 and w.dtype == OP16 and a.stride(1) == 1 and w.stride(1) == 1, "gemm_qkv_pool2x2 operands: 16-bit, K-contiguous")
    N, K = w.shape
    qkv = torch.empty(B * H * W, N, dtype=OP16, device=a.device)
    q2 = torch.empty(B * (H // 2) * (W // 2), q_cols, dtype=OP16, device=a.device)
    check(lib().msam2_gemm_qkv_pool2x2(_p(a), a.stride(0), _p(w), w.stride(0), _p(bias), _p(qkv), qkv.stride(0), _p(q2), q2.stride(0),
                                       B, H, W, N, K, q_cols, _stream()))
    return qkv, q2


def gemm_rope(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], table: Tuple[torch.Tensor, torch.Tensor], *,
              rope_cols: int, head_dim: int, rows_per_batch: int, n_rope: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """16-bit out[M,N] = rope(a @ w^T + bias): columns < rope_cols (whole heads of head_dim channels) of rows whose position
    m % rows_per_batch is < n_rope are rotated with table row (m % rows_per_batch) % n_pos -- the q/k projections of RoPEAttention
    with the rotation applied to the fp32 accumulator in the store."""
    _req(a.dim() == 2 and w.dim() == 2 and a.shape[1] == w.shape[1], f"gemm_rope shapes {tuple(a.shape)} x {tuple(w.shape)}")
    _req(a.dtype == OP16 and w.dtype == OP16 and a.stride(1) == 1 and w.stride(1) == 1, "gemm_rope operands: 16-bit, K-contiguous")
    cs, sn = table
    _req(cs.dtype == F32 and cs.is_contiguous() and sn.is_contiguous() and cs.shape == sn.shape and cs.shape[1] * 2 == head_dim,
         "gemm_rope: table must be cos/sin fp32 [n_pos, head_dim/2]")
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=OP16, device=a.device)
    _req(out.dtype == OP16 and out.shape == (M, N) and out.stride(1) == 1, "gemm_rope: out must be 16-bit [M, N] row-major")
    check(lib().msam2_gemm_rope(_p(a), a.stride(0), _p(w), w.stride(0), _p(bias), _p(out), out.stride(0), M, N, K, _p(cs), _p(sn),
                                rope_cols, head_dim, rows_per_batch, n_rope, cs.shape[0], _stream()))
    return out


def layernorm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float, *, act: int = ACT_NONE,
              out_dtype: torch.dtype = OP16) -> torch.Tensor:
    """Row LayerNorm over the last dim of a [rows, C] tensor (C contiguous)."""
    C = x.shape[-1]
    x2 = x.reshape(-1, C)
    _req(x2.stride(1) == 1, "layernorm input rows must be contiguous")
    y = torch.empty(x2.shape, dtype=out_dtype, device=x.device)
    check(lib().msam2_layernorm(_p(x2), _is_bf16(x2), x2.stride(0), _p(weight), _p(bias), _p(y), _is_bf16(y), y.stride(0),
                                x2.shape[0], C, eps, act, _stream()))
    return y.reshape(x.shape)


def layernorm_dual(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float):
    """fp32 [rows, C] -> (LayerNorm rows in fp32, the same rows in the 16-bit operand type) from one launch"""
    C = x.shape[-1]
    x2 = x.reshape(-1, C)
    _req(x2.dtype == F32 and x2.stride(1) == 1 and C % 4 == 0, "layernorm_dual: fp32 rows, C % 4 == 0")
    y = torch.empty(x2.shape, dtype=F32, device=x.device)
    y16 = torch.empty(x2.shape, dtype=OP16, device=x.device)
    check(lib().msam2_layernorm_dual(_p(x2), x2.stride(0), _p(weight), _p(bias), _p(y), y.stride(0), _p(y16), y16.stride(0), x2.shape[0], C, eps,
                                     _stream()))
    return y.reshape(x.shape), y16.reshape(x.shape)


def _rowln_outputs(name: str, residual: torch.Tensor, M: Optional[int], N: int, ln_w: torch.Tensor, ln_b: torch.Tensor, biases, vectors_text: str,
                   out: Optional[torch.Tensor], out16: Optional[torch.Tensor], device):
    """The output side of the three full-row wrappers, checked in their order: residual fp32 [M, N] (M None: the residual's rows give M);
    ln_w, ln_b fp32 [N] and every (bias or None, length) of `biases` fp32 contiguous, named by `vectors_text`; out / out16 allocated on
    `device` where None, then validated.  Returns (M, out, out16)."""
    _req(residual.dim() == 2 and residual.dtype == F32 and residual.shape == (residual.shape[0] if M is None else M, N) and residual.stride(1) == 1,
         f"{name}: residual must be fp32 [M, N]")
    M = residual.shape[0]
    _req(ln_w.dtype == F32 and ln_b.dtype == F32 and ln_w.numel() == N and ln_b.numel() == N and ln_w.is_contiguous() and ln_b.is_contiguous()
         and all(b is None or (b.dtype == F32 and b.numel() == n and b.is_contiguous()) for b, n in biases),
         f"{name}: {vectors_text}")
    if out is None:
        out = torch.empty(M, N, dtype=F32, device=device)
    if out16 is None:
        out16 = torch.empty(M, N, dtype=OP16, device=device)
    _req(out.dtype == F32 and out.shape == (M, N) and out.stride(1) == 1 and out16.dtype == OP16 and out16.shape == (M, N) and out16.stride(1) == 1,
         f"{name}: out is fp32 [M, N], out16 16-bit [M, N], rows contiguous")
    return M, out, out16


def gemm_residual_layernorm_supported(N: int, K: int) -> bool:
    """True when `gemm_residual_layernorm` is built for this output width and reduction length (per-slice quantities only)."""
    return bool(lib().msam2_gemm_residual_layernorm_supported(N, K))


def gemm_residual_layernorm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], residual: torch.Tensor, ln_w: torch.Tensor,
                            ln_b: torch.Tensor, eps: float, *, out: Optional[torch.Tensor] = None, out16: Optional[torch.Tensor] = None):
    """(c32, y16) = (a @ w^T + bias + residual in fp32, LayerNorm(c32 rows) in the 16-bit operand type) from one kernel: the bits of
    `gemm(a, w, bias, residual=residual, out_dtype=F32)` and of `layernorm(c32, ln_w, ln_b, eps)`.  a [M, K], w [N, K] 16-bit, residual fp32
    [M, N].  A form that is not built (`gemm_residual_layernorm_supported`) is an error."""
    _req(a.dim() == 2 and w.dim() == 2 and a.shape[1] == w.shape[1], f"gemm_residual_layernorm shapes {tuple(a.shape)} x {tuple(w.shape)}")
    _req(a.dtype == OP16 and w.dtype == OP16 and a.stride(1) == 1 and w.stride(1) == 1, "gemm_residual_layernorm operands: 16-bit, K-contiguous")
    M, K = a.shape
    N = w.shape[0]
    _req(gemm_residual_layernorm_supported(N, K),
         f"gemm_residual_layernorm: N = {N}, K = {K} is not built (N = 384 with K % 64 == 0; N = 256 with K = 64, 256 or 2048)")
    M, out, out16 = _rowln_outputs("gemm_residual_layernorm", residual, M, N, ln_w, ln_b, ((bias, N),), "bias, ln_w, ln_b are fp32 [N]", out, out16,
                                   a.device)
    check(lib().msam2_gemm_residual_layernorm(_p(a), a.stride(0), _p(w), w.stride(0), _p(bias), _p(residual), residual.stride(0), _p(out),
                                              out.stride(0), _p(ln_w), _p(ln_b), float(eps), _p(out16), out16.stride(0), M, N, K, _stream()))
    return out, out16


def mlp_residual_layernorm_supported(N: int, H: int) -> bool:
    """True when `mlp_residual_layernorm` is built for this width and hidden width (per-slice quantities only)."""
    return bool(lib().msam2_mlp_residual_layernorm_supported(N, H))


def mlp_residual_layernorm(a: torch.Tensor, w1: torch.Tensor, b1: Optional[torch.Tensor], w2: torch.Tensor, b2: Optional[torch.Tensor],
                           residual: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor, eps: float, *, out: Optional[torch.Tensor] = None,
                           out16: Optional[torch.Tensor] = None):
    """(c32, y16) = (gelu(a @ w1^T + b1) @ w2^T + b2 + residual in fp32, LayerNorm(c32 rows) in the 16-bit operand type) from one kernel;
    the hidden activations are rounded to the operand type and never leave the chip: the bits of `gemm(a, w1, b1, act=ACT_GELU)` followed
    by `gemm_residual_layernorm(h, w2, b2, residual, ...)`.  a [M, N], w1 [H, N], w2 [N, H] 16-bit as stored, residual fp32 [M, N].  A form
    that is not built (`mlp_residual_layernorm_supported`) is an error."""
    _req(a.dim() == 2 and w1.dim() == 2 and w2.dim() == 2 and a.shape[1] == w1.shape[1] and w2.shape == (w1.shape[1], w1.shape[0]),
         f"mlp_residual_layernorm shapes {tuple(a.shape)} x {tuple(w1.shape)} x {tuple(w2.shape)}")
    _req(a.dtype == OP16 and w1.dtype == OP16 and w2.dtype == OP16 and a.stride(1) == 1 and w1.stride(1) == 1 and w2.stride(1) == 1,
         "mlp_residual_layernorm operands: 16-bit, reduction dimension contiguous")
    M, N = a.shape
    H = w1.shape[0]
    _req(mlp_residual_layernorm_supported(N, H), f"mlp_residual_layernorm: N = {N}, H = {H} is not built (N = 384 with H % 128 == 0)")
    M, out, out16 = _rowln_outputs("mlp_residual_layernorm", residual, M, N, ln_w, ln_b, ((b1, H), (b2, N)),
                                   "b1 is fp32 [H]; b2, ln_w, ln_b are fp32 [N]", out, out16, a.device)
    check(lib().msam2_mlp_residual_layernorm_fwd(_p(a), a.stride(0), _p(w1), w1.stride(0), _p(b1), _p(w2), w2.stride(0), _p(b2), _p(residual),
                                                 residual.stride(0), _p(out), out.stride(0), _p(ln_w), _p(ln_b), float(eps), _p(out16),
                                                 out16.stride(0), M, N, H, _stream()))
    return out, out16


def gemm_merged_residual_layernorm_supported(N: int, D: int, splits: int) -> bool:
    """True when `gemm_merged_residual_layernorm` is built for this output width, head dim and (effective) split count."""
    return bool(lib().msam2_gemm_merged_residual_layernorm_supported(N, D, splits))


def gemm_merged_residual_layernorm(workspace: torch.Tensor, splits: int, D: int, w: torch.Tensor, bias: Optional[torch.Tensor],
                                   residual: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor, eps: float, *,
                                   out: Optional[torch.Tensor] = None, out16: Optional[torch.Tensor] = None):
    """`gemm_residual_layernorm` on the rows `attention_merge` would write: `workspace` holds the partials of an attention call made
    with defer_merge=True for one head and M = residual.shape[0] query rows, `splits` is the EFFECTIVE count (attention_effective_splits).
    (c32, y16) have the bits of attention_merge -> gemm(fp32 + residual) -> layernorm; the merged rows are written nowhere."""
    _req(w.dim() == 2 and w.dtype == OP16 and w.stride(1) == 1 and w.shape[1] == D, f"gemm_merged_residual_layernorm: w is 16-bit [N, {D}], K-contiguous")
    _req(workspace.dtype == torch.uint8 and workspace.is_contiguous(), "gemm_merged_residual_layernorm: workspace is a contiguous uint8 buffer")
    N = w.shape[0]
    M, out, out16 = _rowln_outputs("gemm_merged_residual_layernorm", residual, None, N, ln_w, ln_b, ((bias, N),), "bias, ln_w, ln_b are fp32 [N]",
                                   out, out16, w.device)
    check(lib().msam2_gemm_merged_residual_layernorm(_p(workspace), workspace.numel(), int(splits), int(D), _p(w), w.stride(0), _p(bias), _p(residual),
                                                     residual.stride(0), _p(out), out.stride(0), _p(ln_w), _p(ln_b), float(eps), _p(out16),
                                                     out16.stride(0), M, N, _stream()))
    return out, out16


def ln_mlp_residual_supported(dim: int) -> bool:
    return bool(lib().msam2_ln_mlp_residual_supported(dim))


def mlp_fused_permute_w2(w2: torch.Tensor) -> torch.Tensor:
    """kernel-ready copy of fc2's weight [dim, hidden] (16-bit) for ln_mlp_residual"""
    _req(w2.dim() == 2 and w2.dtype == OP16 and w2.is_contiguous() and w2.shape[1] % 32 == 0, "mlp_fused_permute_w2: 16-bit [dim, hidden]")
    out = torch.empty_like(w2)
    check(lib().msam2_mlp_fused_permute_w2(_p(w2), _p(out), w2.shape[0], w2.shape[1], _stream()))
    return out


def ln_mlp_residual(x: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor, eps: float, w1: torch.Tensor, b1: torch.Tensor, w2p: torch.Tensor,
                    b2: torch.Tensor, also16: bool = False):
    """fp32 [T, dim] = x + fc2(GELU(fc1(LayerNorm(x)))) in one kernel (dim 96 / 192, and 384 -- opt-in in the trunk: ln_mlp_residual_supported; w2p from
    mlp_fused_permute_w2, whose layout depends on dim).
    also16: returns (fp32 rows, the same rows in the 16-bit operand type) -- written by the same store."""
    T, dim = x.shape
    _req(x.dtype == F32 and x.is_contiguous() and w1.dtype == OP16 and w2p.dtype == OP16 and w1.shape == (4 * dim, dim) and w2p.shape == (dim, 4 * dim)
         and w1.is_contiguous() and w2p.is_contiguous(), "ln_mlp_residual: x fp32 [T, dim], w1 [4 dim, dim], w2p [dim, 4 dim] 16-bit contiguous")
    out = torch.empty_like(x)
    if also16:
        out16 = torch.empty(x.shape, dtype=OP16, device=x.device)
        check(lib().msam2_ln_mlp_residual_fwd_dual(_p(x), T, dim, _p(ln_w), _p(ln_b), float(eps), _p(w1), _p(b1), _p(w2p), _p(b2), _p(out), _p(out16),
                                                   _stream()))
        return out, out16
    check(lib().msam2_ln_mlp_residual_fwd(_p(x), T, dim, _p(ln_w), _p(ln_b), float(eps), _p(w1), _p(b1), _p(w2p), _p(b2), _p(out), _stream()))
    return out


def proj_ln_mlp_residual_supported(dim: int) -> bool:
    return bool(lib().msam2_proj_ln_mlp_residual_supported(dim))


def mlp_fused_permute_w1(w1: torch.Tensor) -> torch.Tensor:
    """kernel-ready copy of fc1's weight [hidden, dim] (16-bit) for proj_ln_mlp_residual: input index permuted per 32-block"""
    _req(w1.dim() == 2 and w1.dtype == OP16 and w1.is_contiguous() and w1.shape[1] % 32 == 0, "mlp_fused_permute_w1: 16-bit [hidden, dim]")
    out = torch.empty_like(w1)
    check(lib().msam2_mlp_fused_permute_w1(_p(w1), _p(out), w1.shape[0], w1.shape[1], _stream()))
    return out


def mlp_fused_w1_order(dim: int) -> torch.Tensor:
    """the permutation behind mlp_fused_permute_w1 / mlp_fused_permute_w2 (dim 96 / 192): index tensor `src` with permuted[..., i] = w[..., src[i]];
    position 16 s + 8 h + j of every 32-block holds element 16 s + 8 (j >> 2) + 4 h + (j & 3)"""
    i = torch.arange(dim)
    q = i & 31
    s, h, j = q >> 4, (q >> 3) & 1, q & 7
    return (i & ~31) + 16 * s + 8 * (j >> 2) + 4 * h + (j & 3)


def proj_ln_mlp_residual(o: torch.Tensor, wp: torch.Tensor, bp: torch.Tensor, res: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor, eps: float,
                         w1p: torch.Tensor, b1: torch.Tensor, w2p: torch.Tensor, b2: torch.Tensor, also16: bool = False, next_ln=None):
    """fp32 [T, dim] = x1 + fc2(GELU(fc1(LayerNorm(x1)))) with x1 = res + o wp^T + bp, one kernel, x1 never written (dim 96 / 192; w1p from
    mlp_fused_permute_w1, w2p from mlp_fused_permute_w2).  Returns (out, out16 or None, xn16 or None): out16 = the rows in the 16-bit operand type
    (also16), xn16 = LayerNorm(out rows; *next_ln) in that type (next_ln = (weight, bias, eps)) -- written by the same store."""
    T, dim = res.shape
    _req(res.dtype == F32 and res.is_contiguous() and o.dtype == OP16 and o.is_contiguous() and o.shape == (T, dim) and wp.dtype == OP16
         and wp.is_contiguous() and wp.shape == (dim, dim), "proj_ln_mlp_residual: res fp32 [T, dim], o 16-bit [T, dim], wp 16-bit [dim, dim] contiguous")
    _req(w1p.dtype == OP16 and w2p.dtype == OP16 and w1p.shape == (4 * dim, dim) and w2p.shape == (dim, 4 * dim) and w1p.is_contiguous()
         and w2p.is_contiguous(), "proj_ln_mlp_residual: w1p [4 dim, dim], w2p [dim, 4 dim] 16-bit contiguous")
    out = torch.empty_like(res)
    out16 = torch.empty(res.shape, dtype=OP16, device=res.device) if also16 else None
    xn16 = torch.empty(res.shape, dtype=OP16, device=res.device) if next_ln is not None else None
    nw, nb, neps = next_ln if next_ln is not None else (None, None, 0.0)
    check(lib().msam2_proj_ln_mlp_residual_fwd(_p(o), _p(wp), _p(bp), _p(res), T, dim, _p(ln_w), _p(ln_b), float(eps), _p(w1p), _p(b1), _p(w2p), _p(b2),
                                               _p(out), _p(out16), _p(nw), _p(nb), float(neps), _p(xn16), _stream()))
    return out, out16, xn16


def _strides3(t: torch.Tensor) -> "ctypes.Array":
    return (ctypes.c_int64 * 3)(t.stride(0), t.stride(1), t.stride(2))


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, splits: int = 1,
              out: Optional[torch.Tensor] = None, scale: Optional[float] = None, workspace: Optional[torch.Tensor] = None,
              defer_merge: bool = False, lse: Optional[torch.Tensor] = None, dropout: Optional[tuple] = None) -> torch.Tensor:
    """softmax(q k^T / sqrt(D)) v.  q [B,H,Lq,D], k/v [B,H,Lk,D] as (possibly strided) bf16 views with D contiguous.
    Returns [B,H,Lq,D] view of a [B,Lq,H,D] buffer (heads recombined for the following out-projection).
    defer_merge (needs a caller-owned `workspace`): run the split-KV pass only; finish with attention_merge().
    lse (fp32 [B,H,Lq] contiguous): also return the log-sum-exp rows (log2 domain) the backward needs; runs with >= 2 splits.
    dropout = (p, seed, offset) with lse: train-mode dropout on the attention probabilities inside the flash kernel (seed: int or
    DeviceSeed; probability (b,h,q,k) = element offset + ((b*H+h)*Lq+q)*Lk+k of the stream); `backward.attention_backward(...,
    dropout=...)` re-creates the mask."""
    B, H, Lq, D = q.shape
    Lk = k.shape[2]
    for t in (q, k, v):
        _req(t.dtype == OP16 and t.stride(3) == 1, "attention tensors must be 16-bit (ops.OP16) with contiguous head dim")
    if out is None:
        out = torch.empty(B, Lq, H, D, dtype=OP16, device=q.device).permute(0, 2, 1, 3)
    if lse is not None:
        _req(lse.dtype == F32 and lse.is_contiguous() and lse.numel() == B * H * Lq and not defer_merge, "attention: lse must be fp32 [B,H,Lq]")
        splits = max(splits, 2)
    ws_bytes = lib().msam2_attention_workspace_bytes(B, H, Lq, D, splits)
    ws = workspace if workspace is not None else (torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=q.device) if splits > 1 else None)
    _req(not defer_merge or (workspace is not None and splits > 1), "defer_merge needs splits > 1 and a caller-owned workspace")
    _req(ws is None or ws.numel() * ws.element_size() >= ws_bytes, "attention workspace too small")
    sc = scale if scale is not None else 1.0 / math.sqrt(D)
    if dropout is not None and dropout[0] > 0:
        _req(lse is not None, "attention: dropout is a training feature (pass lse)")
        pd, seed, offset = dropout
        seed_dev = None
        if isinstance(seed, DeviceSeed):
            seed, seed_dev = seed.base, seed.dev
        check(lib().msam2_attention_fwd_lse_dropout(_p(q), _strides3(q), _p(k), _strides3(k), _p(v), _strides3(v), _p(out), _strides3(out),
                                                    B, H, Lq, Lk, D, sc, splits, _p(ws), ws_bytes if ws is not None else 0, _p(lse), float(pd),
                                                    int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), _p(seed_dev), _stream()))
        return out
    if lse is not None:
        check(lib().msam2_attention_fwd_lse(_p(q), _strides3(q), _p(k), _strides3(k), _p(v), _strides3(v), _p(out), _strides3(out),
                                            B, H, Lq, Lk, D, sc, splits, _p(ws), ws_bytes if ws is not None else 0, _p(lse), _stream()))
        return out
    check(lib().msam2_attention_fwd(_p(q), _strides3(q), _p(k), _strides3(k), _p(v), _strides3(v), _p(out), _strides3(out),
                                    B, H, Lq, Lk, D, sc, -splits if defer_merge else splits, _p(ws), ws_bytes if ws is not None else 0, _stream()))
    return out


def attention_kv64(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, splits: int = 1, scale: Optional[float] = None,
                   workspace: Optional[torch.Tensor] = None, defer_merge: bool = False,
                   key_count: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """softmax(q k^T / sqrt(256)) v for q [B,H,Lq,256], k [B,H,Lk,256] and 64-wide value rows v [B,H,Lk,64] (the memory bank itself:
    the memory cross-attention with v_proj folded into out_proj).  Returns the [B,H,Lq,64] view of a [B,Lq,H,64] buffer (or `out`, a
    [B,H,Lq,64] view with contiguous rows).
    defer_merge: the split pass only (finish with attention_merge on the returned view).
    key_count: int32 device scalar in [1, Lk]: only the first `key_count` keys are attended to, Lk being the capacity the launch is
    shaped for (a hipGraph captured for a padded memory bank serves every fill level)."""
    B, H, Lq, D = q.shape
    Lk = k.shape[2]
    _req(D == 256 and k.shape[3] == 256 and v.shape[3] == 64 and v.shape[2] == Lk, "attention_kv64: q/k rows of 256, v rows of 64")
    _req(key_count is None or (key_count.dtype == torch.int32 and key_count.numel() == 1 and key_count.device == q.device),
         "attention_kv64: key_count is one int32 on the tensors' device")
    for t in (q, k, v):
        _req(t.dtype == OP16 and t.stride(3) == 1, "attention tensors must be 16-bit (ops.OP16) with contiguous head dim")
    if out is None:
        out = torch.empty(B, Lq, H, 64, dtype=OP16, device=q.device).permute(0, 2, 1, 3)
    _req(out.dtype == OP16 and out.shape == (B, H, Lq, 64) and out.stride(3) == 1, "attention_kv64: out is a 16-bit [B,H,Lq,64] view")
    ws_bytes = lib().msam2_attention_workspace_bytes(B, H, Lq, 64, splits)
    ws = workspace if workspace is not None else (torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=q.device) if splits > 1 else None)
    _req(not defer_merge or (workspace is not None and splits > 1), "defer_merge needs splits > 1 and a caller-owned workspace")
    _req(ws is None or ws.numel() * ws.element_size() >= ws_bytes, "attention workspace too small")
    sc = scale if scale is not None else 1.0 / math.sqrt(D)
    if key_count is not None:
        check(lib().msam2_attention_kv64_dyn_fwd(_p(q), _strides3(q), _p(k), _strides3(k), _p(v), _strides3(v), _p(out), _strides3(out),
                                                 B, H, Lq, Lk, _p(key_count), sc, -splits if defer_merge else splits, _p(ws),
                                                 ws_bytes if ws is not None else 0, _stream()))
        return out
    check(lib().msam2_attention_kv64_fwd(_p(q), _strides3(q), _p(k), _strides3(k), _p(v), _strides3(v), _p(out), _strides3(out),
                                         B, H, Lq, Lk, sc, -splits if defer_merge else splits, _p(ws), ws_bytes if ws is not None else 0, _stream()))
    return out


def attention_effective_splits(Lk: int, splits: int) -> int:
    return int(lib().msam2_attention_effective_splits(Lk, splits))


def attention_kv64_partial(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, splits: int, split_begin: int, split_count: int,
                           workspace: torch.Tensor, scale: Optional[float] = None, key_count: Optional[torch.Tensor] = None) -> None:
    """Splits [split_begin, split_begin + split_count) of a `splits`-way attention_kv64 (effective count) into `workspace`; finish with
    attention_merge on a [B,H,Lq,64] output view once every slot is filled (parallel.KVSplit all-gathers the other ranks' slots)."""
    B, H, Lq, D = q.shape
    Lk = k.shape[2]
    for t in (q, k, v):
        _req(t.dtype == OP16 and t.stride(3) == 1, "attention tensors must be 16-bit (ops.OP16) with contiguous head dim")
    sc = scale if scale is not None else 1.0 / math.sqrt(D)
    if key_count is not None:
        _req(key_count.dtype == torch.int32 and key_count.numel() == 1, "attention_kv64_partial: key_count is one int32 on the device")
        check(lib().msam2_attention_kv64_dyn_partial(_p(q), _strides3(q), _p(k), _strides3(k), _p(v), _strides3(v), B, H, Lq, Lk, _p(key_count),
                                                     sc, splits, split_begin, split_count, _p(workspace),
                                                     workspace.numel() * workspace.element_size(), _stream()))
        return
    check(lib().msam2_attention_kv64_partial(_p(q), _strides3(q), _p(k), _strides3(k), _p(v), _strides3(v), B, H, Lq, Lk, sc, splits,
                                             split_begin, split_count, _p(workspace), workspace.numel() * workspace.element_size(), _stream()))


def attention_workspace(B: int, H: int, Lq: int, D: int, splits: int, device) -> torch.Tensor:
    return torch.empty(max(lib().msam2_attention_workspace_bytes(B, H, Lq, D, splits), 1), dtype=torch.uint8, device=device)


def attention_merge(out: torch.Tensor, Lk: int, splits: int, workspace: torch.Tensor) -> torch.Tensor:
    """Finish attention(..., defer_merge=True): out is the [B,H,Lq,D] view that call returned."""
    B, H, Lq, D = out.shape
    check(lib().msam2_attention_merge(_p(out), _strides3(out), B, H, Lq, Lk, D, splits, _p(workspace),
                                      workspace.numel() * workspace.element_size(), _stream()))
    return out


def window_attention(qkv: torch.Tensor, B: int, H: int, W: int, heads: int, ws: int, qkv_bias: torch.Tensor,
                     q_pooled: Optional[torch.Tensor] = None, scale: Optional[float] = None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Hiera windowed MHA straight from the fused qkv tokens [B*H*W, 3*heads*D] (bf16); if q_pooled is given
    ([B*(H/2)*(W/2), heads*D]) queries come from it with window ws/2.  Returns o [B*Hq*Wq, heads*D] bf16."""
    dim_out = qkv.shape[1] // 3
    D = dim_out // heads
    _req(qkv.dtype == OP16 and qkv.stride(1) == 1, "qkv must be 16-bit (ops.OP16) row-major")
    if q_pooled is None:
        qt, q_ts, hq, wq, ws_q = qkv, qkv.stride(0), H, W, ws
    else:
        qt, q_ts, hq, wq, ws_q = q_pooled, q_pooled.stride(0), H // 2, W // 2, ws // 2
    o = out if out is not None else torch.empty(B * hq * wq, dim_out, dtype=OP16, device=qkv.device)
    _req(o.dtype == OP16 and o.shape == (B * hq * wq, dim_out) and o.stride(1) == 1, "window_attention: out is 16-bit [B*Hq*Wq, heads*D] rows")
    kpad = qkv_bias[dim_out:2 * dim_out]
    vpad = qkv_bias[2 * dim_out:]
    kptr = qkv.data_ptr() + dim_out * 2
    vptr = qkv.data_ptr() + 2 * dim_out * 2
    check(lib().msam2_window_attention_fwd(_p(qt), q_ts, D, hq, wq, ws_q, kptr, vptr, qkv.stride(0), D, H, W, ws, _p(kpad),
                                           _p(vpad), _p(o), o.stride(0), D, B, heads, D, scale if scale is not None else 1.0 / math.sqrt(D), _stream()))
    return o


def window_qkv_attention_supported(dim: int, dim_out: int, heads: int, ws: int, pool: bool, H: int, W: int) -> bool:
    """True when `window_qkv_attention` is built for a block of this form (per-slice quantities only, never the batch)."""
    return bool(lib().msam2_window_qkv_attention_supported(dim, dim_out, heads, ws, int(bool(pool)), H, W))


def window_qkv_attention(xn: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, B: int, H: int, W: int, heads: int, ws: int,
                         pool: bool = False, scale: Optional[float] = None) -> torch.Tensor:
    """`window_attention(gemm(xn, w, bias), ...)` (with 2x2 max-pooled queries when `pool`) as one kernel: the q | k | v map is never
    written.  xn 16-bit [B*H*W, dim], w 16-bit [3*heads*96, dim], bias fp32 -> o 16-bit [B*Hq*Wq, heads*96].  A form that is not built
    (`window_qkv_attention_supported`) is an error."""
    _req(xn.dim() == 2 and w.dim() == 2 and xn.shape[0] == B * H * W and xn.shape[1] == w.shape[1] and w.shape[0] == 3 * heads * 96,
         "window_qkv_attention shapes")
    _req(xn.dtype == OP16 and w.dtype == OP16 and xn.is_contiguous() and w.is_contiguous(), "window_qkv_attention operands: 16-bit, contiguous")
    _req(bias.dtype == F32 and bias.is_contiguous() and bias.numel() == w.shape[0], "window_qkv_attention: bias is fp32 [3*heads*96]")
    hq, wq = (H // 2, W // 2) if pool else (H, W)
    o = torch.empty(B * hq * wq, heads * 96, dtype=OP16, device=xn.device)
    check(lib().msam2_window_qkv_attention_fwd(_p(xn), _p(w), _p(bias), _p(o), B, H, W, xn.shape[1], heads, ws, int(bool(pool)),
                                               scale if scale is not None else 1.0 / math.sqrt(96), _stream()))
    return o


def attention_small(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Decoder attention with head dim 16/32: q [B,Lq,C], k/v [B,Lk,C] bf16 (C = heads*D contiguous) -> [B,Lq,C] bf16."""
    B, Lq, C = q.shape
    Lk = k.shape[1]
    D = C // heads
    for t in (q, k, v):
        _req(t.dtype == OP16 and t.stride(2) == 1, "attention_small tensors must be 16-bit (ops.OP16), channel-contiguous")
    o = out if out is not None else torch.empty(B, Lq, C, dtype=OP16, device=q.device)
    _req(o.dtype == OP16 and o.shape == (B, Lq, C) and o.stride(2) == 1, "attention_small: out is 16-bit [B,Lq,C] with contiguous channels")
    check(lib().msam2_attention_small_fwd(_p(q), q.stride(0), q.stride(1), _p(k), k.stride(0), k.stride(1), _p(v), v.stride(0),
                                          v.stride(1), _p(o), o.stride(0), o.stride(1), B, heads, Lq, Lk, D,
                                          1.0 / math.sqrt(D), _stream()))
    return o


def add_cast(a: torch.Tensor, b: Optional[torch.Tensor] = None, alpha: float = 1.0, out_dtype: torch.dtype = OP16,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = a + alpha*b over a logical [D0, D1, C] volume (C contiguous in a and b; outer dims may be strided or, for b,
    broadcast with stride 0).  Result is contiguous (or written into the contiguous `out`)."""
    _req(a.dim() == 3 and (a.stride(2) == 1 or a.shape[2] == 1), "add_cast: a must be [D0,D1,C] with contiguous C")
    D0, D1, C = a.shape
    bs0 = bs1 = 0
    if b is not None:
        b = b.expand(D0, D1, C)
        _req(b.stride(2) == 1 or C == 1, "add_cast: b must have contiguous C")
        bs0, bs1 = b.stride(0), b.stride(1)
    if out is None:
        out = torch.empty(D0, D1, C, dtype=out_dtype, device=a.device)
    _req(out.is_contiguous() and out.numel() == D0 * D1 * C, "add_cast: out must be a contiguous [D0,D1,C] buffer")
    check(lib().msam2_add_cast(_p(a), _is_bf16(a), a.stride(0), a.stride(1), _p(b), _is_bf16(b) if b is not None else 0, bs0,
                               bs1, alpha, _p(out), _is_bf16(out), D0, D1, C, _stream()))
    return out


class DeviceSeed:
    """Stream id of a dropout call whose low part lives on the device: effective seed = base + *dev (int64 [1] tensor, written by
    `counter_bump`).  A hipGraph replay of a training step then draws new masks, because the counter is advanced by a kernel of the
    step instead of being baked into the captured arguments."""
    __slots__ = ("base", "dev")

    def __init__(self, base: int, dev: torch.Tensor):
        assert dev.dtype == torch.int64 and dev.numel() == 1 and dev.is_cuda
        self.base, self.dev = int(base), dev


def counter_bump(counter: torch.Tensor, snapshot: Optional[torch.Tensor] = None) -> None:
    """counter[0] += 1 on the device (int64 [1]); snapshot[0] = the new value."""
    _req(counter.dtype == torch.int64 and counter.numel() == 1 and (snapshot is None or (snapshot.dtype == torch.int64 and snapshot.numel() == 1)),
         "counter_bump: int64 [1] tensors")
    check(lib().msam2_counter_bump(_p(counter), _p(snapshot), _stream()))


def dropout(x: torch.Tensor, p: float, seed, offset: int, residual: Optional[torch.Tensor] = None,
            out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = residual + (keep ? x / (1 - p) : 0) on a [rows, cols] map (row-major, rows may be strided); the mask is element
    (offset + r * cols + c) of the counter-based stream `seed` (an int, or a `DeviceSeed`), so calling it again on a gradient with the
    same (seed, offset) is the backward.  residual: fp32 [rows, cols]."""
    seed_dev = None
    if isinstance(seed, DeviceSeed):
        seed, seed_dev = seed.base, seed.dev
    _req(x.dim() == 2 and x.stride(1) == 1, "dropout: [rows, cols] row-major")
    rows, cols = x.shape
    y = out if out is not None else torch.empty(rows, cols, dtype=out_dtype or x.dtype, device=x.device)
    _req(y.shape == x.shape and y.stride(1) == 1, "dropout: out must be [rows, cols] row-major (rows may be strided)")
    if residual is not None:
        _req(residual.dtype == F32 and residual.shape == x.shape and residual.stride(1) == 1, "dropout: residual must be fp32 [rows, cols]")
    check(lib().msam2_dropout(_p(x), _is_bf16(x), x.stride(0), _p(residual), residual.stride(0) if residual is not None else 0, _p(y), _is_bf16(y),
                              y.stride(0), rows, cols, float(p), int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), _p(seed_dev), _stream()))
    return y


def add_cast_into(out: torch.Tensor, a: torch.Tensor, b: Optional[torch.Tensor] = None, alpha: float = 1.0) -> torch.Tensor:
    """Strided gather/copy(+add) of a [D0,D1,C] view into a contiguous slice of a larger buffer (memory-bank assembly)."""
    return add_cast(a, b, alpha, out=out)


def gate_no_obj_(x: torch.Tensor, score: torch.Tensor, value: float) -> torch.Tensor:
    """x[b] = value where score[b] <= 0 (fp32, contiguous, in place)."""
    _req(x.dtype == F32 and x.is_contiguous(), "gate_no_obj: fp32 contiguous")
    B = x.shape[0]
    check(lib().msam2_gate_rows(_p(x), _p(score), value, B, x.numel() // B, _stream()))
    return x


def any_positive(x: torch.Tensor) -> torch.Tensor:
    """[B, ...] fp32 -> [B, 1] fp32 (1.0 where any element of the row is > 0)."""
    _req(x.dtype == F32 and x.is_contiguous(), "any_positive: fp32 contiguous")
    B = x.shape[0]
    out = torch.empty(B, 1, dtype=F32, device=x.device)
    check(lib().msam2_any_positive(_p(x), _p(out), B, x.numel() // B, _stream()))
    return out


def maxpool2x2(x: torch.Tensor, B: int, H: int, W: int, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """x: [B*H*W, C] token-major view (row stride may exceed C) -> [B*(H/2)*(W/2), C]."""
    C = x.shape[1]
    _req(x.stride(1) == 1, "maxpool2x2: channel dim must be contiguous")
    y = torch.empty(B * (H // 2) * (W // 2), C, dtype=out_dtype or x.dtype, device=x.device)
    check(lib().msam2_maxpool2x2(_p(x), _is_bf16(x), x.stride(0), _p(y), _is_bf16(y), y.stride(0), B, H, W, C, _stream()))
    return y


def upsample2x_add_(y: torch.Tensor, top: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
    """y[B,H,W,C] += nearest2x(top[B,H/2,W/2,C]) in place (fp32, contiguous)."""
    _req(y.dtype == F32 and top.dtype == F32 and y.is_contiguous() and top.is_contiguous(), "upsample2x_add: fp32 contiguous")
    check(lib().msam2_upsample2x_add(_p(y), _p(top), B, H, W, y.shape[-1], _stream()))
    return y


def rope_table(side: int, D: int, theta: float, device) -> Tuple[torch.Tensor, torch.Tensor]:
    cs = torch.empty(side * side, D // 2, dtype=F32, device=device)
    sn = torch.empty_like(cs)
    check(lib().msam2_rope_table(_p(cs), _p(sn), side, D, theta, _stream()))
    return cs, sn


def rope_(x: torch.Tensor, n_rope: int, table: Tuple[torch.Tensor, torch.Tensor]) -> torch.Tensor:
    """Rotate rows l < n_rope of every batch of x [B, L, D] (bf16 view, D contiguous) in place."""
    B, L, D = x.shape
    _req(x.dtype == OP16 and x.stride(2) == 1, "rope: 16-bit with contiguous D")
    cs, sn = table
    check(lib().msam2_rope_inplace(_p(x), x.stride(0), x.stride(1), B, L, n_rope, cs.shape[0], D, _p(cs), _p(sn), _stream()))
    return x


def bilinear_upsample(x: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """fp32 [..., h, w] -> [..., H, W], align_corners=False."""
    _req(x.dtype == F32 and x.is_contiguous(), "bilinear: fp32 contiguous")
    h, w = x.shape[-2:]
    planes = x.numel() // (h * w)
    y = torch.empty(*x.shape[:-2], H, W, dtype=F32, device=x.device)
    check(lib().msam2_bilinear_upsample(_p(x), _p(y), planes, h, w, H, W, _stream()))
    return y


def sine_pos_2d(h: int, w: int, C: int, device, temperature: float = 10000.0) -> torch.Tensor:
    out = torch.empty(h * w, C, dtype=F32, device=device)
    check(lib().msam2_sine_pos_2d(_p(out), h, w, C, temperature, _stream()))
    return out


def fourier_pe_grid(gauss: torch.Tensor, h: int, w: int) -> torch.Tensor:
    C = 2 * gauss.shape[1]
    out = torch.empty(h * w, C, dtype=F32, device=gauss.device)
    check(lib().msam2_fourier_pe_grid(_p(out), _p(gauss.contiguous()), h, w, C, _stream()))
    return out


def hiera_pos_embed(pos_embed: torch.Tensor, pos_embed_window: torch.Tensor, h: int, w: int) -> torch.Tensor:
    _, C, bh, bw = pos_embed.shape
    out = torch.empty(h * w, C, dtype=F32, device=pos_embed.device)
    check(lib().msam2_hiera_pos_embed(_p(out), _p(pos_embed.contiguous()), _p(pos_embed_window.contiguous()), C, bh, bw, h, w,
                                      pos_embed_window.shape[-1], _stream()))
    return out


def im2col_patch(img: torch.Tensor) -> torch.Tensor:
    """img fp32 [B,3,S,S] -> bf16 [B*(S/4)^2, 160]."""
    _req(img.dtype == F32 and img.is_contiguous() and img.shape[1] == 3 and img.shape[2] == img.shape[3], "im2col_patch: [B,3,S,S] fp32")
    B, _, S, _ = img.shape
    out = torch.empty(B * (S // 4) ** 2, 160, dtype=OP16, device=img.device)
    check(lib().msam2_im2col_patch7x7s4(_p(img), _p(out), B, S, _stream()))
    return out


def patch_embed_supported(S: int, E: int) -> bool:
    """the one-kernel patch embedding (msam2_patch_embed7x7s4) takes this problem: whole 32-token wave blocks per token row, E <= 128"""
    So = S // 4
    return S % 4 == 0 and So % 32 == 0 and E <= 128


def patch_embed(img: torch.Tensor, w_perm: torch.Tensor, bias: torch.Tensor, pos: Optional[torch.Tensor] = None) -> torch.Tensor:
    """img fp32 [B,3,S,S] -> fp32 tokens [B*(S/4)^2, E] = conv7x7/s4/p3 + bias (+ pos [(S/4)^2, E], broadcast over the batch) in ONE kernel, no
    im2col map.  w_perm: 16-bit [ceil(E/32)*32, 176] in the kernel's reduction order, zero tap first (modeling.encoder.PatchEmbed._weight_perm)."""
    _req(img.dtype == F32 and img.is_contiguous() and img.shape[1] == 3 and img.shape[2] == img.shape[3], "patch_embed: [B,3,S,S] fp32")
    B, _, S, _ = img.shape
    E = bias.shape[0]
    _req(patch_embed_supported(S, E), "patch_embed: unsupported size (use im2col_patch + gemm)")
    _req(w_perm.dtype == OP16 and w_perm.is_contiguous() and tuple(w_perm.shape) == ((E + 31) // 32 * 32, 176), "patch_embed: w_perm [ceil32(E), 176] 16-bit")
    _req(bias.dtype == F32 and bias.is_contiguous(), "patch_embed: fp32 bias")
    if pos is not None:
        _req(pos.dtype == F32 and pos.is_contiguous() and tuple(pos.shape) == ((S // 4) ** 2, E), "patch_embed: pos fp32 [(S/4)^2, E]")
    out = torch.empty(B * (S // 4) ** 2, E, dtype=F32, device=img.device)
    check(lib().msam2_patch_embed7x7s4(_p(img), _p(w_perm), _p(bias), _p(pos), _p(out), B, S, E, _stream()))
    return out


def im2col3x3s2(x: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
    """bf16 NHWC -> [B*(H/2)*(W/2), ld] patches, columns (ky,kx,c), ld = 9*C rounded up to a multiple of 8 (zero filled)."""
    C = x.shape[-1]
    _req(x.dtype == OP16 and x.is_contiguous(), "im2col3x3s2: 16-bit contiguous NHWC")
    ld = (9 * C + 7) // 8 * 8
    out = torch.empty(B * (H // 2) * (W // 2), ld, dtype=OP16, device=x.device)
    check(lib().msam2_im2col3x3s2(_p(x), _p(out), B, H, W, C, ld, _stream()))
    return out


def conv3x3s2_ln_gelu(x: torch.Tensor, B: int, H: int, W: int, weight, bias, ln_w, ln_b, mask_mode: int = 0,
                      mask_scale: float = 0.0, mask_bias: float = 0.0) -> torch.Tensor:
    cout, cin = weight.shape[0], weight.shape[1]
    _req(x.dtype == (F32 if cin == 1 else OP16) and x.is_contiguous() and x.numel() == B * H * W * cin,
         "conv3x3s2_ln_gelu: contiguous NHWC [B*H*W, cin], fp32 for cin = 1, 16-bit otherwise")
    _req(all(t.dtype == F32 and t.is_contiguous() for t in (weight, bias, ln_w, ln_b)) and tuple(weight.shape[2:]) == (3, 3)
         and bias.numel() == cout and ln_w.numel() == cout and ln_b.numel() == cout, "conv3x3s2_ln_gelu: fp32 contiguous [cout, cin, 3, 3] weight, [cout] vectors")
    y = torch.empty(B * (H // 2) * (W // 2), cout, dtype=OP16, device=x.device)
    check(lib().msam2_conv3x3s2_ln_gelu(_p(x), _is_bf16(x), _p(weight), _p(bias), _p(ln_w), _p(ln_b), _p(y), B, H, W, cin, cout,
                                        mask_mode, mask_scale, mask_bias, _stream()))
    return y


def conv3x3s2_mfma_ln_gelu_supported(cin: int, cout: int) -> bool:
    """True when `conv3x3s2_mfma_ln_gelu` is built for these channel counts (4 -> 16, 16 -> 64, 64 -> 256)."""
    return bool(lib().msam2_conv3x3s2_mfma_ln_gelu_supported(cin, cout))


def conv3x3s2_mfma_ln_gelu(x: torch.Tensor, B: int, H: int, W: int, w_packed: torch.Tensor, bias: torch.Tensor, ln_w: torch.Tensor,
                           ln_b: torch.Tensor, eps: float, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """16-bit [B*(H/2)*(W/2), cout] = GELU(LayerNorm2d(conv3x3 s2 p1(x) + bias)) from one kernel: the bits of `im2col3x3s2` -> `gemm(out_dtype=F32)`
    -> `layernorm(act=ACT_GELU)`.  x 16-bit contiguous NHWC [B*H*W, cin]; w_packed 16-bit [cout, ld] with columns (ky, kx, c), zero filled
    up to ld >= ceil8(9 cin): the weight that `gemm` takes.  A form that is not built (`conv3x3s2_mfma_ln_gelu_supported`) is an error."""
    _req(x.dtype == OP16 and x.is_contiguous() and x.numel() % (B * H * W) == 0, "conv3x3s2_mfma_ln_gelu: 16-bit contiguous NHWC")
    cin = x.numel() // (B * H * W)
    _req(w_packed.dim() == 2 and w_packed.dtype == OP16 and w_packed.stride(1) == 1, "conv3x3s2_mfma_ln_gelu: w_packed must be 16-bit [cout, ld]")
    cout = w_packed.shape[0]
    _req(conv3x3s2_mfma_ln_gelu_supported(cin, cout), f"conv3x3s2_mfma_ln_gelu: {cin} -> {cout} channels is not built (4 -> 16, 16 -> 64, 64 -> 256)")
    _req(w_packed.shape[1] >= (9 * cin + 7) // 8 * 8, "conv3x3s2_mfma_ln_gelu: w_packed rows hold ceil8(9 cin) columns")
    _req(all(t.dtype == F32 and t.is_contiguous() and t.numel() == cout for t in (bias, ln_w, ln_b)), "conv3x3s2_mfma_ln_gelu: bias, ln_w, ln_b are fp32 [cout]")
    M = B * (H // 2) * (W // 2)
    if out is None:
        out = torch.empty(M, cout, dtype=OP16, device=x.device)
    _req(out.dtype == OP16 and out.shape == (M, cout) and out.stride(1) == 1, "conv3x3s2_mfma_ln_gelu: out must be 16-bit [M, cout], rows contiguous")
    check(lib().msam2_conv3x3s2_mfma_ln_gelu(_p(x), _p(w_packed), w_packed.stride(0), _p(bias), _p(ln_w), _p(ln_b), float(eps), _p(out),
                                             out.stride(0), B, H, W, cin, cout, _stream()))
    return out


def dwconv7x7_ln(x: torch.Tensor, B: int, H: int, W: int, w_tap_major, bias, ln_w, ln_b) -> torch.Tensor:
    _req(x.dtype == F32 and x.is_contiguous(), "dwconv7x7_ln: fp32 contiguous NHWC")
    C = x.shape[-1]
    y = torch.empty(B * H * W, C, dtype=OP16, device=x.device)
    check(lib().msam2_dwconv7x7_ln(_p(x), _p(w_tap_major), _p(bias), _p(ln_w), _p(ln_b), _p(y), B, H, W, C, _stream()))
    return y


def convt2x2_shuffle(g: torch.Tensor, bias, skip: torch.Tensor, ln_w, ln_b, B: int, h: int, w: int) -> torch.Tensor:
    """skip: the high-resolution features, 16-bit or (C = 32 / 64) fp32 as the FPN returns them -- no 16-bit copy pass in front"""
    C = g.shape[1] // 4
    _req(g.dtype == OP16 and skip.dtype in (OP16, F32) and g.is_contiguous() and skip.is_contiguous(), "convt2x2_shuffle: contiguous 16-bit g, 16-bit / fp32 skip")
    y = torch.empty(B * 4 * h * w, C, dtype=OP16, device=g.device)
    if skip.dtype == F32:
        _req(C in (32, 64), "convt2x2_shuffle: fp32 skip features need C = 32 / 64")
        check(lib().msam2_convt2x2_shuffle_f32skip(_p(g), _p(bias), _p(skip), _p(ln_w), _p(ln_b), _p(y), B, h, w, C, _stream()))
    else:
        check(lib().msam2_convt2x2_shuffle(_p(g), _p(bias), _p(skip), _p(ln_w), _p(ln_b), _p(y), B, h, w, C, _stream()))
    return y


def convt2x2_shuffle_shared(g: torch.Tensor, bias, skip: torch.Tensor, ln_w, ln_b, B: int, h: int, w: int) -> torch.Tensor:
    """convt2x2_shuffle with ONE skip map [4hw, C] (16-bit or fp32) read for all B batch elements (batch stride 0): N prompt sets on
    one image without N copies of the high-resolution features.  Bit-identical to convt2x2_shuffle on the repeated map."""
    C = g.shape[1] // 4
    _req(g.dtype == OP16 and skip.dtype in (OP16, F32) and g.is_contiguous() and skip.is_contiguous(), "convt2x2_shuffle_shared: contiguous 16-bit g, 16-bit / fp32 skip")
    _req(skip.numel() == 4 * h * w * C, "convt2x2_shuffle_shared: skip must be one [4hw, C] map")
    y = torch.empty(B * 4 * h * w, C, dtype=OP16, device=g.device)
    check(lib().msam2_convt2x2_shuffle_shared(_p(g), _p(bias), _p(skip), _is_bf16(skip), _p(ln_w), _p(ln_b), _p(y), B, h, w, C, 0, _stream()))
    return y


def hyper_masks(hyper: torch.Tensor, up: torch.Tensor, n: int, P: int) -> torch.Tensor:
    K, C = hyper.shape[1], hyper.shape[2]
    _req(hyper.dtype == F32 and hyper.shape[0] == n, "hyper_masks: hyper must be fp32 [n, K, C]")
    _req(up.dtype == OP16 and up.is_contiguous() and up.numel() == n * P * C, "hyper_masks: up must be 16-bit contiguous [n*P, C]")
    masks = torch.empty(n, K, P, dtype=F32, device=up.device)
    check(lib().msam2_hyper_masks(_p(hyper.contiguous()), _p(up), _p(masks), n, K, P, C, _stream()))
    return masks


def prompt_points(xy: torch.Tensor, labels: torch.Tensor, gauss, point_emb, not_a_point, image_size: float, n_pad: int = 0) -> torch.Tensor:
    """xy fp32 [n,P,2], labels int32 [n,P] -> fp32 [n,P + n_pad,C]; the last n_pad points of every set are the padding point ((0,0), label -1)."""
    n, P = labels.shape
    C = point_emb.shape[1]
    out = torch.empty(n, P + n_pad, C, dtype=F32, device=xy.device)
    check(lib().msam2_prompt_points_padded(_p(xy.contiguous()), _p(labels.contiguous()), _p(gauss), _p(point_emb), _p(not_a_point), _p(out),
                                           n, P, n_pad, C, float(image_size), _stream()))
    return out


def select_mask(masks: torch.Tensor, ious: torch.Tensor, obj: torch.Tensor, multimask: bool, dynamic: bool, delta: float,
                thresh: float):
    n, K, h, w = masks.shape
    low = torch.empty(n, 1, h, w, dtype=F32, device=masks.device)
    sel = torch.empty(n, dtype=torch.int32, device=masks.device)
    iou_sel = torch.empty(n, 1, dtype=F32, device=masks.device)
    check(lib().msam2_select_mask(_p(masks), _p(ious), _p(obj), _p(low), _p(sel), _p(iou_sel), n, h * w, int(multimask), int(dynamic),
                                  delta, thresh, _stream()))
    return low, sel, iou_sel


def gather_rows(x: torch.Tensor, sel: Optional[torch.Tensor], offset: int = 0) -> torch.Tensor:
    n, T, C = x.shape
    y = torch.empty(n, C, dtype=F32, device=x.device)
    check(lib().msam2_gather_rows(_p(x.contiguous()), _p(sel), _p(y), n, T, C, offset, _stream()))
    return y


def obj_ptr_mix_(ptr: torch.Tensor, obj: torch.Tensor, no_obj_ptr: torch.Tensor) -> torch.Tensor:
    _req(ptr.dim() == 2 and ptr.dtype == F32 and ptr.is_contiguous(), "obj_ptr_mix: ptr must be fp32 contiguous [n, C]")
    _req(obj.dtype == F32 and obj.is_contiguous() and obj.numel() == ptr.shape[0], "obj_ptr_mix: obj must be fp32 contiguous [n]")
    _req(no_obj_ptr.dtype == F32 and no_obj_ptr.is_contiguous() and no_obj_ptr.numel() == ptr.shape[1], "obj_ptr_mix: no_obj_ptr must be fp32 contiguous [C]")
    check(lib().msam2_obj_ptr_mix(_p(ptr), _p(obj), _p(no_obj_ptr), ptr.shape[0], ptr.shape[1], _stream()))
    return ptr


def connected_components(mask_u8: torch.Tensor):
    """Drop-in for ``sam2_train._C.get_connected_componnets`` (connected_components.cu:213-282)."""
    if not mask_u8.is_cuda:
        raise RuntimeError("inputs must be a CUDA tensor")
    if mask_u8.dim() != 4 or mask_u8.shape[1] != 1:
        raise RuntimeError("inputs must be [N, 1, H, W] shape")
    if mask_u8.dtype != torch.uint8:
        raise RuntimeError("inputs must be a uint8 type")
    N, _, H, W = mask_u8.shape
    if H % 2:
        raise RuntimeError("height must be a even number")
    if W % 2:
        raise RuntimeError("width must be a even number")
    m = mask_u8.contiguous()
    labels = torch.empty(N, 1, H, W, dtype=torch.int32, device=m.device)
    counts = torch.empty_like(labels)
    nb = lib().msam2_cc_workspace_bytes(N, H, W)
    ws = torch.empty(nb, dtype=torch.uint8, device=m.device)
    check(lib().msam2_cc_label(_p(m), _p(labels), _p(counts), N, H, W, _p(ws), nb, _stream()))
    return [labels, counts]


def fill_holes_(mask: torch.Tensor, max_area: int) -> torch.Tensor:
    """fill_holes_in_mask_scores (utils/misc.py:247-258), in place on an fp32 [N,1,H,W] tensor."""
    _req(mask.dtype == F32 and mask.is_contiguous(), "fill_holes: fp32 contiguous")
    N, _, H, W = mask.shape
    nb = lib().msam2_fill_holes_workspace_bytes(N, H, W)
    ws = torch.empty(nb, dtype=torch.uint8, device=mask.device)
    check(lib().msam2_fill_holes(_p(mask), N, H, W, max_area, _p(ws), nb, _stream()))
    return mask


# ---------------------------------------------------------------------------------------------------------------------
class HipGraph:
    """Capture everything enqueued on the current stream inside the ``with`` block; ``replay()`` relaunches it."""

    def __init__(self):
        self._exec = ctypes.c_void_p()
        self._stream = None

    def __enter__(self):
        self._stream = _stream()
        check(lib().msam2_graph_begin(self._stream))
        return self

    def __exit__(self, et, ev, tb):
        rc = lib().msam2_graph_end(self._stream, ctypes.byref(self._exec))
        if et is None:
            check(rc)
        return False

    def replay(self):
        check(lib().msam2_graph_launch(self._exec, _stream()))

    def __del__(self):
        try:
            if self._exec:
                lib().msam2_graph_destroy(self._exec)
        except Exception:
            pass


def space_to_depth(x: torch.Tensor, B: int, H: int, W: int, k: int) -> torch.Tensor:
    """NHWC [B*H*W, C] -> bf16 [B*(H/k)*(W/k), ld] patches with columns (ky,kx,c), ld = k*k*C rounded up to 8."""
    C = x.shape[-1]
    _req(x.dtype in (F32, OP16) and x.is_contiguous() and x.numel() == B * H * W * C, "space_to_depth: fp32 / 16-bit contiguous NHWC [B*H*W, C]")
    ld = (k * k * C + 7) // 8 * 8
    out = torch.empty(B * (H // k) * (W // k), ld, dtype=OP16, device=x.device)
    check(lib().msam2_space_to_depth(_p(x), _is_bf16(x), _p(out), B, H, W, C, k, ld, _stream()))
    return out


def aa_downsample(x: torch.Tensor, factor: int, in_scale: float = 1.0, in_bias: float = 0.0) -> torch.Tensor:
    """fp32 [..., H, W] -> [..., H/f, W/f] anti-aliased bilinear (of x*in_scale + in_bias)."""
    _req(x.dtype == F32 and x.is_contiguous(), "aa_downsample: fp32 contiguous")
    H, W = x.shape[-2:]
    y = torch.empty(*x.shape[:-2], H // factor, W // factor, dtype=F32, device=x.device)
    check(lib().msam2_aa_downsample(_p(x), _p(y), x.numel() // (H * W), H, W, factor, in_scale, in_bias, _stream()))
    return y


def fill_components_(mask: torch.Tensor, max_area: int, threshold: float, above: bool, fill_value: float) -> torch.Tensor:
    """In place on fp32 [N,1,H,W]: components of (mask > threshold) if `above` else (mask <= threshold) with area <= max_area
    are set to fill_value (SAM2Transforms.postprocess_masks, utils/transforms.py:74-98)."""
    _req(mask.dtype == F32 and mask.is_contiguous(), "fill_components: fp32 contiguous")
    N, _, H, W = mask.shape
    nb = lib().msam2_fill_holes_workspace_bytes(N, H, W)
    ws = torch.empty(nb, dtype=torch.uint8, device=mask.device)
    check(lib().msam2_fill_components(_p(mask), N, H, W, int(max_area), float(threshold), int(above), float(fill_value), _p(ws), nb, _stream()))
    return mask


def image_prep(img_u8_hwc: torch.Tensor, size: int, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)) -> torch.Tensor:
    """uint8 [H,W,3] on device -> fp32 [3,size,size], /255, bilinear resize, ImageNet normalisation."""
    _req(img_u8_hwc.dtype == torch.uint8 and img_u8_hwc.dim() == 3 and img_u8_hwc.shape[2] == 3 and img_u8_hwc.is_contiguous(),
         "image_prep: uint8 [H,W,3] contiguous")
    H, W, _ = img_u8_hwc.shape
    out = torch.empty(3, size, size, dtype=F32, device=img_u8_hwc.device)
    m = (ctypes.c_float * 3)(*mean)
    s = (ctypes.c_float * 3)(*std)
    check(lib().msam2_image_prep(_p(img_u8_hwc), _p(out), H, W, size, m, s, _stream()))
    return out


def non_overlap(masks: torch.Tensor) -> torch.Tensor:
    """[n,1,H,W] fp32 -> same shape: per pixel the arg-max object keeps its score, the others are clamped to <= -10."""
    m = masks.to(F32).contiguous()
    n = m.shape[0]
    out = torch.empty_like(m)
    check(lib().msam2_non_overlap(_p(m), _p(out), n, m.numel() // n, _stream()))
    return out


def token_mlp3(hs: torch.Tensor, tok: torch.Tensor, w1, b1, w2, b2, w3, b3, out_dim: torch.Tensor, sigmoid: torch.Tensor,
               packed=None):
    """G three-layer ReLU MLPs of width 256 on tokens tok[g] of hs fp32 [B, T, 256] -> fp32 [B, G, 256] (first out_dim[g] valid).
    packed = (out_offset, out_stride, total): int32 [G] device tables + the element count of the flat fp32 result, head g of batch element b
    at [out_offset[g] + b * out_stride[g] : + out_dim[g]] -- heads of different widths as contiguous tensors without slicing copies."""
    B, T, C = hs.shape
    G = tok.shape[0]
    _req(hs.dtype == F32 and hs.stride(2) == 1 and C == 256, "token_mlp3: hs must be fp32 [B,T,256] with contiguous channels")
    _req(w1.dtype == OP16 and w1.shape == (G, C, C) and w1.is_contiguous() and w2.shape == (G, C, C) and w3.shape == (G, C, C), "token_mlp3 weights")
    if packed is not None:
        off, ld, total = packed
        _req(off.dtype == torch.int32 and ld.dtype == torch.int32 and off.numel() == G and ld.numel() == G, "token_mlp3: packed tables are int32 [G]")
        out = torch.empty(total, dtype=F32, device=hs.device)
        check(lib().msam2_token_mlp3_packed(_p(hs), hs.stride(0), hs.stride(1), _p(tok), _p(w1), _p(b1), _p(w2), _p(b2), _p(w3), _p(b3),
                                            _p(out_dim), _p(sigmoid), _p(out), _p(off), _p(ld), G, B, C, _stream()))
        return out
    out = torch.empty(B, G, C, dtype=F32, device=hs.device)
    check(lib().msam2_token_mlp3(_p(hs), hs.stride(0), hs.stride(1), _p(tok), _p(w1), _p(b1), _p(w2), _p(b2), _p(w3), _p(b3),
                                 _p(out_dim), _p(sigmoid), _p(out), G, B, C, _stream()))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# automatic mask generation: post-processing on low-res logits (csrc/amg.hip)
def _f32(x: float) -> float:
    """A Python threshold as torch compares an fp32 tensor with it (rounded to fp32)."""
    return float(torch.tensor(x, dtype=F32))


def mask_stats(logits: torch.Tensor, h: int, w: int, thr: float, offset: float):
    """fp32 [M, lh, lw] low-res logits -> (counts int32 [M, 3], boxes int32 [M, 4]) of their (h, w) bilinear up-sampling:
    counts = (#v > thr + offset, #v > thr - offset, #v > thr), boxes = inclusive xyxy of v > thr ([0,0,0,0] if empty)."""
    _req(logits.dtype == F32 and logits.is_contiguous() and logits.dim() == 3, "mask_stats: fp32 contiguous [M, lh, lw]")
    M, lh, lw = logits.shape
    counts = torch.empty(M, 3, dtype=torch.int32, device=logits.device)
    boxes = torch.empty(M, 4, dtype=torch.int32, device=logits.device)
    nb = lib().msam2_mask_stats_workspace_bytes(M)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=logits.device)
    check(lib().msam2_mask_stats(_p(logits), M, lh, lw, int(h), int(w), _f32(thr), _f32(thr + offset), _f32(thr - offset), _p(counts), _p(boxes),
                                 _p(ws), nb, _stream()))
    return counts, boxes


def mask_rle(logits: torch.Tensor, h: int, w: int, crop_xy: Tuple[int, int], orig_hw: Tuple[int, int], thr: float):
    """Uncompressed RLEs ({"size": [H, W], "counts": [...]}, utils/amg.py format) of (bilinear (h, w) up-sampling of fp32 [M, lh, lw] > thr)
    pasted at crop_xy = (x0, y0) into an orig_hw = (H, W) frame of zeros.  One small copy (run counts) and one copy of all counts to the host."""
    _req(logits.dtype == F32 and logits.is_contiguous() and logits.dim() == 3, "mask_rle: fp32 contiguous [M, lh, lw]")
    M, lh, lw = logits.shape
    H, W = int(orig_hw[0]), int(orig_hw[1])
    x0, y0 = int(crop_xy[0]), int(crop_xy[1])
    t = _f32(thr)
    if M == 0:
        return []
    runs = torch.empty(M, dtype=torch.int32, device=logits.device)
    check(lib().msam2_mask_rle_runs(_p(logits), M, lh, lw, int(h), int(w), x0, y0, H, W, t, _p(runs), _stream()))
    off = torch.zeros(M + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(runs.cpu().to(torch.int64), 0)
    total = int(off[-1])
    counts = torch.empty(total, dtype=torch.int32, device=logits.device)
    off_d = off.to(logits.device)
    check(lib().msam2_mask_rle(_p(logits), M, lh, lw, int(h), int(w), x0, y0, H, W, t, _p(off_d), _p(counts), _stream()))
    flat = counts.cpu().tolist()
    o = off.tolist()
    return [{"size": [H, W], "counts": flat[o[i]:o[i + 1]]} for i in range(M)]


def _f32_below(x: float) -> float:
    """The largest fp32 t <= x: for every fp32 v, v > t exactly when v > x in double precision (torchvision compares its fp32 IoU with
    the double threshold)."""
    t = torch.tensor(x, dtype=F32)
    if float(t) > x:
        t = torch.nextafter(t, torch.tensor(-math.inf, dtype=F32))
    return float(t)


def box_nms(boxes: torch.Tensor, scores: torch.Tensor, iou_threshold: float) -> torch.Tensor:
    """torchvision.ops.nms semantics (stable descending score order, IoU > threshold suppresses): int64 indices of the kept boxes,
    in rank order."""
    _req(boxes.dim() == 2 and boxes.shape[1] == 4 and scores.dim() == 1 and scores.shape[0] == boxes.shape[0], "box_nms: boxes [K, 4], scores [K]")
    K = boxes.shape[0]
    dev = boxes.device
    if K == 0:
        return torch.empty(0, dtype=torch.int64, device=dev)
    b = boxes.to(F32).contiguous()
    s = scores.to(F32).contiguous()
    keep = torch.empty(K, dtype=torch.int64, device=dev)
    n_keep = torch.empty(1, dtype=torch.int32, device=dev)
    nb = lib().msam2_box_nms_workspace_bytes(K)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    check(lib().msam2_box_nms(_p(b), _p(s), K, _f32_below(iou_threshold), _p(keep), _p(n_keep), _p(ws), nb, _stream()))
    return keep[: int(n_keep.item())]


# ---------------------------------------------------------------------------------------------------------------------
# The label-volume entries (csrc/volume_labels.hip, prompts.hip, volume_prep.hip, components.hip, surface.hip).  Their limits, checked here
# so that the message names the caller's tensor; each mirrors a constant of the library, which checks again:
LABEL_MAX_OBJECTS = 32            # csrc/common.h LABEL_MAX_OBJ: objects (ids) per call
LABEL_MAX_SLICES = 65535          # csrc/common.h LABEL_MAX_SLICES: D of a volume, T of a stack
LABEL_MAX_SIDE = 8192             # csrc/common.h LABEL_MAX_SIDE: rows and columns
LABEL_MAX_VOXELS = 2 ** 31 - 2    # csrc/common.h LABEL_MAX_VOXELS: D * H * W of the entries that index voxels with an int32
LABEL_MAX_THRESHOLDS = 8          # csrc/volume_labels.hip LBL_MAX_THR: thresholds per label_slices call


def _label_values(what: str, ids, at_least: int):
    """host integers or a tensor -> a list of label values, each 1 .. 255"""
    vals = [int(v) for v in (ids.tolist() if isinstance(ids, torch.Tensor) else ids)]
    _req(len(vals) >= at_least and all(1 <= v <= 255 for v in vals), f"{what} must be integers in 1 .. 255 (0 is the background)")
    return vals


def _device_table(what: str, t, dtype, shape, dev, whose: str, dtype_text: Optional[str] = None) -> None:
    """t must be a contiguous tensor of `dtype` (one, or a tuple of accepted ones: the first is named) and `shape` on `dev`, the device of
    the tensor `whose` names ("labels'", "source's")"""
    dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
    _req(isinstance(t, torch.Tensor) and t.dtype in dtypes and t.is_contiguous() and tuple(t.shape) == tuple(shape) and t.device == dev,
         f"{what} must be {dtype_text or str(dtypes[0]).split('.')[-1]} contiguous {list(shape)} on the {whose} device")


def _workspace8(nbytes: int, dev) -> torch.Tensor:
    """at least nbytes bytes, 8-byte aligned"""
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)


# ---------------------------------------------------------------------------------------------------------------------
# end of the 3-D path: label volumes and per-organ counts from low-res logits (csrc/volume_labels.hip)
def label_ids(ids, device) -> torch.Tensor:
    """Label values of the objects as the uint8 [n] device tensor label_slices takes: checked on the host (integers 1 .. 255, distinct)."""
    vals = _label_values("label_slices: ids", ids, 1)
    _req(len(set(vals)) == len(vals), "label_slices: ids must be distinct")
    return torch.tensor(vals, dtype=torch.uint8).to(device)


def label_slices(logits: torch.Tensor, ids, H: int, W: int, label_thr: float = 0.0, gt: Optional[torch.Tensor] = None, thresholds=None,
                 exclusive: bool = False, labels=True):
    """fp32 [T, n, lh, lw] low-res logits -> (labels uint8 [T, H, W] | None, counts int32 [K, T, n, 3] | None) of their (H, W) bilinear
    resize, which is never written: labels = ids[o] of the highest-scoring object above label_thr per voxel (ties to the lower index,
    0 = background); counts = (|P & G|, |P|, |G|) per threshold, slice and object, P = v_o > threshold (exclusive: and o is the voxel's
    label), G = gt == ids[o] (gt uint8 [T, H, W]; without it only |P| is filled).  counts are returned iff thresholds are given
    (at most 8 per call, rounded to fp32 as metrics.seg_counts passes them); labels=False skips the label volume, a uint8 contiguous
    [T, H, W] tensor is filled in place.
    ids: host integers (checked: distinct, 1 .. 255), or the device tensor of label_ids() taken as is.  Nothing is copied to the host."""
    _req(logits.dtype == F32 and logits.is_contiguous() and logits.dim() == 4, "label_slices: fp32 contiguous [T, n, lh, lw]")
    T, n, lh, lw = logits.shape
    dev = logits.device
    on_dev = isinstance(ids, torch.Tensor) and ids.device == dev and dev.type != "cpu"
    ids_d = ids.contiguous() if on_dev else label_ids(ids, dev)
    _req(ids_d.dtype == torch.uint8 and ids_d.numel() == n, f"label_slices: {n} objects need {n} uint8 ids")
    H, W = int(H), int(W)
    thr_d = counts = out = None
    K = 0
    if thresholds is not None:
        thr_d = thresholds if isinstance(thresholds, torch.Tensor) else torch.tensor([float(t) for t in thresholds], dtype=F32)
        thr_d = thr_d.to(device=dev, dtype=F32).contiguous()
        K = thr_d.numel()
        counts = torch.empty(K, T, n, 3, dtype=torch.int32, device=dev)
    if gt is not None:
        _device_table("label_slices: gt", gt, torch.uint8, (T, H, W), dev, "logits'")
    if isinstance(labels, torch.Tensor):
        _device_table("label_slices: labels", labels, torch.uint8, (T, H, W), dev, "logits'")
        out = labels
    elif labels:
        out = torch.empty(T, H, W, dtype=torch.uint8, device=dev)
    check(lib().msam2_label_slices(_p(logits), _p(ids_d), T, n, lh, lw, H, W, _f32(label_thr), _p(thr_d), K, _p(gt), int(bool(exclusive)),
                                   _p(out), _p(counts), _stream()))
    return out, counts


CONFIDENCE_OUTPUTS = ("labels", "core", "envelope", "conf")


def label_confidence(logits: torch.Tensor, ids, H: int, W: int, margins, select: int = 0, label_thr: float = 0.0, labels=True, core=True,
                     envelope=True, conf=True, counts=True):
    """fp32 [T, n, lh, lw] low-res logits -> (labels, core, envelope, conf: uint8 [T, H, W] | None each, counts int32 [T, n, 2 + 2K] | None) of
    their (H, W) bilinear resize, which is never written -- label_slices' pass, keeping the second-best value as well.  Per voxel tv = the top
    value with its object `to`, sv = the second (ties to the lower index, the tied value is sv).  Labelled (tv > label_thr): margin
    m = tv - max(label_thr, sv); background with a finite tv: nearest object `to`, m = label_thr - tv.  margins: K host floats (1 .. 8,
    finite, > 0, strictly ascending, rounded to fp32), in logit units.
    labels = label_slices' bytes; core = ids[to] where labelled and m >= margins[select], else 0; envelope = the label, and on background
    ids[to] where m < margins[select]; conf = #{k: m >= margins[k]} (K where no object is nearest: 0 = least certain).  counts columns:
    0 voxels labelled o, 1 voxels with v_o > label_thr that another object took, 2 .. 2 + K labelled o with m < margins[k],
    2 + K .. 2 + 2K background nearest o with m < margins[k].
    Every output: True = allocated here, False = skipped, or (volumes) a uint8 contiguous [T, H, W] tensor / (counts) an int32 contiguous
    [T, n, 2 + 2K] tensor filled in place.  ids: as label_slices takes them.  Nothing is copied to the host."""
    _req(logits.dtype == F32 and logits.is_contiguous() and logits.dim() == 4, "label_confidence: fp32 contiguous [T, n, lh, lw]")
    T, n, lh, lw = logits.shape
    dev = logits.device
    on_dev = isinstance(ids, torch.Tensor) and ids.device == dev and dev.type != "cpu"
    ids_d = ids.contiguous() if on_dev else label_ids(ids, dev)
    _req(ids_d.dtype == torch.uint8 and ids_d.numel() == n, f"label_confidence: {n} objects need {n} uint8 ids")
    H, W = int(H), int(W)
    _req(not isinstance(margins, torch.Tensor) or margins.device.type == "cpu", "label_confidence: margins are host numbers (the call reads them)")
    m = [float(v) for v in (margins.tolist() if isinstance(margins, torch.Tensor) else margins)]
    K = len(m)
    m_host = (ctypes.c_float * max(K, 1))(*m)
    vols = []
    for name, want in zip(CONFIDENCE_OUTPUTS, (labels, core, envelope, conf)):
        if isinstance(want, torch.Tensor):
            _device_table(f"label_confidence: {name}", want, torch.uint8, (T, H, W), dev, "logits'")
            vols.append(want)
        else:
            vols.append(torch.empty(T, H, W, dtype=torch.uint8, device=dev) if want else None)
    if isinstance(counts, torch.Tensor):
        _device_table("label_confidence: counts", counts, torch.int32, (T, n, 2 + 2 * K), dev, "logits'")
        cnt = counts
    else:
        cnt = torch.empty(T, n, 2 + 2 * K, dtype=torch.int32, device=dev) if counts else None
    check(lib().msam2_label_confidence(_p(logits), _p(ids_d), T, n, lh, lw, H, W, _f32(label_thr), m_host, K, int(select), _p(vols[0]), _p(vols[1]),
                                       _p(vols[2]), _p(vols[3]), _p(cnt), _stream()))
    return vols[0], vols[1], vols[2], vols[3], cnt


# ---------------------------------------------------------------------------------------------------------------------
# start of the 3-D path: box and click prompts from a label volume (csrc/prompts.hip)
def _label_volume_args(what: str, labels: torch.Tensor, ids, min_side: int = 1, max_voxels: bool = False):
    """the checks the entries on label volumes share -> (ids on the device, D, H, W, n).  Every entry states its own contract: min_side = 2
    where a voxel needs an in-plane neighbour (csrc/surface.hip), max_voxels where the library indexes voxels with an int32 (components.hip,
    surface.hip; label_stats and label_pick use 64-bit offsets and have no cap)"""
    _req(isinstance(labels, torch.Tensor) and labels.dtype == torch.uint8 and labels.dim() == 3 and labels.is_contiguous(),
         f"{what}: labels must be a uint8 contiguous [D, H, W] label volume")
    D, H, W = labels.shape
    _req(1 <= D <= LABEL_MAX_SLICES and 1 <= H <= LABEL_MAX_SIDE and 1 <= W <= LABEL_MAX_SIDE,
         f"{what}: sizes {D} x {H} x {W} (1 .. {LABEL_MAX_SLICES} slices of 1 .. {LABEL_MAX_SIDE} rows and columns)")
    dev = labels.device
    ids_d, n = None, 0
    if ids is not None:                                    # (label_components takes no ids)
        on_dev = isinstance(ids, torch.Tensor) and ids.device == dev and dev.type != "cpu"
        ids_d = ids.contiguous() if on_dev else label_ids(ids, dev)
        n = ids_d.numel()
        _req(ids_d.dtype == torch.uint8 and ids_d.dim() == 1 and 1 <= n <= LABEL_MAX_OBJECTS,
             f"{what}: ids must be 1 .. {LABEL_MAX_OBJECTS} uint8 label values, got {n}")
    _req(labels.is_cuda, f"{what}: the label volume must be on the GPU")
    _req(H >= min_side and W >= min_side, f"{what}: H x W = {H} x {W} (at least {min_side} rows and columns)")
    _req(not max_voxels or D * H * W <= LABEL_MAX_VOXELS, f"{what}: {D * H * W} voxels (at most 2^31 - 2)")
    return ids_d, D, H, W, n


def label_stats(labels: torch.Tensor, ids, rows: Optional[torch.Tensor] = None):
    """uint8 [D, H, W] label volume -> (stats int32 [D, n, 5], rows int32 [D, n, H]): stats = (count, r0, r1, c0, c1), the number of
    voxels equal to ids[j] in slice d and their inclusive row / column extent ((0, -1, -1, -1, -1) where the object is absent); rows =
    the count per row, the workspace label_pick reads (pass one of that shape to reuse it).  Voxels that are 0 or not in ids are ignored.
    ids: host integers (checked: distinct, 1 .. 255), or the device tensor of label_ids() taken as is.  Nothing is copied to the host."""
    ids_d, D, H, W, n = _label_volume_args("label_stats", labels, ids)
    dev = labels.device
    if rows is None:
        rows = torch.empty(D, n, H, dtype=torch.int32, device=dev)
    _device_table("label_stats: rows", rows, torch.int32, (D, n, H), dev, "labels'")
    stats = torch.empty(D, n, 5, dtype=torch.int32, device=dev)
    check(lib().msam2_label_stats(_p(labels), _p(ids_d), D, H, W, n, _p(stats), _p(rows), _stream()))
    return stats, rows


def label_pick(labels: torch.Tensor, ids, stats: torch.Tensor, rows: torch.Tensor, k: Optional[torch.Tensor] = None,
               u: Optional[torch.Tensor] = None) -> torch.Tensor:
    """xy int32 [D, n, 2] = (column, row) of the k-th voxel of object j in slice d in raster order (np.argwhere's), from the volume and
    label_stats' two tables.  k int32 [D, n]: explicit indices; or u uint32 [D, n] (int32 is taken as the same 32 bits): uniform random
    words, k = (u * count) >> 32.  (-1, -1) where the object is absent; k outside [0, count) is clamped to count - 1."""
    ids_d, D, H, W, n = _label_volume_args("label_pick", labels, ids)
    dev = labels.device
    _req((k is None) != (u is None), "label_pick: exactly one of k and u")
    _device_table("label_pick: stats", stats, torch.int32, (D, n, 5), dev, "labels'")
    _device_table("label_pick: rows", rows, torch.int32, (D, n, H), dev, "labels'")
    if u is None:
        _device_table("label_pick: k", k, torch.int32, (D, n), dev, "labels'")
    else:
        _device_table("label_pick: u", u, (torch.uint32, torch.int32), (D, n), dev, "labels'")
    xy = torch.empty(D, n, 2, dtype=torch.int32, device=dev)
    check(lib().msam2_label_pick(_p(labels), _p(ids_d), _p(stats), _p(rows), _p(k), _p(u), D, H, W, n, _p(xy), _stream()))
    return xy


# ---------------------------------------------------------------------------------------------------------------------
# closing the loop: corrective clicks from the error regions of a prediction against the ground truth (csrc/clicks.hip)
CLICK_MODES = {"center": 0, "uniform": 1}


def label_error_clicks_workspace_bytes(D: int, H: int, W: int, n: int, mode: str = "center") -> int:
    _req(mode in CLICK_MODES, f"label_error_clicks: mode {mode!r} (one of {tuple(CLICK_MODES)})")
    return int(lib().msam2_label_error_clicks_workspace_bytes(D, H, W, n, CLICK_MODES[mode]))


def label_error_clicks(pred: torch.Tensor, gt: torch.Tensor, ids, mode: str = "center", k: Optional[torch.Tensor] = None,
                       u: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Two uint8 [D, H, W] label volumes -> clicks int32 [D, n, 8] = (x, y, label, |FN|, |FP|, max d2(FN), max d2(FP), 0) per slice and object:
    FN = {gt == ids[j] and pred != ids[j]}, FP = {pred == ids[j] and gt != ids[j]}, d2 = the squared distance to the nearest pixel outside the
    region, the one-pixel frame around the image included.  mode="center": the voxel of largest d2 (ties to the smallest y * W + x) of the
    region with the larger maximum, label 1 for FN (strictly larger), 0 for FP.  mode="uniform": the k-th voxel of FN | FP in raster order,
    k int32 [D, n] or u uint32 [D, n] (int32 is taken as the same 32 bits; k = (u * count) >> 32), label 1 iff it is in FN; the d2 fields are
    -1.  No error voxel: (-1, -1, -1, 0, 0, ...).  workspace: a contiguous 8-byte-aligned device tensor of at least
    `label_error_clicks_workspace_bytes` bytes to reuse; out: the table to fill.  Nothing is copied to the host."""
    ids_d, D, H, W, n = _label_volume_args("label_error_clicks", pred, ids, max_voxels=True)
    dev = pred.device
    _device_table("label_error_clicks: gt", gt, torch.uint8, pred.shape, dev, "labels'")
    _req(mode in CLICK_MODES, f"label_error_clicks: mode {mode!r} (one of {tuple(CLICK_MODES)})")
    if mode == "center":
        _req(k is None and u is None, "label_error_clicks: k and u belong to mode='uniform'")
    else:
        _req((k is None) != (u is None), "label_error_clicks: mode='uniform' needs exactly one of k and u")
        if u is None:
            _device_table("label_error_clicks: k", k, torch.int32, (D, n), dev, "labels'")
        else:
            _device_table("label_error_clicks: u", u, (torch.uint32, torch.int32), (D, n), dev, "labels'")
    nb = lib().msam2_label_error_clicks_workspace_bytes(D, H, W, n, CLICK_MODES[mode])
    if workspace is None:
        workspace = _workspace8(nb, dev)
    _req(isinstance(workspace, torch.Tensor) and workspace.is_contiguous() and workspace.device == dev
         and workspace.numel() * workspace.element_size() >= nb and workspace.data_ptr() % 8 == 0,
         f"label_error_clicks: workspace must be a contiguous 8-byte-aligned tensor of at least {nb} bytes on the labels' device")
    if out is None:
        out = torch.empty(D, n, 8, dtype=torch.int32, device=dev)
    _device_table("label_error_clicks: out", out, torch.int32, (D, n, 8), dev, "labels'")
    check(lib().msam2_label_error_clicks(_p(pred), _p(gt), _p(ids_d), _p(k), _p(u), D, H, W, n, CLICK_MODES[mode], _p(out), _p(workspace),
                                         workspace.numel() * workspace.element_size(), _stream()))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# in front of both: volume intake -- window, Pillow-exact resize, normalise; nearest resize of label maps (csrc/volume_prep.hip)
PREP_SOURCE_TYPES = {torch.uint8: 0, torch.int16: 1, torch.float32: 2}
LABEL_SOURCE_TYPES = {torch.uint8: 0, torch.int16: 1, torch.int32: 2, torch.int64: 3}


def _prep_sizes(what: str, T: int, H0: int, W0: int, S: int) -> None:
    _req(1 <= T <= LABEL_MAX_SLICES and 1 <= H0 <= LABEL_MAX_SIDE and 1 <= W0 <= LABEL_MAX_SIDE and 1 <= S <= LABEL_MAX_SIDE,
         f"{what}: sizes {T} x {H0} x {W0} -> {S} (1 .. {LABEL_MAX_SLICES} slices, sides 1 .. {LABEL_MAX_SIDE})")


def volume_prep_workspace_bytes(T: int, H0: int, W0: int, size: int) -> int:
    """bytes of the uint8 workspace volume_prep needs for T slices of H0 x W0 -> size: 0 when the call takes the fused form"""
    return int(lib().msam2_volume_prep_workspace_bytes(int(T), int(H0), int(W0), int(size)))


def volume_prep(src: torch.Tensor, size: int, tables_x, tables_y, windows=None, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225),
                out=True, grey=False, workspace: Optional[torch.Tensor] = None):
    """Raw slice stack [T, Cin, H0, W0] (Cin 1 or 3; uint8, int16 or float32, contiguous, on the GPU) -> (out fp32 [T, 3, size, size] | None,
    grey uint8 [T, 3, size, size] | None): channel c = plane c % Cin through window c (windows: three (lo, hi) pairs, needed for int16 /
    float32), Pillow's 8-bit bicubic resize byte for byte, then ((float)g / 255 - mean) / std in fp32.  tables_x / tables_y: (coefficients
    int32 [size, ksize], bounds int32 [size, 2]) device tensors of volume_prep.resample_tables for W0 -> size / H0 -> size, None when that
    dimension is already `size`.  out / grey: True allocates, a tensor is filled in place, False skips it.  workspace: uint8 tensor of
    volume_prep_workspace_bytes (allocated when needed and not given).  No host sync."""
    _req(isinstance(src, torch.Tensor) and src.dtype in PREP_SOURCE_TYPES and src.dim() == 4 and src.is_contiguous() and src.is_cuda,
         "volume_prep: src must be a uint8 / int16 / float32 contiguous [T, Cin, H0, W0] tensor on the GPU")
    T, Cin, H0, W0 = src.shape
    S, dev = int(size), src.device
    _req(Cin in (1, 3), f"volume_prep: Cin = {Cin} (1 or 3)")
    _prep_sizes("volume_prep", T, H0, W0, S)
    tabs = []
    for what, n, tab in (("tables_x", W0, tables_x), ("tables_y", H0, tables_y)):
        if n == S:
            _req(tab is None, f"volume_prep: {what} must be None, that pass is skipped ({n} -> {S})")
            tabs += [None, None, 0]
            continue
        _req(tab is not None and len(tab) == 2 and isinstance(tab[0], torch.Tensor) and tab[0].dim() == 2, f"volume_prep: {what} = (coefficients, bounds)")
        ks = tab[0].shape[1]
        _device_table(f"volume_prep: {what}[0]", tab[0], torch.int32, (S, ks), dev, "source's")
        _device_table(f"volume_prep: {what}[1]", tab[1], torch.int32, (S, 2), dev, "source's")
        tabs += [tab[0], tab[1], ks]
    win = None
    if src.dtype != torch.uint8:
        _req(windows is not None and len(windows) == 3 and all(len(w) == 2 for w in windows), "volume_prep: int16 / float32 sources need three (lo, hi) windows")
        win = (ctypes.c_double * 6)(*[float(v) for w in windows for v in w])
    res = []
    for what, t, dt in (("out", out, F32), ("grey", grey, torch.uint8)):
        if isinstance(t, torch.Tensor):
            _device_table(f"volume_prep: {what}", t, dt, (T, 3, S, S), dev, "source's", str(dt))
            res.append(t)
        else:
            res.append(torch.empty(T, 3, S, S, dtype=dt, device=dev) if t else None)
    _req(res[0] is not None or res[1] is not None, "volume_prep: at least one of out and grey")
    nb = volume_prep_workspace_bytes(T, H0, W0, S)
    if nb and workspace is None:
        workspace = torch.empty(nb, dtype=torch.uint8, device=dev)
    if workspace is not None:
        _req(workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.device == dev, "volume_prep: workspace must be a uint8 tensor on the source's device")
    m, s = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    check(lib().msam2_volume_prep(_p(src), PREP_SOURCE_TYPES[src.dtype], T, Cin, H0, W0, S, win, _p(tabs[0]), _p(tabs[1]), tabs[2], _p(tabs[3]),
                                  _p(tabs[4]), tabs[5], m, s, _p(res[1]), _p(res[0]), _p(workspace),
                                  0 if workspace is None else workspace.numel(), _stream()))
    return res[0], res[1]


def label_resize(src: torch.Tensor, size: int, ymap: torch.Tensor, xmap: torch.Tensor, obj_ids=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Label map [T, H0, W0] (uint8 / int16 / int32 / int64, contiguous, on the GPU) -> uint8 [T, size, size] label volume: a nearest
    gather through ymap / xmap (int32 [size] device tensors of volume_prep.nearest_map); a value is kept if it is 1 .. 255 and, with
    obj_ids given (host integers 1 .. 255), one of them; every other voxel is 0."""
    _req(isinstance(src, torch.Tensor) and src.dtype in LABEL_SOURCE_TYPES and src.dim() == 3 and src.is_contiguous() and src.is_cuda,
         "label_resize: src must be a uint8 / int16 / int32 / int64 contiguous [T, H0, W0] tensor on the GPU")
    T, H0, W0 = src.shape
    S, dev = int(size), src.device
    _prep_sizes("label_resize", T, H0, W0, S)
    _device_table("label_resize: ymap", ymap, torch.int32, (S,), dev, "source's")
    _device_table("label_resize: xmap", xmap, torch.int32, (S,), dev, "source's")
    keep = None
    if obj_ids is not None:
        keep = (ctypes.c_uint32 * 8)()
        for v in _label_values("label_resize: obj_ids", obj_ids, 0):      # (may repeat, may be empty: nothing is kept)
            keep[v >> 5] |= 1 << (v & 31)
    if out is None:
        out = torch.empty(T, S, S, dtype=torch.uint8, device=dev)
    _device_table("label_resize: out", out, torch.uint8, (T, S, S), dev, "source's")
    check(lib().msam2_label_resize(_p(src), LABEL_SOURCE_TYPES[src.dtype], T, H0, W0, S, _p(ymap), _p(xmap), keep, _p(out), _stream()))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# between the two: connected components, island removal and overlap counts of label volumes (csrc/components.hip)
LABEL_CONNECTIVITIES = (4, 8, 6, 18, 26)


def label_components(labels: torch.Tensor, connectivity: int = 26):
    """uint8 [D, H, W] label volume -> (comp, size), both int32 [D, H, W].  Two voxels are adjacent iff they carry the same non-zero value
    and differ by one offset of the neighbourhood: connectivity 6 / 18 / 26 in 3-D, 4 / 8 in plane (every slice on its own).  comp = 0 on
    the background, else 1 + the smallest linear index of the voxel's component; size = the component's voxel count at that smallest voxel,
    0 elsewhere.  All 255 values are handled at once.  Nothing is copied to the host."""
    _req(int(connectivity) in LABEL_CONNECTIVITIES, f"label_components: connectivity {connectivity} (one of {LABEL_CONNECTIVITIES})")
    _, D, H, W, _ = _label_volume_args("label_components", labels, None, max_voxels=True)
    dev = labels.device
    comp = torch.empty(D, H, W, dtype=torch.int32, device=dev)
    size = torch.empty_like(comp)
    nb = lib().msam2_label_components_workspace_bytes(D, H, W)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    check(lib().msam2_label_components(_p(labels), D, H, W, int(connectivity), _p(comp), _p(size), _p(ws), nb, _stream()))
    return comp, size


def label_largest_mask(keep_largest, n: int) -> int:
    """keep_largest (one bool, or one per object) as the bit mask msam2_label_clean takes"""
    if isinstance(keep_largest, (bool, int)):
        return (2 ** n - 1) if keep_largest else 0
    flags = [bool(f) for f in keep_largest]
    _req(len(flags) == n, f"label_clean: keep_largest names {len(flags)} objects, ids {n}")
    return sum(1 << j for j, f in enumerate(flags) if f)


def label_clean(labels: torch.Tensor, comp: torch.Tensor, size: torch.Tensor, ids, min_voxels=None, keep_largest=True,
                out: Optional[torch.Tensor] = None):
    """Island removal with label_components' tables -> (out uint8 [D, H, W], info int32 [n, 6]).  A component of value ids[j] is kept iff
    its size >= max(1, min_voxels[j]) and (keep_largest[j] is false or it is the largest of that value: ties to the smaller canonical
    index; a largest one below min_voxels[j] leaves nothing).  Voxels that are 0 or not in ids stay.  min_voxels: None, one int, a sequence
    or an int32 device tensor [n]; keep_largest: one bool or one per object; out: None (a new volume), or a uint8 volume to fill -- labels
    itself for in place.  info = (components found, voxels found, largest size, its canonical name or 0, components kept, voxels kept).
    Nothing is copied to the host."""
    ids_d, D, H, W, n = _label_volume_args("label_clean", labels, ids, max_voxels=True)
    dev = labels.device
    _device_table("label_clean: comp", comp, torch.int32, labels.shape, labels.device, "labels'")
    _device_table("label_clean: size", size, torch.int32, labels.shape, labels.device, "labels'")
    mask = label_largest_mask(keep_largest, n)
    mv = None
    if isinstance(min_voxels, torch.Tensor):
        mv = min_voxels.to(device=dev, dtype=torch.int32).contiguous()
        _req(mv.shape == (n,), f"label_clean: min_voxels must hold {n} values")
    elif min_voxels is not None:
        vals = [int(min_voxels)] * n if isinstance(min_voxels, int) else [int(v) for v in min_voxels]
        _req(len(vals) == n and all(0 <= v < 2 ** 31 for v in vals), f"label_clean: min_voxels must be {n} counts in 0 .. 2^31 - 1")
        mv = torch.tensor(vals, dtype=torch.int32).to(dev) if any(vals) else None
    if out is None:
        out = torch.empty_like(labels)
    _device_table("label_clean: out", out, torch.uint8, labels.shape, labels.device, "labels'")
    info = torch.empty(n, 6, dtype=torch.int32, device=dev)
    nb = lib().msam2_label_clean_workspace_bytes(n)
    ws = _workspace8(nb, dev)
    check(lib().msam2_label_clean(_p(labels), _p(comp), _p(size), _p(ids_d), n, _p(mv), mask, _p(out), _p(info), _p(ws), nb, D, H, W, _stream()))
    return out, info


def label_overlap(pred: torch.Tensor, gt: torch.Tensor, ids) -> torch.Tensor:
    """counts int32 [D, n, 3] = (|P & G|, |P|, |G|) per slice and object, P = pred == ids[j], G = gt == ids[j], of two uint8 [D, H, W] label
    volumes: the triple label_slices gives with exclusive=True at one threshold.  Nothing is copied to the host."""
    ids_d, D, H, W, n = _label_volume_args("label_overlap", pred, ids, max_voxels=True)
    _device_table("label_overlap: gt", gt, torch.uint8, pred.shape, pred.device, "labels'")
    counts = torch.empty(D, n, 3, dtype=torch.int32, device=pred.device)
    check(lib().msam2_label_overlap(_p(pred), _p(gt), _p(ids_d), D, H, W, n, _p(counts), _stream()))
    return counts


# ---------------------------------------------------------------------------------------------------------------------
# measurements: per-organ geometry, surface and intensity tables of a label volume and its image (csrc/measure.hip)
MEASURE_MAX_BINS = 65536          # csrc/measure.hip MS_MAX_BINS
MEASURE_IMAGE_TYPES = {torch.uint8: 0, torch.int16: 1}


def label_measure(labels: torch.Tensor, ids, image: Optional[torch.Tensor] = None, hist_lo: Optional[int] = None, bins: int = 0,
                  faces: bool = True, out=None):
    """uint8 [D, H, W] label volume (+ the int16 / uint8 image of that shape) -> (moments int64 [n, 14], extent int32 [n, 6], vrange int32
    [n, 2], faces int64 [n, 6] | None, hist int32 [n, bins] | None) on the device, one pass: moments = (count, Sz, Sy, Sx, Szz, Syy, Sxx, Szy,
    Szx, Syx, Sv, Svv, below, above) over the voxels equal to ids[j] (indices z, y, x; image value v; below / above = voxels with v < hist_lo /
    v >= hist_lo + bins; columns 10 - 13 are 0 without an image); extent = inclusive (z0, z1, y0, y1, x0, x1), -1 when absent; vrange =
    (min v, max v), (2^31 - 1, -2^31) when absent or without an image; faces (faces=True) = interior faces per axis z, y, x (axis neighbours of
    which exactly one is the organ), then the faces on the volume's frame per axis; hist (bins >= 1, needs the image) = voxels with
    v == hist_lo + b.  hist_lo: None = 0.  Voxels that are 0 or not in ids belong to no organ.
    out: the five tables of an earlier call (None where skipped), filled in place: with it the call allocates nothing and can be captured.
    ids: host integers (checked: distinct, 1 .. 255), or the device tensor of label_ids() taken as is.  Nothing is copied to the host."""
    ids_d, D, H, W, n = _label_volume_args("label_measure", labels, ids, max_voxels=True)
    dev = labels.device
    bins, lo = int(bins), 0 if hist_lo is None else int(hist_lo)
    _req(0 <= bins <= MEASURE_MAX_BINS, f"label_measure: bins = {bins} (0 = no histogram, else 1 .. {MEASURE_MAX_BINS})")
    _req(-2 ** 31 <= lo < 2 ** 31, f"label_measure: hist_lo = {lo} (an int32)")
    itype = 0
    if image is not None:
        _device_table("label_measure: image", image, (torch.int16, torch.uint8), (D, H, W), dev, "labels'", "int16 or uint8")
        itype = MEASURE_IMAGE_TYPES[image.dtype]
    _req(bins == 0 or image is not None, "label_measure: a histogram needs an image")
    shapes = ((torch.int64, (n, 14)), (torch.int32, (n, 6)), (torch.int32, (n, 2)), (torch.int64, (n, 6)) if faces else None,
              (torch.int32, (n, bins)) if bins else None)
    names = ("moments", "extent", "vrange", "faces", "hist")
    if out is None:
        out = tuple(None if s is None else torch.empty(s[1], dtype=s[0], device=dev) for s in shapes)
    _req(isinstance(out, (tuple, list)) and len(out) == 5, "label_measure: out must be the five tables (moments, extent, vrange, faces, hist)")
    for name, s, t in zip(names, shapes, out):
        if s is None:
            _req(t is None, f"label_measure: out's {name} must be None (the table is not asked for)")
        else:
            _device_table(f"label_measure: out's {name}", t, s[0], s[1], dev, "labels'")
    m, e, v, f, h = out
    check(lib().msam2_label_measure(_p(labels), _p(ids_d), _p(image), itype, D, H, W, n, lo, bins, _p(m), _p(e), _p(v), _p(f), _p(h), _stream()))
    return m, e, v, f, h


# ---------------------------------------------------------------------------------------------------------------------
# instances: contiguous ids, pair tables and painted maps behind PQ / AJI / lesion-wise F1 (csrc/instances.hip)
INSTANCE_MAX_PAIRS = 1 << 26      # csrc/instances.hip INS_MAX_CAP
INSTANCE_MAX_MASKS = 65535        # csrc/instances.hip INS_MAX_MASKS


def _instance_map(what: str, m, dev=None, shape=None):
    """an instance map: int32 contiguous [H, W] or [D, H, W] on the GPU -> (D, H, W)"""
    _req(isinstance(m, torch.Tensor) and m.dtype == torch.int32 and m.dim() in (2, 3) and m.is_contiguous() and m.is_cuda,
         f"{what} must be an int32 contiguous [H, W] or [D, H, W] instance map on the GPU")
    _req(dev is None or m.device == dev, f"{what} must be on the device of the first map")
    _req(shape is None or tuple(m.shape) == tuple(shape), f"{what} must have the shape {list(shape or ())} of the first map")
    D, H, W = (1, *m.shape) if m.dim() == 2 else m.shape
    _req(1 <= D <= LABEL_MAX_SLICES and 1 <= H <= LABEL_MAX_SIDE and 1 <= W <= LABEL_MAX_SIDE and D * H * W <= LABEL_MAX_VOXELS,
         f"{what}: sizes {D} x {H} x {W} (1 .. {LABEL_MAX_SLICES} slices of 1 .. {LABEL_MAX_SIDE} rows and columns, at most 2^31 - 2 voxels)")
    return D, H, W


def instance_remap(map: torch.Tensor, id_bound: int, cap: int, labels: Optional[torch.Tensor] = None, out=None):
    """Instance map with arbitrary ids in 0 .. id_bound - 1 (0 = background) -> (out, orig, size, cls, info): out = the map with contiguous ids
    1 .. n in ascending order of the original id (remap_label(by_size=False)); orig / size / cls int32 [cap] = original id, voxel count and the
    largest value of the uint8 volume `labels` over the instance (0 without labels); info int32 [4] = (instances found, voxels with an id
    outside [0, id_bound): they become 0, 1 if found > cap, 0).  found > cap: out is complete, the tables hold the first cap instances.
    out: the five tensors of an earlier call, filled in place (its map may be `map` itself).  Nothing is copied to the host."""
    D, H, W = _instance_map("instance_remap: map", map)
    dev = map.device
    id_bound, cap = int(id_bound), int(cap)
    _req(1 <= id_bound < 2 ** 31, f"instance_remap: id_bound = {id_bound} (1 .. 2^31 - 1)")
    _req(1 <= cap < 2 ** 31, f"instance_remap: cap = {cap} table rows (1 .. 2^31 - 1)")
    if labels is not None:
        _device_table("instance_remap: labels", labels, torch.uint8, map.shape, dev, "map's")
    if out is None:
        out = (torch.empty_like(map), *(torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(3)), torch.empty(4, dtype=torch.int32, device=dev))
    _req(isinstance(out, (tuple, list)) and len(out) == 5, "instance_remap: out must be the five tensors (out, orig, size, cls, info)")
    for name, t, shape in zip(("map", "orig", "size", "cls", "info"), out, (map.shape, (cap,), (cap,), (cap,), (4,))):
        _device_table(f"instance_remap: out's {name}", t, torch.int32, shape, dev, "map's")
    o, orig, size, cls, info = out
    nb = lib().msam2_instance_remap_workspace_bytes(id_bound)
    ws = torch.empty(nb // 4, dtype=torch.int32, device=dev)
    check(lib().msam2_instance_remap(_p(map), _p(labels), D, H, W, id_bound, _p(o), _p(orig), _p(size), _p(cls), cap, _p(info), _p(ws), nb, _stream()))
    return o, orig, size, cls, info


def instance_apply(map: torch.Tensor, table: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[i] = table[map[i]] for a device int32 [n + 1] table with table[0] == 0 (the caller's contract); an id outside [0, n] gives 0.
    out: None (a new map), or an int32 map of that shape to fill -- `map` itself for in place.  Nothing is copied to the host."""
    _instance_map("instance_apply: map", map)
    _req(isinstance(table, torch.Tensor) and table.dim() == 1 and table.numel() >= 1, "instance_apply: table must be int32 [n + 1]")
    _device_table("instance_apply: table", table, torch.int32, table.shape, map.device, "map's")
    if out is None:
        out = torch.empty_like(map)
    _device_table("instance_apply: out", out, torch.int32, map.shape, map.device, "map's")
    check(lib().msam2_instance_apply(_p(map), _p(table), table.numel() - 1, map.numel(), _p(out), _stream()))
    return out


def instance_pairs_workspace(na: int, cap: int, dev) -> torch.Tensor:
    """the workspace instance_pairs needs for na instances in `a` and cap pair rows"""
    nb = lib().msam2_instance_pairs_workspace_bytes(int(na), int(cap))
    _req(nb > 0, f"instance_pairs: na = {na} instances (1 .. 2^31 - 2) or cap = {cap} pair rows (1 .. {INSTANCE_MAX_PAIRS})")
    return _workspace8(nb, dev)


def instance_pairs(a: torch.Tensor, b: torch.Tensor, na: int, nb: int, cap: int, out=None, workspace: Optional[torch.Tensor] = None):
    """Two instance maps of one shape with contiguous ids (a: 1 .. na, b: 1 .. nb, 0 = background) -> (pairs int32 [cap, 3], area_a int32 [na],
    area_b int32 [nb], info int32 [4]): pairs = rows (i, j, |a == i and b == j|) of every non-empty pair sorted by (i, j), rows beyond
    info[0] are 0; info = (rows written, 1 if the distinct pairs exceeded cap: no row is written then, voxels of a with an id outside
    [0, na]: background, the same for b).  out: the four tables of an earlier call, workspace: instance_pairs_workspace(na, cap, device) --
    with both the call allocates nothing and can be captured.  Nothing is copied to the host: the caller checks info[1]."""
    D, H, W = _instance_map("instance_pairs: a", a)
    dev = a.device
    _instance_map("instance_pairs: b", b, dev, a.shape)
    na, nb, cap = int(na), int(nb), int(cap)
    _req(1 <= na <= LABEL_MAX_VOXELS and 1 <= nb <= LABEL_MAX_VOXELS, f"instance_pairs: na = {na}, nb = {nb} instances (1 .. 2^31 - 2)")
    _req(1 <= cap <= INSTANCE_MAX_PAIRS, f"instance_pairs: cap = {cap} pair rows (1 .. {INSTANCE_MAX_PAIRS})")
    shapes = ((cap, 3), (na,), (nb,), (4,))
    if out is None:
        out = tuple(torch.empty(s, dtype=torch.int32, device=dev) for s in shapes)
    _req(isinstance(out, (tuple, list)) and len(out) == 4, "instance_pairs: out must be the four tables (pairs, area_a, area_b, info)")
    for name, t, s in zip(("pairs", "area_a", "area_b", "info"), out, shapes):
        _device_table(f"instance_pairs: out's {name}", t, torch.int32, s, dev, "a's")
    need = lib().msam2_instance_pairs_workspace_bytes(na, cap)
    if workspace is None:
        workspace = _workspace8(need, dev)
    _req(isinstance(workspace, torch.Tensor) and workspace.dtype == torch.int64 and workspace.is_contiguous() and workspace.device == dev and
         workspace.numel() * 8 >= need, f"instance_pairs: workspace must be int64 contiguous with at least {need} bytes on a's device")
    pairs, area_a, area_b, info = out
    check(lib().msam2_instance_pairs(_p(a), _p(b), D, H, W, na, nb, _p(pairs), cap, _p(area_a), _p(area_b), _p(info), _p(workspace),
                                     workspace.numel() * 8, _stream()))
    return pairs, area_a, area_b, info


def instance_paint(masks: torch.Tensor, order: Optional[torch.Tensor] = None, boxes: Optional[torch.Tensor] = None, skip_covered: bool = True,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """masks uint8 [N, H, W] (non-zero = inside) -> instance map int32 [H, W] painted in the order of `order` (int32 [N] mask indices on the
    device; None = 0 .. N - 1) by the rule of func_2d/function.py:621-624: at position k the mask is skipped if none of its pixels is still 0
    in the map, else all its pixels become k + 1.  skip_covered=False paints every mask.  boxes int32 [N, 4] (per mask: x0, y0, x1, y1
    inclusive): pixels outside the box count as outside the mask.  Nothing is copied to the host."""
    _req(isinstance(masks, torch.Tensor) and masks.dtype == torch.uint8 and masks.dim() == 3 and masks.is_contiguous() and masks.is_cuda,
         "instance_paint: masks must be a uint8 contiguous [N, H, W] tensor on the GPU")
    N, H, W = masks.shape
    dev = masks.device
    _req(1 <= N <= INSTANCE_MAX_MASKS, f"instance_paint: {N} masks (1 .. {INSTANCE_MAX_MASKS})")
    _req(1 <= H <= LABEL_MAX_SIDE and 1 <= W <= LABEL_MAX_SIDE, f"instance_paint: H x W = {H} x {W} (1 .. {LABEL_MAX_SIDE} rows and columns)")
    if order is not None:
        _device_table("instance_paint: order", order, torch.int32, (N,), dev, "masks'")
    if boxes is not None:
        _device_table("instance_paint: boxes", boxes, torch.int32, (N, 4), dev, "masks'")
    if out is None:
        out = torch.empty(H, W, dtype=torch.int32, device=dev)
    _device_table("instance_paint: out", out, torch.int32, (H, W), dev, "masks'")
    nb = lib().msam2_instance_paint_workspace_bytes(N)
    ws = torch.empty(nb // 4, dtype=torch.int32, device=dev)
    check(lib().msam2_instance_paint(_p(masks), N, H, W, _p(order), _p(boxes), 1 if skip_covered else 0, _p(out), _p(ws), nb, _stream()))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# after the overlap scores: exact distance transforms and surface distances of label volumes (csrc/surface.hip)
EDT_FEATURES = {"surface": 0, "outside": 1}
SURFACE_WORKSPACE_BYTES = 512 << 20    # an interface default, not a measured optimum


def _spacing(what: str, spacing):
    """(sz, sy, sx) as floats; each positive with a square that is a normal float64 and at most 2.6e297 (no product with a squared index
    difference below 2^33 overflows, none flushes to 0): the range the library accepts"""
    sp = tuple(float(s) for s in spacing)
    _req(len(sp) == 3 and all(s > 0.0 and 2.2250738585072014e-308 <= s * s <= 1.7976931348623157e308 / 2.0 ** 36 for s in sp),
         f"{what}: spacing must be three positive values (sz, sy, sx) with squares in 2.3e-308 .. 2.6e297, got {sp}")
    return sp


def label_edt(labels: torch.Tensor, value: int, spacing=(1.0, 1.0, 1.0), features: str = "surface", box=None) -> torch.Tensor:
    """Exact squared Euclidean distance transform of one value of a uint8 [D, H, W] label volume (H, W >= 2) inside a box -> float64
    [bd, bh, bw] on the device: d2 = min over the features f of ((sx^2 dx^2 + sy^2 dy^2) + sz^2 dz^2), every product and sum rounded on its
    own -- the bits of the brute-force minimum (at unit spacing an exact integer), +inf when the box holds no feature.
    features="surface": the voxels equal to `value` with a face neighbour that differs or lies outside the volume (6 neighbours; the 4 in
    plane when D == 1); "outside": the voxels != value (the classic in-mask distance; beyond the volume there are no features).
    box: host integers (z0, z1, y0, y1, x0, x1), inclusive, default the whole volume; features are taken from the box only.
    Nothing is copied to the host."""
    _, D, H, W, _ = _label_volume_args("label_edt", labels, None, min_side=2, max_voxels=True)
    _req(features in EDT_FEATURES, f"label_edt: features {features!r} (one of {tuple(EDT_FEATURES)})")
    _req(0 <= int(value) <= 255, f"label_edt: value {value} (0 .. 255)")
    sz, sy, sx = _spacing("label_edt", spacing)
    bx = [0, D - 1, 0, H - 1, 0, W - 1] if box is None else [int(b) for b in box]
    _req(len(bx) == 6 and 0 <= bx[0] <= bx[1] < D and 0 <= bx[2] <= bx[3] < H and 0 <= bx[4] <= bx[5] < W,
         f"label_edt: box {bx} must be (z0, z1, y0, y1, x0, x1), inclusive, inside the {D} x {H} x {W} volume")
    bd, bh, bw = bx[1] - bx[0] + 1, bx[3] - bx[2] + 1, bx[5] - bx[4] + 1
    dev = labels.device
    d2 = torch.empty(bd, bh, bw, dtype=torch.float64, device=dev)
    nb = lib().msam2_label_edt_workspace_bytes(bd, bh, bw)
    ws = _workspace8(nb, dev)
    check(lib().msam2_label_edt(_p(labels), D, H, W, int(value), EDT_FEATURES[features], (ctypes.c_int32 * 6)(*bx), sz, sy, sx, _p(d2), _p(ws), nb,
                                _stream()))
    return d2


def _organ_extents(stats: "torch.Tensor"):
    """label_stats' table on the host, int64 [D, n, 5] -> per organ (count, (z0, z1, y0, y1, x0, x1) or None)"""
    D, n, _ = stats.shape
    out = []
    for j in range(n):
        s = stats[:, j]
        zs = (s[:, 0] > 0).nonzero()[0]
        if len(zs) == 0:
            out.append((0, None))
            continue
        p = s[zs]
        out.append((int(p[:, 0].sum()), (int(zs[0]), int(zs[-1]), int(p[:, 1].min()), int(p[:, 2].max()), int(p[:, 3].min()), int(p[:, 4].max()))))
    return out


def _organ_boxes(what: str, volumes, ids_d: torch.Tensor, distinct: bool = True, extra: Optional[torch.Tensor] = None):
    """The preparation of the entries that work per organ inside a box -> (values, per volume: `_organ_extents`' list).  One `label_stats`
    call per volume (z extent: the slices with count > 0; rows and columns: the stats' min / max), then ONE device-to-host copy of those
    small tables with the ids: the only synchronisation on the way in.  distinct: ids taken from the device as they are must still be
    distinct values in 1 .. 255.  extra: an integer device table that rides in the same copy; it comes back flat, as a third result."""
    D, n = volumes[0].shape[0], ids_d.numel()
    tables = [label_stats(v, ids_d)[0].reshape(-1) for v in volumes] + [ids_d.to(torch.int32)]
    if extra is not None:
        tables = [t.to(torch.int64) for t in tables] + [extra.reshape(-1).to(torch.int64)]
    host = torch.cat(tables).cpu().numpy().astype("int64")                                                 # the one copy
    m = D * n * 5
    values = host[len(volumes) * m: len(volumes) * m + n].tolist()
    _req(not distinct or (len(set(values)) == n and all(1 <= v <= 255 for v in values)), f"{what}: ids must be distinct values in 1 .. 255")
    extents = [_organ_extents(host[k * m: (k + 1) * m].reshape(D, n, 5)) for k in range(len(volumes))]
    return (values, extents) if extra is None else (values, extents, host[len(volumes) * m + n:])


def _boxes_or_empty(extents):
    """`_organ_extents`' list -> a box per organ, the voxel (0, 0, 0) for an absent one"""
    return [list(box) if box is not None else [0, 0, 0, 0, 0, 0] for _, box in extents]


def _out_volume(what: str, labels: torch.Tensor, out: Optional[torch.Tensor]):
    """out=None (a new volume) or a uint8 volume to fill, labels itself for in place -> (out, in_place as the library's int)"""
    if out is None:
        out = torch.empty_like(labels)
    _device_table(f"{what}: out", out, torch.uint8, labels.shape, labels.device, "labels'")
    return out, int(out.data_ptr() == labels.data_ptr())


def _box_workspace(what: str, values, per_box_need, all_at_once_need: int, workspace_bytes: int, dev):
    """per_box_need[j]: what the box of values[j] alone needs -- refused above workspace_bytes -> (workspace, its bytes): what all organs need
    at once, at most workspace_bytes (the library then goes through them in groups), 16-byte granular"""
    for v, nb in zip(values, per_box_need):
        _req(nb <= workspace_bytes, f"{what}: the box of id {v} alone needs a workspace of {nb} bytes, workspace_bytes is {workspace_bytes}")
    nb = min(int(all_at_once_need), int(workspace_bytes))
    return torch.empty((nb + 15) // 16 * 2, dtype=torch.int64, device=dev), nb                           # (the caching allocator aligns to 512 bytes)


def label_surface_distances(pred: torch.Tensor, gt: torch.Tensor, ids, spacing=(1.0, 1.0, 1.0), workspace_bytes: int = SURFACE_WORKSPACE_BYTES):
    """`surface_segments` with offsets int64 [n, 2] and capacity int32 [n, 2] as device tensors beside dist and counts: everything on the
    device (the two small tables go there in one asynchronous copy each)."""
    dist, offs, caps, counts = surface_segments(pred, gt, ids, spacing, workspace_bytes)
    n = len(offs)
    dev = pred.device
    return dist, torch.tensor(offs, dtype=torch.int64).reshape(n, 2).to(dev), torch.tensor(caps, dtype=torch.int32).reshape(n, 2).to(dev), counts


def surface_segments(pred: torch.Tensor, gt: torch.Tensor, ids, spacing=(1.0, 1.0, 1.0), workspace_bytes: int = SURFACE_WORKSPACE_BYTES):
    """The squared surface distances behind HD95 / ASSD / NSD of two uint8 [D, H, W] label volumes (H, W >= 2) on the device ->
    (dist float64 [total] (device), offsets [n][2] and capacity [n][2] (host lists: the caller slices with them), counts int32 [n, 2] (device)).
    Segment (j, 0) = dist[offsets[j, 0]: offsets[j, 0] + counts[j, 0]] holds d2(q, surface of ids[j] in gt) for every voxel q on the surface of
    ids[j] in pred, segment (j, 1) the other direction (`label_edt`'s definitions and bits); the order inside a segment is unspecified, the
    rest of the segment up to its capacity (the organ's voxel count there) is +inf, so a sort of the whole segment puts the values first.
    An organ absent from either volume stores nothing (capacity 0; the count of the side that has it is still reported).

    The boxes and capacities come from `_organ_boxes` over pred and gt (box = the union of the two extents; capacity = the summed count): its
    one device-to-host copy is the only synchronisation on the way in; nothing else is copied to the host.
    Organs are processed in groups whose workspace (20 bytes per box voxel) stays below `workspace_bytes`; an organ whose box alone needs more
    raises with the needed size in the message."""
    ids_d, D, H, W, n = _label_volume_args("label_surface_distances", pred, ids, min_side=2, max_voxels=True)
    _device_table("label_surface_distances: gt", gt, torch.uint8, pred.shape, pred.device, "labels'")
    sz, sy, sx = _spacing("label_surface_distances", spacing)
    dev = pred.device
    values, (ext_p, ext_g) = _organ_boxes("label_surface_distances", (pred, gt), ids_d, distinct=False)   # (an id listed twice is scored twice)
    boxes, caps, offs, total = [], [], [], 0
    for (cp, bp), (cg, bg) in zip(ext_p, ext_g):
        both = bp is not None and bg is not None
        one = bp or bg or (0, 0, 0, 0, 0, 0)
        other = bg if both else one
        boxes.append([min(one[0], other[0]), max(one[1], other[1]), min(one[2], other[2]), max(one[3], other[3]), min(one[4], other[4]),
                      max(one[5], other[5])])
        caps.append([cp if both else 0, cg if both else 0])
        offs.append([total, total + caps[-1][0]])
        total += sum(caps[-1])
    dist = torch.full((max(total, 1),), float("inf"), dtype=torch.float64, device=dev)
    counts = torch.empty(n, 2, dtype=torch.int32, device=dev)
    L = lib()
    need = [L.msam2_label_surface_distances_workspace_bytes((ctypes.c_int32 * 6)(*b), 1) for b in boxes]
    groups, cur, used = [], [], 0
    for j, nb in enumerate(need):
        if cur and used + nb > workspace_bytes:
            groups.append(cur)
            cur, used = [], 0
        cur.append(j)
        used += nb
    groups.append(cur)
    ws, _ = _box_workspace("label_surface_distances", values, need, max(sum(need[j] for j in g) for g in groups), workspace_bytes, dev)
    for g in groups:
        k = len(g)
        flat = lambda rows: [v for j in g for v in rows[j]]                                                 # noqa: E731
        check(L.msam2_label_surface_distances(_p(pred), _p(gt), D, H, W, (ctypes.c_uint8 * k)(*[values[j] for j in g]),
                                              (ctypes.c_int32 * (6 * k))(*flat(boxes)), (ctypes.c_int64 * (2 * k))(*flat(offs)),
                                              (ctypes.c_int32 * (2 * k))(*flat(caps)), k, sz, sy, sx, _p(dist), dist.numel(),
                                              counts[g[0]:].data_ptr(), _p(ws), ws.numel() * 8, _stream()))
    return dist, offs, caps, counts


# ---------------------------------------------------------------------------------------------------------------------
# after island removal: the enclosed holes of every organ, 3-D or slice by slice (csrc/holes.hip)
HOLE_CLAIMS = {"background": 0, "any": 1}
HOLES_WORKSPACE_BYTES = 1 << 30    # an interface default, not a measured optimum


def label_fill_holes(labels: torch.Tensor, ids, connectivity: int = 6, max_voxels=None, claim: str = "background",
                     out: Optional[torch.Tensor] = None, workspace_bytes: int = HOLES_WORKSPACE_BYTES):
    """scipy.ndimage.binary_fill_holes per organ of a uint8 [D, H, W] label volume on the device -> (out uint8 [D, H, W], info int32 [n, 4]).
    A hole of v = ids[j] is a connected component of {voxels != v} under `connectivity` -- that of the BACKGROUND FLOOD, binary_fill_holes'
    structure: 6 (scipy's default, the dual of 26-connected organs) / 18 / 26 in 3-D, 4 / 8 in plane, every slice on its own -- that holds no
    voxel of the frame (the six faces of the volume; in plane the four edges of the slice).  Its size counts all its voxels, whatever they
    carry; it qualifies iff max_voxels[j] == 0 or size <= max_voxels[j]; a voxel of it is eligible iff its input value is 0
    (claim="background") or always ("any").  out = ids[j*] for the smallest j* such that the voxel is eligible in a qualifying hole of ids[j*],
    else labels.  All holes are holes of the input: the order of ids decides only who gets a voxel that lies in the holes of several organs.
    max_voxels: None, one int, a sequence or an int32 device tensor [n]; out: None (a new volume), or a uint8 volume to fill -- labels itself
    for in place (a D*H*W-byte snapshot of the input then rides in the workspace).  info = (holes found, voxels in them, holes that
    qualify, voxels of out that are ids[j] and were not in labels).

    The boxes come from `_organ_boxes`: its one device-to-host copy is the only synchronisation, nothing else is copied to the host.
    Organs go through in groups whose workspace (9 bytes per box voxel, and the snapshot) stays below
    `workspace_bytes`; an organ whose box alone needs more raises with the needed size in the message."""
    ids_d, D, H, W, n = _label_volume_args("label_fill_holes", labels, ids, max_voxels=True)
    _req(int(connectivity) in LABEL_CONNECTIVITIES, f"label_fill_holes: connectivity {connectivity} (one of {LABEL_CONNECTIVITIES})")
    _req(claim in HOLE_CLAIMS, f"label_fill_holes: claim {claim!r} (one of {tuple(HOLE_CLAIMS)})")
    dev = labels.device
    mv = None
    if isinstance(max_voxels, torch.Tensor):
        mv = max_voxels.to(device=dev, dtype=torch.int32).contiguous()
        _req(mv.shape == (n,), f"label_fill_holes: max_voxels must hold {n} values")
    elif max_voxels is not None:
        vals = [int(max_voxels)] * n if isinstance(max_voxels, int) else [int(v) for v in max_voxels]
        _req(len(vals) == n and all(0 <= v < 2 ** 31 for v in vals), f"label_fill_holes: max_voxels must be {n} counts in 0 .. 2^31 - 1")
        mv = torch.tensor(vals, dtype=torch.int32).to(dev) if any(vals) else None
    out, in_place = _out_volume("label_fill_holes", labels, out)
    values, (extents,) = _organ_boxes("label_fill_holes", (labels,), ids_d)
    boxes = _boxes_or_empty(extents)
    L = lib()
    c, flat = int(connectivity), (ctypes.c_int32 * (6 * n))(*[v for b in boxes for v in b])
    need = [L.msam2_label_fill_holes_workspace_bytes(D, H, W, (ctypes.c_int32 * 6)(*b), 1, c, in_place, 0) for b in boxes]
    ws, nb = _box_workspace("label_fill_holes", values, need, L.msam2_label_fill_holes_workspace_bytes(D, H, W, flat, n, c, in_place, 1),
                            workspace_bytes, dev)
    info = torch.empty(n, 4, dtype=torch.int32, device=dev)
    check(L.msam2_label_fill_holes(_p(labels), D, H, W, (ctypes.c_uint8 * n)(*values), flat, n, c, _p(mv), HOLE_CLAIMS[claim], _p(out), _p(info),
                                   _p(ws), nb, _stream()))
    return out, info


# ---------------------------------------------------------------------------------------------------------------------
# out of the label volume: closed surface meshes per organ, surface nets or voxel faces (csrc/mesh.hip)
MESH_PLACEMENTS = {"corner": 0, "nets": 1}
MESH_MAX_RELAX = 64                    # csrc/mesh.hip MESH_MAX_RELAX
MESH_MAX_LATTICE = 1 << 29             # csrc/mesh.hip MESH_MAX_LATTICE
MESH_WORKSPACE_BYTES = 2 << 30         # an interface default, not a measured optimum


def label_mesh_sizes(labels: torch.Tensor, ids) -> torch.Tensor:
    """uint8 [D, H, W] label volume -> int64 [n, 2] on the device: (vertices, quads) of the surface mesh of every listed organ -- lattice
    points whose eight voxels are not all equal in labels == ids[j] (voxels outside the volume are not the organ), and voxel faces between
    the organ and anything else, the volume's frame included (the row sums of label_measure's faces).  One pass, integer adds.
    ids: host integers (checked: distinct, 1 .. 255), or the device tensor of label_ids() taken as is.  Nothing is copied to the host."""
    ids_d, D, H, W, n = _label_volume_args("label_mesh_sizes", labels, ids, max_voxels=True)
    counts = torch.empty(n, 2, dtype=torch.int64, device=labels.device)
    check(lib().msam2_label_mesh_count(_p(labels), _p(ids_d), D, H, W, n, _p(counts), _stream()))
    return counts


def label_mesh(labels: torch.Tensor, ids, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), placement: str = "nets", relax: int = 0,
               workspace_bytes: int = MESH_WORKSPACE_BYTES):
    """`label_mesh_with_values` without its last result: (vertices, quads, v_offsets, q_offsets, counts)."""
    return label_mesh_with_values(labels, ids, spacing, origin, placement, relax, workspace_bytes)[:5]


def label_mesh_with_values(labels: torch.Tensor, ids, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), placement: str = "nets", relax: int = 0,
                           workspace_bytes: int = MESH_WORKSPACE_BYTES):
    """Closed, consistently oriented surface meshes of the organs of a uint8 [D, H, W] label volume on the device -> (vertices float32
    [nv, 3] (rows (z, y, x), physical units), quads int32 [nq, 4], v_offsets [n + 1] and q_offsets [n + 1] (host lists: organ j owns
    vertices[v_offsets[j]: v_offsets[j + 1]] and quads[q_offsets[j]: q_offsets[j + 1]], whose entries are its own vertex numbers from 0),
    counts int32 [n, 2] (device): the (vertices, quads) the library found, equal to the segments' lengths, values: the label values as
    host integers -- they came with the one copy, so a caller that gave ids as a device tensor need not read them back).
    A vertex per lattice point (corner of eight voxels) whose voxels are not all inside or all outside the organ, in ascending lattice
    order; a quad per voxel face between organ and not-organ (voxels beyond the volume are not the organ: an organ cut by the field of view
    is closed), wound so that its normal looks out, ordered by (lowest lattice corner, axis z / y / x).  placement="corner": vertices at the
    voxel corners (the voxel-face surface); "nets": at the mean of the midpoints of the cell's crossed edges (surface nets).  relax: 0 .. 64
    Jacobi sweeps towards the mean of the linked vertices, every vertex kept inside its own cell.  A voxel centre (z, y, x) sits at
    origin + (z sz, y sy, x sx).  DESIGN 7.22 has the exact arithmetic; the tables are equal to its restatement bit for bit.

    The sizes (`label_mesh_sizes`) ride in the one device-to-host copy of `_organ_boxes`: the only synchronisation on the way in, nothing
    else is copied to the host.  Organs go through in groups whose workspace (about 1.25 bytes per lattice point of the organ's box, 48
    more with relax > 0) stays below `workspace_bytes`; an organ whose box alone needs more raises with the needed size in the message."""
    ids_d, D, H, W, n = _label_volume_args("label_mesh", labels, ids, max_voxels=True)
    _req(placement in MESH_PLACEMENTS, f"label_mesh: placement {placement!r} (one of {tuple(MESH_PLACEMENTS)})")
    relax = int(relax)
    _req(0 <= relax <= MESH_MAX_RELAX, f"label_mesh: relax = {relax} sweeps (0 .. {MESH_MAX_RELAX})")
    sp = _spacing("label_mesh", spacing)
    og = tuple(float(o) for o in origin)
    _req(len(og) == 3 and all(o - o == 0.0 for o in og), f"label_mesh: origin must be three finite values (oz, oy, ox), got {og}")
    dev = labels.device
    values, (extents,), sizes = _organ_boxes("label_mesh", (labels,), ids_d, extra=label_mesh_sizes(labels, ids_d))
    boxes = _boxes_or_empty(extents)
    sizes = sizes.reshape(n, 2)
    for v, b in zip(values, boxes):
        lattice = (b[1] - b[0] + 2) * (b[3] - b[2] + 2) * (b[5] - b[4] + 2)
        _req(lattice <= MESH_MAX_LATTICE, f"label_mesh: the box of id {v} has {lattice} lattice points (at most 2^29 per organ)")
    v_offs = [0] + [int(x) for x in sizes[:, 0].cumsum()]
    q_offs = [0] + [int(x) for x in sizes[:, 1].cumsum()]
    # (an empty tensor's data_ptr() is 0 and the entry refuses NULL tables: keep one row when every organ is absent, slice afterwards)
    vertices = torch.empty(max(v_offs[-1], 1), 3, dtype=torch.float32, device=dev)
    quads = torch.empty(max(q_offs[-1], 1), 4, dtype=torch.int32, device=dev)
    counts = torch.empty(n, 2, dtype=torch.int32, device=dev)
    L = lib()
    need = [L.msam2_label_mesh_workspace_bytes((ctypes.c_int32 * 6)(*b), relax) for b in boxes]
    ws, nb = _box_workspace("label_mesh", values, need, sum(need), workspace_bytes, dev)
    i64 = lambda rows: (ctypes.c_int64 * n)(*[int(r) for r in rows])                                       # noqa: E731
    check(L.msam2_label_mesh(_p(labels), D, H, W, (ctypes.c_uint8 * n)(*values), (ctypes.c_int32 * (6 * n))(*[v for b in boxes for v in b]),
                             i64(v_offs[:-1]), i64(sizes[:, 0]), i64(q_offs[:-1]), i64(sizes[:, 1]), n, MESH_PLACEMENTS[placement], relax,
                             (ctypes.c_double * 3)(*sp), (ctypes.c_double * 3)(*og), vertices.data_ptr(), quads.data_ptr(), _p(counts), _p(ws), nb,
                             _stream()))
    return vertices[:v_offs[-1]], quads[:q_offs[-1]], v_offs, q_offs, counts, values


# ---------------------------------------------------------------------------------------------------------------------
# between the label volume and the scores: erosion, dilation, opening, closing by a ball of a physical radius (csrc/morph.hip)
MORPH_OPS = {"erode": 0, "dilate": 1, "open": 2, "close": 3}
MORPH_WORKSPACE_BYTES = 2 << 30    # an interface default, not a measured optimum


def _radius2(what: str, radius, radius2, n: int):
    """radius= / radius2= (one value, or one per object) -> n squared radii as floats: r2 = float(radius) * float(radius), or radius2 as is"""
    _req((radius is None) != (radius2 is None), f"{what}: exactly one of radius and radius2")
    given = radius if radius2 is None else radius2
    vals = [float(v) for v in (given.tolist() if isinstance(given, torch.Tensor) else given)] if hasattr(given, "__len__") else [float(given)] * n
    r2 = [v * v for v in vals] if radius2 is None else vals
    _req(len(vals) == n and all(0.0 <= v < float("inf") for v in vals + r2),
         f"{what}: radius / radius2 must be one value or {n} values, each >= 0 with a finite square")
    return r2


def label_morph(labels: torch.Tensor, ids, op: str, radius=None, radius2=None, spacing=(1.0, 1.0, 1.0), claim: str = "background",
                out: Optional[torch.Tensor] = None, workspace_bytes: int = MORPH_WORKSPACE_BYTES):
    """Erosion, dilation, opening or closing of every listed organ of a uint8 [D, H, W] label volume (H, W >= 2) by a ball of a physical
    radius, on the device -> (out uint8 [D, H, W], info int32 [n, 4]).  d2(q, f) = ((sx^2 dx^2 + sy^2 dy^2) + sz^2 dz^2) in float64 as
    `label_edt` computes it; the ball is d2 <= r2, with <=.  r2 reaches the library as a float64: radius= gives float(radius) * float(radius),
    radius2= gives it directly, exactly one of the two (one value, or one per object).  (3 ** 0.5) ** 2 == 2.9999999999999996: radius=sqrt(3)
    does NOT reach a voxel at d2 = 3, radius2=3.0 does.
    With M = (labels == ids[j]): dilate = {q in the volume: min over f in M of d2(q, f) <= r2}; erode = {q in M: no voxel f of the volume
    outside M has d2(q, f) <= r2} -- there are no features beyond the volume, so an organ cut by the field of view does not erode from the frame
    (`label_edt(features="outside")`; at unit spacing scipy's binary_erosion(border_value=1)); open = dilate(erode(M)), close = erode(dilate(M)).
    erode / open: a voxel of a listed organ that is not in its result becomes 0, everything else stays.  dilate / close: a voxel may change only
    if it is eligible -- its input value is 0 (claim="background") or not in ids ("any": an unlisted lesion may be overwritten); a listed organ
    never loses a voxel; an eligible voxel inside the results of several organs goes to the organ whose ORIGINAL mask is nearest (smallest d2),
    ties to the organ earlier in ids: a margin between two neighbours is split along their mid-surface.
    out: None (a new volume), or a uint8 volume to fill -- labels itself for in place (a D*H*W-byte snapshot of the input then rides in the
    workspace).  info = (voxels before, voxels in the organ's own result set, voxels after, voxels taken from non-zero values); an absent organ
    gives a row of zeros and changes nothing.

    The boxes come from `_organ_boxes`: its one device-to-host copy is the only synchronisation, nothing else is copied to the host.
    Organs go through in groups whose workspace (19 bytes per voxel of the organ's box grown by the ball,
    11 for erode / open; dilate / close also 8 bytes per voxel of the volume) stays below `workspace_bytes`; an organ whose box alone needs more
    raises with the needed size in the message.  The result depends on neither the grouping nor the boxes."""
    ids_d, D, H, W, n = _label_volume_args("label_morph", labels, ids, min_side=2, max_voxels=True)
    _req(op in MORPH_OPS, f"label_morph: op {op!r} (one of {tuple(MORPH_OPS)})")
    _req(claim in HOLE_CLAIMS, f"label_morph: claim {claim!r} (one of {tuple(HOLE_CLAIMS)})")
    sz, sy, sx = _spacing("label_morph", spacing)
    r2 = _radius2("label_morph", radius, radius2, n)
    dev = labels.device
    out, in_place = _out_volume("label_morph", labels, out)
    values, (extents,) = _organ_boxes("label_morph", (labels,), ids_d)
    boxes = _boxes_or_empty(extents)
    L = lib()
    o, flat, r2s = MORPH_OPS[op], (ctypes.c_int32 * (6 * n))(*[v for b in boxes for v in b]), (ctypes.c_double * n)(*r2)
    need = [L.msam2_label_morph_workspace_bytes(D, H, W, (ctypes.c_int32 * 6)(*b), 1, o, (ctypes.c_double * 1)(r2[j]), sz, sy, sx, in_place, 0)
            for j, b in enumerate(boxes)]
    for v, nb in zip(values, need):
        _req(nb > 0, f"label_morph: the box of id {v} grown by its ball has more than 2^25 rows (slices x rows)")
    ws, nb = _box_workspace("label_morph", values, need, L.msam2_label_morph_workspace_bytes(D, H, W, flat, n, o, r2s, sz, sy, sx, in_place, 1),
                            workspace_bytes, dev)
    info = torch.empty(n, 4, dtype=torch.int32, device=dev)
    check(L.msam2_label_morph(_p(labels), D, H, W, (ctypes.c_uint8 * n)(*values), flat, n, o, r2s, sz, sy, sx, HOLE_CLAIMS[claim], _p(out),
                              _p(info), _p(ws), nb, _stream()))
    return out, info


# ---------------------------------------------------------------------------------------------------------------------
# 2-D memory bank (csrc/bank.hip); every tensor fp32.  Operands of bank_dots / bank_commit are 3-D views [rows, n_ch, n_px] with
# arbitrary strides, read in place.
BANK_MAX = 32          # physical slots the device tables are laid out for
BANK_MAX_ROWS = 8      # candidates / images of a step


def _bank_operand(t: torch.Tensor, what: str):
    _req(t.dim() == 3 and t.dtype == F32, f"{what}: fp32 [rows, n_ch, n_px] view")
    return _p(t), (ctypes.c_int64 * 3)(*t.stride())


def bank_dots_chain(K: int, vec: int) -> int:
    """n of the bound |computed - exact| <= gamma_n sum|x_i y_i| of bank_dots for rows of K elements read `vec` (1 / 4) at a time."""
    return lib().msam2_bank_dots_chain(int(K), int(vec))


def bank_dots_workspace(R: int, Cn: int, device) -> torch.Tensor:
    return torch.empty(max(lib().msam2_bank_dots_workspace_bytes(R, Cn), 4) // 4, dtype=F32, device=device)


def bank_dots(x: torch.Tensor, y: torch.Tensor, y2: Optional[torch.Tensor] = None, *, dots: Optional[torch.Tensor] = None,
              xx: Optional[torch.Tensor] = None, yy: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """dots [R, Cn] = X Y^T over the flattened (n_ch, n_px) maps, Y = rows of y then rows of y2; xx [R], yy [Cn] squared norms
    (written when given).  Returns dots."""
    px, sx = _bank_operand(x, "bank_dots x")
    py, sy = _bank_operand(y, "bank_dots y")
    R, n_ch, n_px = x.shape
    rows_a = y.shape[0]
    _req(tuple(y.shape[1:]) == (n_ch, n_px), "bank_dots: y rows differ in shape from x rows")
    py2, sy2, rows_b = None, None, 0
    if y2 is not None:
        py2, sy2 = _bank_operand(y2, "bank_dots y2")
        rows_b = y2.shape[0]
        _req(tuple(y2.shape[1:]) == (n_ch, n_px), "bank_dots: y2 rows differ in shape from x rows")
    Cn = rows_a + rows_b
    if dots is None:
        dots = torch.empty(R, Cn, dtype=F32, device=x.device)
    _req(dots.dtype == F32 and dots.is_contiguous() and dots.numel() >= R * Cn, "bank_dots: dots fp32 contiguous [R, Cn]")
    if workspace is None:
        workspace = bank_dots_workspace(R, Cn, x.device)
    check(lib().msam2_bank_dots(px, sx, R, py, sy, rows_a, py2, sy2, rows_b, n_ch, n_px, _p(dots), _p(xx), _p(yy), _p(workspace),
                                workspace.numel() * 4, _stream()))
    return dots


def bank_sample(dots: torch.Tensor, xx: torch.Tensor, yy: torch.Tensor, order: torch.Tensor, N: int, cap: int, u: torch.Tensor,
                indices: Optional[torch.Tensor] = None, probs: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 indices [B, S] (logical bank positions) drawn by inverse CDF with the uniforms u [B, S] from softmax(cosines)."""
    _req(dots.dim() == 2 and dots.dtype == F32 and dots.stride(1) == 1 and u.dim() == 2 and u.dtype == F32 and u.is_contiguous(),
         "bank_sample: dots fp32 [B, >= cap], u fp32 contiguous [B, S]")
    _req(order.dtype == torch.int32 and order.numel() >= BANK_MAX, "bank_sample: order int32 [32]")
    B, S = u.shape
    _req(dots.shape[0] == B and dots.shape[1] >= N, "bank_sample: dots rows / columns")
    if indices is None:
        indices = torch.empty(B, S, dtype=torch.int32, device=u.device)
    # the kernel indexes dots by physical slot < cap; a [B, N] tensor (live slots are 0 .. N-1) is addressed with cap = N
    cap_k = min(int(cap), dots.shape[1])
    check(lib().msam2_bank_sample(_p(dots), dots.stride(0), _p(xx), _p(yy), _p(order), int(N), cap_k, _p(u), B, S, _p(indices), _p(probs),
                                  _stream()))
    return indices


def bank_gather(feats: torch.Tensor, pos: torch.Tensor, order: torch.Tensor, indices: torch.Tensor, N: int,
                memory: Optional[torch.Tensor] = None, memory_pos: Optional[torch.Tensor] = None):
    """feats / pos: the bank's token-major stores [cap, HW, C]; indices int32 [B, S] -> memory, memory_pos [S*HW, B, C]."""
    _req(feats.dim() == 3 and feats.is_contiguous() and pos.shape == feats.shape and pos.is_contiguous() and feats.dtype == F32 and pos.dtype == F32,
         "bank_gather: fp32 contiguous stores [cap, HW, C]")
    _req(indices.dtype == torch.int32 and indices.is_contiguous() and indices.dim() == 2, "bank_gather: indices int32 [B, S]")
    cap, HW, C = feats.shape
    B, S = indices.shape
    if memory is None:
        memory = torch.empty(S * HW, B, C, dtype=F32, device=feats.device)
    if memory_pos is None:
        memory_pos = torch.empty(S * HW, B, C, dtype=F32, device=feats.device)
    _req(memory.is_contiguous() and memory_pos.is_contiguous() and memory.numel() == S * HW * B * C and memory_pos.numel() == memory.numel(),
         "bank_gather: outputs fp32 contiguous [S*HW, B, C]")
    check(lib().msam2_bank_gather(_p(feats), _p(pos), _p(order), _p(indices), B, S, HW, C, int(N), cap, _p(memory), _p(memory_pos), _stream()))
    return memory, memory_pos


def bank_decide(gram: torch.Tensor, iou_bank: torch.Tensor, order: torch.Tensor, N: int, cap: int, dots: torch.Tensor,
                iou_pred: torch.Tensor, fill: bool, accept: Optional[torch.Tensor] = None, slot_cand: Optional[torch.Tensor] = None,
                iou_out: Optional[torch.Tensor] = None):
    """Runs the replacement (or fill) loop on the device tables in place; returns (accept int32 [B], slot_cand int32 [32])."""
    _req(gram.dtype == F32 and gram.is_contiguous() and gram.numel() == BANK_MAX * BANK_MAX, "bank_decide: gram fp32 [32, 32]")
    _req(iou_bank.dtype == F32 and iou_bank.numel() == BANK_MAX and order.dtype == torch.int32 and order.numel() == BANK_MAX,
         "bank_decide: iou_bank fp32 [32], order int32 [32]")
    _req(iou_pred.dim() == 2 and iou_pred.dtype == F32 and iou_pred.is_contiguous(), "bank_decide: iou_pred fp32 contiguous [B, M]")
    B, M = iou_pred.shape
    _req(dots.dtype == F32 and dots.is_contiguous() and dots.numel() >= B * (N + B), "bank_decide: dots fp32 contiguous [B, N + B]")
    if accept is None:
        accept = torch.empty(B, dtype=torch.int32, device=gram.device)
    if slot_cand is None:
        slot_cand = torch.empty(BANK_MAX, dtype=torch.int32, device=gram.device)
    check(lib().msam2_bank_decide(_p(gram), _p(iou_bank), _p(order), int(N), int(cap), _p(dots), _p(iou_pred), B, M, 1 if fill else 0, _p(accept),
                                  _p(slot_cand), _p(iou_out), _stream()))
    return accept, slot_cand


def bank_commit(slot_cand: torch.Tensor, feats: torch.Tensor, pos: torch.Tensor, embed: torch.Tensor, feats_store: torch.Tensor,
                pos_store: torch.Tensor, embed_store: torch.Tensor) -> None:
    """feats / pos [B, C, HW] and embed [B, Ce, HW] views (any strides) -> the slots slot_cand names: token-major feats_store / pos_store
    [cap, HW, C], embed_store [cap, Ce*HW] in (channel, pixel) order."""
    pf, sf = _bank_operand(feats, "bank_commit feats")
    pp, sp = _bank_operand(pos, "bank_commit pos")
    pe, se = _bank_operand(embed, "bank_commit embed")
    B, C, HW = feats.shape
    Ce = embed.shape[1]
    cap = feats_store.shape[0]
    _req(pos.shape == feats.shape and embed.shape[0] == B and embed.shape[2] == HW, "bank_commit: candidate shapes")
    _req(feats_store.is_contiguous() and pos_store.is_contiguous() and embed_store.is_contiguous() and feats_store.numel() == cap * HW * C
         and pos_store.numel() == cap * HW * C and embed_store.numel() == cap * Ce * HW and feats_store.dtype == F32 and pos_store.dtype == F32
         and embed_store.dtype == F32, "bank_commit: fp32 contiguous stores [cap, HW, C], [cap, HW, C], [cap, Ce*HW]")
    _req(slot_cand.dtype == torch.int32 and slot_cand.numel() >= cap, "bank_commit: slot_cand int32 [32]")
    check(lib().msam2_bank_commit(_p(slot_cand), cap, pf, sf, pp, sp, C, pe, se, Ce, HW, B, _p(feats_store), _p(pos_store), _p(embed_store),
                                  _stream()))
