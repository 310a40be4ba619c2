"""Argument contracts of the pointwise and conv-tail entries without a GPU: the C entries refuse tensors that their vector accesses cannot take
(fake pointers: a refused call launches nothing), and the Python wrappers that pass raw pointers refuse strided or wrong-typed tensors."""
import ctypes

import pytest
import torch


def test_alignment_refusals_of_the_c_entries():
    """msam2_dwconv7x7_ln loads f32x4 from x, weight and bias and stores four 16-bit values; msam2_hyper_masks loads eight 16-bit values;
    msam2_im2col3x3s2 loads and stores four: none of them checked the alignment of what it was given"""
    from medical_sam2_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    ptr = (ctypes.addressof(buf) + 15) & ~15
    cases = {
        "dwconv7x7_ln: x": lambda: L.msam2_dwconv7x7_ln(ptr + 4, ptr, ptr, ptr, ptr, ptr, 1, 2, 2, 256, None),
        "dwconv7x7_ln: weight": lambda: L.msam2_dwconv7x7_ln(ptr, ptr + 8, ptr, ptr, ptr, ptr, 1, 2, 2, 256, None),
        "dwconv7x7_ln: bias": lambda: L.msam2_dwconv7x7_ln(ptr, ptr, ptr + 4, ptr, ptr, ptr, 1, 2, 2, 256, None),
        "dwconv7x7_ln: y": lambda: L.msam2_dwconv7x7_ln(ptr, ptr, ptr, ptr, ptr, ptr + 2, 1, 2, 2, 256, None),
        "dwconv7x7_ln: C": lambda: L.msam2_dwconv7x7_ln(ptr, ptr, ptr, ptr, ptr, ptr, 1, 2, 2, 128, None),
        "dwconv7x7_ln: shape": lambda: L.msam2_dwconv7x7_ln(ptr, ptr, ptr, ptr, ptr, ptr, 1, 0, 2, 256, None),
        "hyper_masks: up": lambda: L.msam2_hyper_masks(ptr, ptr + 8, ptr, 1, 4, 16, 32, None),
        "hyper_masks: up by one element": lambda: L.msam2_hyper_masks(ptr, ptr + 2, ptr, 1, 4, 16, 32, None),
        "hyper_masks: C": lambda: L.msam2_hyper_masks(ptr, ptr, ptr, 1, 4, 16, 64, None),
        "im2col3x3s2: x": lambda: L.msam2_im2col3x3s2(ptr + 4, ptr, 1, 2, 2, 4, 40, None),
        "im2col3x3s2: out": lambda: L.msam2_im2col3x3s2(ptr, ptr + 2, 1, 2, 2, 4, 40, None),
        "im2col3x3s2: ld": lambda: L.msam2_im2col3x3s2(ptr, ptr, 1, 2, 2, 4, 36, None),
    }
    for what, call in cases.items():
        rc = call()
        msg = L.msam2_last_error().decode()
        assert rc < 0, (what, rc)
        assert what.split(":")[0] in msg, (what, msg)


def test_refusals_of_the_backward_entries():
    """msam2_dwconv7x7 loads and stores f32x4 on x, taps, bias and y; msam2_hiera_pos_embed_bwd divides by window; window_move /
    window_unpartition_cvt move 16-byte chunks; layernorm_bwd holds at most 1024 columns"""
    from medical_sam2_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    ptr = (ctypes.addressof(buf) + 15) & ~15
    pos = lambda C=4, bh=2, bw=2, h=8, w=8, window=8: L.msam2_hiera_pos_embed_bwd(ptr, ptr, ptr, C, bh, bw, h, w, window, ptr, 1 << 20, None)
    wm = lambda img=ptr, ld=8, win=ptr, fill=None, D=8, es=2: L.msam2_window_move(img, ld, win, fill, 1, 2, 2, 1, D, 2, es, 1, None)
    cvt = lambda img=ptr, ld=8, win=ptr, D=8: L.msam2_window_unpartition_cvt(img, ld, win, 1, 2, 2, 1, D, 2, None)
    cases = {
        "dwconv7x7: x": lambda: L.msam2_dwconv7x7(ptr + 4, ptr, ptr, ptr, 1, 2, 2, 4, 0, None),
        "dwconv7x7: w_tap_major": lambda: L.msam2_dwconv7x7(ptr, ptr + 8, ptr, ptr, 1, 2, 2, 4, 0, None),
        "dwconv7x7: bias": lambda: L.msam2_dwconv7x7(ptr, ptr, ptr + 4, ptr, 1, 2, 2, 4, 1, None),
        "dwconv7x7: y": lambda: L.msam2_dwconv7x7(ptr, ptr, None, ptr + 12, 1, 2, 2, 4, 0, None),
        "dwconv7x7: C": lambda: L.msam2_dwconv7x7(ptr, ptr, ptr, ptr, 1, 2, 2, 6, 0, None),
        "hiera_pos_embed_bwd: window = 0": lambda: pos(window=0),
        "hiera_pos_embed_bwd: window < 0": lambda: pos(window=-8),
        "hiera_pos_embed_bwd: C": lambda: pos(C=0),
        "hiera_pos_embed_bwd: bh": lambda: pos(bh=0),
        "hiera_pos_embed_bwd: bw": lambda: pos(bw=-1),
        "hiera_pos_embed_bwd: h": lambda: pos(h=0),
        "hiera_pos_embed_bwd: w": lambda: pos(w=0),
        "hiera_pos_embed_bwd: h % window": lambda: pos(h=12),
        "window_move: img": lambda: wm(img=ptr + 8),
        "window_move: win": lambda: wm(win=ptr + 4),
        "window_move: fill": lambda: wm(fill=ptr + 2),
        "window_move: row stride": lambda: wm(ld=12),
        "window_move: D": lambda: wm(D=4),
        "window_move: element size": lambda: wm(es=3),
        "window_unpartition_cvt: img": lambda: cvt(img=ptr + 8),
        "window_unpartition_cvt: win": lambda: cvt(win=ptr + 4),
        "window_unpartition_cvt: row stride": lambda: cvt(ld=12),
        "window_unpartition_cvt: D": lambda: cvt(D=4),
        "layernorm_bwd: C": lambda: L.msam2_layernorm_bwd(ptr, 1028, ptr, 0, 1028, ptr, ptr, 1028, ptr, ptr, 1, 1025, 1e-6, None, 0, None),
        "layernorm_bwd: rows": lambda: L.msam2_layernorm_bwd(ptr, 8, ptr, 0, 8, ptr, ptr, 8, ptr, ptr, 0, 8, 1e-6, None, 0, None),
    }
    for what, call in cases.items():
        rc = call()
        msg = L.msam2_last_error().decode()
        assert rc < 0, (what, rc)
        assert what.split(":")[0] in msg, (what, msg)


def test_alignment_refusals_of_the_remaining_entries():
    """the alignment refusals of csrc/elementwise.hip, conv.hip and backward.hip that the two tests above do not reach: every call is valid
    but for ONE pointer or stride, so the refusal is that term's.  The code must be MSAM2_ERR_ARG (-1): a call that got past its argument
    checks fails too on a machine without a GPU, with MSAM2_ERR_LAUNCH (-2) and the entry's name in front of the launch error"""
    from medical_sam2_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    ptr = (ctypes.addressof(buf) + 15) & ~15
    dual = lambda x=ptr, ldx=8, w=ptr, b=ptr, y=ptr, ldy=8, y16=ptr, ldy16=8: L.msam2_layernorm_dual(x, ldx, w, b, y, ldy, y16, ldy16, 1, 8, 1e-6, None)
    shared = lambda g=ptr, bias=ptr, skip=ptr, ln_w=ptr, ln_b=ptr, y=ptr, s16=1: L.msam2_convt2x2_shuffle_shared(g, bias, skip, s16, ln_w, ln_b, y, 1, 1, 1,
                                                                                                                 32, 0, None)
    tt = lambda A=ptr, lda=8, B=ptr, ldb=8: L.msam2_gemm_tt(A, lda, B, ldb, ptr, 8, None, 8, 8, 64, None)
    cases = {
        "layernorm_dual: x": lambda: dual(x=ptr + 8), "layernorm_dual: weight": lambda: dual(w=ptr + 4), "layernorm_dual: bias": lambda: dual(b=ptr + 8),
        "layernorm_dual: y": lambda: dual(y=ptr + 4), "layernorm_dual: y16": lambda: dual(y16=ptr + 4), "layernorm_dual: y16 by one element": lambda: dual(y16=ptr + 2),
        "layernorm_dual: ldx": lambda: dual(ldx=10), "layernorm_dual: ldy": lambda: dual(ldy=9), "layernorm_dual: ldy16": lambda: dual(ldy16=10),
        "convt2x2_shuffle_shared: gemm_out": lambda: shared(g=ptr + 8), "convt2x2_shuffle_shared: bias": lambda: shared(bias=ptr + 4),
        "convt2x2_shuffle_shared: skip": lambda: shared(skip=ptr + 8), "convt2x2_shuffle_shared: fp32 skip": lambda: shared(skip=ptr + 8, s16=0),
        "convt2x2_shuffle_shared: ln_w": lambda: shared(ln_w=ptr + 8), "convt2x2_shuffle_shared: ln_b": lambda: shared(ln_b=ptr + 4),
        "convt2x2_shuffle_shared: y": lambda: shared(y=ptr + 8),
        "convt2x2_shuffle: fp32 skip, gemm_out": lambda: L.msam2_convt2x2_shuffle_f32skip(ptr + 8, ptr, ptr, ptr, ptr, ptr, 1, 1, 1, 32, None),
        "convt2x2_shuffle: fp32 skip, skip": lambda: L.msam2_convt2x2_shuffle_f32skip(ptr, ptr, ptr + 8, ptr, ptr, ptr, 1, 1, 1, 32, None),
        "patch_embed: img": lambda: L.msam2_patch_embed7x7s4(ptr + 4, ptr, ptr, None, ptr, 1, 128, 32, None),
        "patch_embed: w_perm": lambda: L.msam2_patch_embed7x7s4(ptr, ptr + 8, ptr, None, ptr, 1, 128, 32, None),
        "im2col_patch: out": lambda: L.msam2_im2col_patch7x7s4(ptr, ptr + 8, 1, 4, None),
        "select_mask: masks": lambda: L.msam2_select_mask(ptr + 8, ptr, ptr, ptr, ptr, ptr, 1, 4, 1, 0, 1.0, 0.95, None),
        "gemm_tt: A": lambda: tt(A=ptr + 8), "gemm_tt: B": lambda: tt(B=ptr + 2), "gemm_tt: lda": lambda: tt(lda=12), "gemm_tt: ldb": lambda: tt(ldb=12),
    }
    for what, call in cases.items():
        rc = call()
        msg = L.msam2_last_error().decode()
        assert rc == -1, (what, rc, msg)
        assert what.split(":")[0] in msg, (what, msg)


def test_backward_wrappers_refuse_strided_and_wrong_typed_tensors():
    """backward.act_backward, layernorm_backward, dwconv7x7 and backward_encoder.maxpool2x2_backward hand raw pointers to the library (host
    tensors: nothing is launched)"""
    import medical_sam2_amd.backward as bwd
    import medical_sam2_amd.backward_encoder as be
    import medical_sam2_amd.ops as ops
    op16, f64 = ops.OP16, torch.float64
    x, g = torch.zeros(4, 8), torch.zeros(8)
    taps = torch.zeros(49, 8)
    bad = {
        "act_backward: float64 pre": lambda: bwd.act_backward(torch.zeros(8, dtype=f64), torch.zeros(8), 1),
        "act_backward: float64 dy": lambda: bwd.act_backward(torch.zeros(8), torch.zeros(8, dtype=f64), 1),
        "act_backward: int dy": lambda: bwd.act_backward(torch.zeros(8, dtype=op16), torch.zeros(8, dtype=torch.int16), 2),
        "act_backward: strided": lambda: bwd.act_backward(torch.zeros(8, 2)[:, 0], torch.zeros(8), 1),
        "layernorm_backward: 16-bit gamma": lambda: bwd.layernorm_backward(x, g.to(op16), x, 1e-6),
        "layernorm_backward: strided gamma": lambda: bwd.layernorm_backward(x, torch.zeros(16)[::2], x, 1e-6),
        "layernorm_backward: short gamma": lambda: bwd.layernorm_backward(x, torch.zeros(4), x, 1e-6),
        "layernorm_backward: 2-d gamma": lambda: bwd.layernorm_backward(x, torch.zeros(1, 8), x, 1e-6),
        "layernorm_backward: float64 dy": lambda: bwd.layernorm_backward(x, g, x.double(), 1e-6),
        "dwconv7x7: 16-bit taps": lambda: bwd.dwconv7x7(x, taps.to(op16), None, 1, 2, 2),
        "dwconv7x7: strided taps": lambda: bwd.dwconv7x7(x, torch.zeros(8, 49).t(), None, 1, 2, 2),
        "dwconv7x7: 16-bit bias": lambda: bwd.dwconv7x7(x, taps, g.to(op16), 1, 2, 2),
        "dwconv7x7: strided bias": lambda: bwd.dwconv7x7(x, taps, torch.zeros(16)[::2], 1, 2, 2),
        "dwconv7x7: short bias": lambda: bwd.dwconv7x7(x, taps, torch.zeros(4), 1, 2, 2),
        "maxpool2x2_backward: column-strided x": lambda: be.maxpool2x2_backward(torch.zeros(4, 16)[:, ::2], torch.zeros(1, 8), 1, 2, 2),
        "maxpool2x2_backward: x rows": lambda: be.maxpool2x2_backward(torch.zeros(5, 8), torch.zeros(1, 8), 1, 2, 2),
        "maxpool2x2_backward: dy rows": lambda: be.maxpool2x2_backward(x, torch.zeros(2, 8), 1, 2, 2),
    }
    for what, call in bad.items():
        with pytest.raises((ValueError, TypeError)):
            call()


def test_wrappers_refuse_strided_and_wrong_typed_tensors():
    """conv3x3s2_ln_gelu, space_to_depth, obj_ptr_mix_ and hyper_masks hand raw pointers to the library: a strided view or another dtype must
    raise before the call (host tensors: nothing is launched)"""
    import medical_sam2_amd.ops as ops
    op16 = ops.OP16
    w1, v4 = torch.zeros(4, 1, 3, 3), torch.zeros(4)
    w4, v16 = torch.zeros(16, 4, 3, 3), torch.zeros(16)
    bad = {
        "conv: strided x": lambda: ops.conv3x3s2_ln_gelu(torch.zeros(16, 2)[:, :1], 1, 4, 4, w1, v4, v4, v4),
        "conv: 16-bit x for cin = 1": lambda: ops.conv3x3s2_ln_gelu(torch.zeros(16, 1, dtype=op16), 1, 4, 4, w1, v4, v4, v4),
        "conv: fp32 x for cin = 4": lambda: ops.conv3x3s2_ln_gelu(torch.zeros(16, 4), 1, 4, 4, w4, v16, v16, v16),
        "conv: float64 x": lambda: ops.conv3x3s2_ln_gelu(torch.zeros(16, 1, dtype=torch.float64), 1, 4, 4, w1, v4, v4, v4),
        "conv: wrong size": lambda: ops.conv3x3s2_ln_gelu(torch.zeros(15, 1), 1, 4, 4, w1, v4, v4, v4),
        "conv: strided weight": lambda: ops.conv3x3s2_ln_gelu(torch.zeros(16, 1), 1, 4, 4, torch.zeros(4, 1, 3, 6)[..., ::2], v4, v4, v4),
        "conv: 16-bit bias": lambda: ops.conv3x3s2_ln_gelu(torch.zeros(16, 1), 1, 4, 4, w1, v4.to(op16), v4, v4),
        "space_to_depth: strided": lambda: ops.space_to_depth(torch.zeros(16, 2)[:, :1], 1, 4, 4, 2),
        "space_to_depth: float64": lambda: ops.space_to_depth(torch.zeros(16, 1, dtype=torch.float64), 1, 4, 4, 2),
        "space_to_depth: wrong size": lambda: ops.space_to_depth(torch.zeros(12, 1), 1, 4, 4, 2),
        "obj_ptr_mix: strided ptr": lambda: ops.obj_ptr_mix_(torch.zeros(2, 8)[:, ::2], torch.zeros(2), torch.zeros(4)),
        "obj_ptr_mix: float64 obj": lambda: ops.obj_ptr_mix_(torch.zeros(2, 4), torch.zeros(2, dtype=torch.float64), torch.zeros(4)),
        "obj_ptr_mix: strided obj": lambda: ops.obj_ptr_mix_(torch.zeros(2, 4), torch.zeros(4)[::2], torch.zeros(4)),
        "obj_ptr_mix: short no_obj_ptr": lambda: ops.obj_ptr_mix_(torch.zeros(2, 4), torch.zeros(2), torch.zeros(3)),
        "obj_ptr_mix: 16-bit ptr": lambda: ops.obj_ptr_mix_(torch.zeros(2, 4, dtype=op16), torch.zeros(2), torch.zeros(4)),
        "hyper_masks: fp32 up": lambda: ops.hyper_masks(torch.zeros(1, 4, 32), torch.zeros(16, 32), 1, 16),
        "hyper_masks: strided up": lambda: ops.hyper_masks(torch.zeros(1, 4, 32), torch.zeros(16, 64, dtype=op16)[:, :32], 1, 16),
        "hyper_masks: 16-bit hyper": lambda: ops.hyper_masks(torch.zeros(1, 4, 32, dtype=op16), torch.zeros(16, 32, dtype=op16), 1, 16),
        "hyper_masks: wrong size": lambda: ops.hyper_masks(torch.zeros(1, 4, 32), torch.zeros(15, 32, dtype=op16), 1, 16),
    }
    for what, call in bad.items():
        with pytest.raises((ValueError, TypeError)):
            call()
