"""attn_winproj_kernel (GPU): the qkv projection inside the window-attention kernel of Hiera stages 1-2 (ops.window_qkv_attention)
against the fp32 oracle that rounds q | k | v where the two-launch path rounds them, against that path itself, and at module level.

Bound: the window-attention family's own, close(out, ref, 0.02, 0.01).  A wrong k order or window map misses it by orders of magnitude.
"""
import os as _os
import sys as _sys

import pytest
import torch

_sys.path.insert(0, _os.path.dirname(_os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

from oracle import sam2_oracle as O  # noqa: E402

DEV = "cuda"
D = 96

# (B, H, W, dim, heads, ws, pool)
CASES = [(2, 16, 16, 96, 1, 8, False),    # block 0 form
         (1, 16, 16, 96, 2, 8, True),     # block 1 form
         (1, 16, 16, 192, 2, 4, False),   # block 2 form
         (1, 16, 16, 192, 4, 4, True),    # block 3 form
         (1, 8, 8, 192, 2, 4, False),     # 64 tokens, fewer than one pass: the ragged path
         (3, 32, 32, 96, 1, 8, False)]    # 48 units = 6 passes of 8 waves
# several passes PER WORKGROUP (the launch caps the grid at 256 workgroups of 8 waves, one unit per wave): the persistent loop over
# resident weights and, at dim 192, the weight ring running on across passes; 2560 units = 320 passes, the last round ragged
MULTIPASS = [(5, 256, 128, 96, 1, 8, False), (5, 128, 128, 192, 2, 4, True)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import medical_sam2_amd.ops as ops_mod
    return ops_mod


def bf(x):
    import medical_sam2_amd.ops as _o
    return x.to(_o.OP16)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def close(a, b, atol, rtol=0.0, what=""):
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    err = (a - b).abs()
    lim = atol + rtol * b.abs()
    bad = (err > lim)
    frac = (err / lim).max().item()
    print(f"{what}: max err {err.max().item():.4g}, {frac:.3f} of the limit")
    assert not bad.any(), f"{what}: max err {err.max().item():.4g} (limit {atol}+{rtol}*|ref|), {bad.sum().item()} bad of {bad.numel()}"


def _attn_ref(q, k, v):
    return O.softmax_attention(q.double(), k.double(), v.double()).float()


_INPUTS = {}


def inputs(B, H, W, dim, heads, ws, pool):
    """(xn, W, b, ref) of a case, built once and shared by the tests that need it"""
    key = (B, H, W, dim, heads, ws, pool)
    if key in _INPUTS:
        return _INPUTS[key]
    T, dim_out = B * H * W, heads * D
    xn = bf(rnd(T, dim, seed=7))
    w = bf(rnd(3 * dim_out, dim, seed=8, scale=dim ** -0.5))
    b = rnd(3 * dim_out, seed=9, scale=0.5)
    qkv = bf(xn.float() @ w.float().T + b)                     # the rounding point of the two-launch path
    win, _ = O.to_windows(qkv.float().reshape(B, H, W, 3 * dim_out), ws)
    Bw = win.shape[0]
    t = win.reshape(Bw, ws * ws, 3, heads, D)
    q, k, v = t[:, :, 0], t[:, :, 1], t[:, :, 2]
    wq = ws
    if pool:
        q = O.maxpool2x2_nhwc(q.reshape(Bw, ws, ws, dim_out))
        wq = ws // 2
        q = q.reshape(Bw, wq * wq, heads, D)
    o = _attn_ref(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)).transpose(1, 2).reshape(Bw, wq, wq, dim_out)
    Hq, Wq = (H // 2, W // 2) if pool else (H, W)
    ref = O.from_windows(o, wq, (Hq, Wq), (Hq, Wq)).reshape(B * Hq * Wq, dim_out)
    _INPUTS[key] = (xn, w, b, ref)
    return _INPUTS[key]


def old_pair(ops, xn, w, b, B, H, W, heads, ws, pool):
    qkv = ops.gemm(xn, w, b)
    qp = ops.maxpool2x2(qkv[:, :heads * D], B, H, W) if pool else None
    return ops.window_attention(qkv, B, H, W, heads, ws, b, q_pooled=qp)


@pytest.mark.parametrize("B,H,W,dim,heads,ws,pool", CASES + MULTIPASS)
def test_fused_vs_oracle_and_old_pair(ops, B, H, W, dim, heads, ws, pool):
    assert ops.window_qkv_attention_supported(dim, heads * D, heads, ws, pool, H, W)
    xn, w, b, ref = inputs(B, H, W, dim, heads, ws, pool)
    dx, dw, db = xn.to(DEV), w.to(DEV), b.to(DEV)
    out = ops.window_qkv_attention(dx, dw, db, B, H, W, heads, ws, pool)
    old = old_pair(ops, dx, dw, db, B, H, W, heads, ws, pool)
    print(f"fused vs old pair: max |diff| {(out.float() - old.float()).abs().max().item():.4g}")
    close(old, ref, 0.02, 0.01, "gemm + window_attention")
    close(out, ref, 0.02, 0.01, "window_qkv_attention")


@pytest.mark.parametrize("dim,heads,ws,pool", [(96, 1, 8, False), (96, 2, 8, True), (192, 2, 4, False), (192, 4, 4, True)])
def test_batch_independence_bitwise(ops, dim, heads, ws, pool):
    B, H, W = 3, 16, 16
    xn = bf(rnd(B * H * W, dim, seed=7)).to(DEV)
    w = bf(rnd(3 * heads * D, dim, seed=8, scale=dim ** -0.5)).to(DEV)
    b = rnd(3 * heads * D, seed=9, scale=0.5).to(DEV)
    full = ops.window_qkv_attention(xn, w, b, B, H, W, heads, ws, pool)
    one = ops.window_qkv_attention(xn[H * W:2 * H * W].contiguous(), w, b, 1, H, W, heads, ws, pool)
    n = one.shape[0]
    assert torch.equal(full[n:2 * n], one)


def test_gate(ops):
    assert not ops.window_qkv_attention_supported(96, 96, 1, 8, False, 20, 20)      # windows do not tile
    assert not ops.window_qkv_attention_supported(96, 64, 1, 8, False, 16, 16)      # head dim 64
    assert not ops.window_qkv_attention_supported(384, 384, 4, 8, False, 16, 16)    # dim 384
    assert not ops.window_qkv_attention_supported(384, 768, 8, 4, True, 16, 16)
    xn = bf(rnd(400, 96, seed=1)).to(DEV)
    with pytest.raises(RuntimeError):
        ops.window_qkv_attention(xn, bf(rnd(288, 96, seed=2)).to(DEV), rnd(288, seed=3).to(DEV), 1, 20, 20, 1, 8, False)


def _block(dim, dim_out, heads, ws, pool, seed):
    from medical_sam2_amd.modeling.encoder import MultiScaleBlock
    torch.manual_seed(seed)
    blk = MultiScaleBlock(dim=dim, dim_out=dim_out, num_heads=heads, q_stride=(2, 2) if pool else None, window_size=ws)
    return blk.to(DEV).eval()


def _run(blk, t, B, H, W, fused, switch, monkeypatch):
    import medical_sam2_amd.modeling.encoder as enc
    monkeypatch.setattr(enc, "_FUSED_QKV_ATTN", switch)
    with torch.no_grad():
        return blk.run(t, B, H, W, fused_qkv_attn=fused)[0] if fused is not None else blk.run(t, B, H, W)[0]


@pytest.mark.parametrize("dim,dim_out,heads,ws,pool", [(96, 96, 1, 8, False), (96, 192, 2, 8, True), (192, 192, 2, 4, False),
                                                      (192, 384, 4, 4, True)])
def test_block_fused_vs_switched_off(ops, monkeypatch, dim, dim_out, heads, ws, pool):
    """one MultiScaleBlock of each form at 32 x 32 tokens: the trunk's call with the fused kernel vs. switched off; the training forward's
    call form (no opt-in) must not reach the fused kernel and gives the bits of the two-launch path"""
    B, H, W = 2, 32, 32
    blk = _block(dim, dim_out, heads, ws, pool, 3)
    t = rnd(B * H * W, dim, seed=5).to(DEV)
    off = _run(blk, t, B, H, W, True, False, monkeypatch)
    calls = []
    real = ops.window_qkv_attention
    monkeypatch.setattr(ops, "window_qkv_attention", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    on = _run(blk, t, B, H, W, True, True, monkeypatch)
    assert calls, "the trunk's call did not take the fused kernel"
    close(on, off, 0.02, 0.01, "block, fused vs switched off")
    del calls[:]
    saved_path = _run(blk, t, B, H, W, None, True, monkeypatch)
    assert not calls, "the training forward's call took the fused kernel"
    assert torch.equal(saved_path, off)


def test_block_unsupported_form_takes_the_old_path(ops, monkeypatch):
    """20 x 20 tokens with 8 x 8 windows (padded tokens): the gate says no and the block gives the switched-off tensor"""
    B, H, W = 1, 20, 20
    blk = _block(96, 96, 1, 8, False, 4)
    t = rnd(B * H * W, 96, seed=6).to(DEV)
    off = _run(blk, t, B, H, W, True, False, monkeypatch)
    on = _run(blk, t, B, H, W, True, True, monkeypatch)
    assert torch.equal(on, off)


def test_training_forward_keeps_the_two_launch_path(ops, monkeypatch):
    """backward_encoder.image_encoder_forward_saved and the frozen-encoder forwards of the training code never take the fused call: same
    bits with the switch on or off"""
    import medical_sam2_amd.build_sam as bs
    import medical_sam2_amd.modeling.encoder as enc
    import medical_sam2_amd.weights as wts
    from medical_sam2_amd.backward_encoder import image_encoder_forward_saved
    m = bs.build_sam2("sam2_hiera_t", device="cpu", hydra_overrides_extra=["++model.image_size=256"])
    m.load_state_dict(wts.init_weights("hiera_t", 0), strict=True)
    m = m.to(DEV).eval()
    img = rnd(1, 3, 256, 256, seed=11).to(DEV)
    calls = []
    real = ops.window_qkv_attention
    monkeypatch.setattr(ops, "window_qkv_attention", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.no_grad():
        monkeypatch.setattr(enc, "_FUSED_QKV_ATTN", True)
        on, _ = image_encoder_forward_saved(m, img)
        assert not calls
        with enc.two_launch_qkv_attention():                   # the frozen-encoder forward of training.py / training_3d.py / autograd.py
            kept = m.forward_image(img)
        assert not calls
        fwd = m.forward_image(img)                             # the inference trunk takes it: stages 1-2 of hiera_t at 64 x 64 tokens
        assert len(calls) == 4
        monkeypatch.setattr(enc, "_FUSED_QKV_ATTN", False)
        off, _ = image_encoder_forward_saved(m, img)
        off_fwd = m.forward_image(img)
    assert torch.equal(on["vision_features"], off["vision_features"])
    assert torch.equal(kept["vision_features"], off_fwd["vision_features"])
    assert fwd["vision_features"].shape == on["vision_features"].shape
