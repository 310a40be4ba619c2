"""mlp_fused_kernel's PROJ form (GPU): the attention output projection inside the one-kernel MLP of Hiera stages 1-2
(ops.proj_ln_mlp_residual), with the optional 16-bit rows and the next block's norm1 rows, against the fp32 oracle on the same 16-bit
weights, against the launches it replaces (ops.gemm(residual=...) + ops.ln_mlp_residual [+ ops.layernorm]) and at block / trunk level.

Bounds: those of tests/test_kernels_gpu.py::test_ln_mlp_residual_fused for the same two comparisons -- the rounding points are the same
(normalised rows and hidden activation in the 16-bit type), only the summation order of the proj sum and of the statistics differs.
"""
import os as _os
import sys as _sys

import pytest
import torch

_sys.path.insert(0, _os.path.dirname(_os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

from helpers import btol  # noqa: E402
from oracle import sam2_oracle as O  # noqa: E402

DEV = "cuda"
PASS = {96: 512, 192: 256}          # tokens of one pass of a workgroup (8 waves x TB blocks of 32)


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
    print(f"{what}: max err {err.max().item():.4g}, {(err / lim).max().item():.3f} of the limit")
    assert not bad.any(), f"{what}: max err {err.max().item():.4g} (limit {atol}+{rtol}*|ref|), {bad.sum().item()} bad of {bad.numel()}"


_PARAMS = {}
_INPUTS = {}


def params(dim):
    """weights of one block half, built once per width: 16-bit values held in fp32 (the oracle's view) -- never modified"""
    if dim not in _PARAMS:
        _PARAMS[dim] = {
            "p.weight": bf(rnd(dim, dim, seed=11) / dim ** 0.5).float(), "p.bias": 0.1 * rnd(dim, seed=12),
            "n.weight": 1 + 0.1 * rnd(dim, seed=2), "n.bias": 0.1 * rnd(dim, seed=3),
            "m.layers.0.weight": bf(rnd(4 * dim, dim, seed=4) / dim ** 0.5).float(), "m.layers.0.bias": 0.1 * rnd(4 * dim, seed=5),
            "m.layers.1.weight": bf(rnd(dim, 4 * dim, seed=6) / (4 * dim) ** 0.5).float(), "m.layers.1.bias": 0.1 * rnd(dim, seed=7),
            "nn.weight": 1 + 0.1 * rnd(dim, seed=8), "nn.bias": 0.1 * rnd(dim, seed=9)}
    return _PARAMS[dim]


def inputs(dim, T, shortcut):
    """(o, res, ref) of a case, built once.  shortcut False: res is the block's input x, the map o was computed from (blocks 0 and 2);
    True: a distinct map of another scale, as block 1's pooled projection is"""
    key = (dim, T, shortcut)
    if key not in _INPUTS:
        P = params(dim)
        x = rnd(T, dim, seed=1, scale=1.5) + 0.3
        o = bf(0.5 * x + rnd(T, dim, seed=21))
        res = (0.7 * rnd(T, dim, seed=22) - 0.2) if shortcut else x
        x1 = res + O.lin(P, "p", o.float())
        ref = x1 + O.lin(P, "m.layers.1", O.gelu(O.lin(P, "m.layers.0", O.lnorm(P, "n", x1, 1e-6))))
        _INPUTS[key] = (o, res, ref)
    return _INPUTS[key]


def dev_weights(ops, dim):
    P = params(dim)
    d = lambda t: t.to(DEV)
    w1, w2 = bf(P["m.layers.0.weight"]).to(DEV), bf(P["m.layers.1.weight"]).to(DEV)
    return dict(wp=bf(P["p.weight"]).to(DEV), bp=d(P["p.bias"]), lw=d(P["n.weight"]), lb=d(P["n.bias"]), w1=w1, b1=d(P["m.layers.0.bias"]),
                w1p=ops.mlp_fused_permute_w1(w1), w2p=ops.mlp_fused_permute_w2(w2), b2=d(P["m.layers.1.bias"]),
                nw=d(P["nn.weight"]), nb=d(P["nn.bias"]))


def fused(ops, Wd, o, res, also16=False, next_ln=False):
    return ops.proj_ln_mlp_residual(o, Wd["wp"], Wd["bp"], res, Wd["lw"], Wd["lb"], 1e-6, Wd["w1p"], Wd["b1"], Wd["w2p"], Wd["b2"], also16=also16,
                                    next_ln=(Wd["nw"], Wd["nb"], 1e-6) if next_ln else None)


def launches(ops, Wd, o, res):
    x1 = ops.gemm(o, Wd["wp"], Wd["bp"], residual=res, out_dtype=torch.float32)
    return ops.ln_mlp_residual(x1, Wd["lw"], Wd["lb"], 1e-6, Wd["w1"], Wd["b1"], Wd["w2p"], Wd["b2"])


def token_counts(dim):
    p = PASS[dim]
    # the last one wraps the grid (256 workgroups): a workgroup runs a second pass, the dim-192 ring carries on across passes with its Wp step
    return [1, 31, p - 1, p + 1, 3 * p + 17, 256 * p + p // 2 + 5]


CASES = [(dim, T, sc) for dim in (96, 192) for T in token_counts(dim) for sc in (False, True)]


@pytest.mark.parametrize("dim,T,shortcut", CASES)
def test_kernel_vs_oracle_and_launches(ops, dim, T, shortcut):
    assert ops.proj_ln_mlp_residual_supported(dim)
    o, res, ref = inputs(dim, T, shortcut)
    Wd = dev_weights(ops, dim)
    do, dres = o.to(DEV), res.to(DEV)
    out, o16, xn = fused(ops, Wd, do, dres)
    assert out.shape == res.shape and out.dtype == torch.float32 and o16 is None and xn is None
    close(out, ref, btol(6e-3), btol(4e-3), "proj + LN + MLP in one kernel vs oracle")
    close(out, launches(ops, Wd, do, dres), btol(4e-3), btol(2e-3), "one kernel vs gemm + ln_mlp_residual")


@pytest.mark.parametrize("dim", [96, 192])
def test_in_place(ops, dim):
    """out == res is allowed at the C ABI (nothing is re-read in the store): same bits as out of place"""
    from medical_sam2_amd._lib import check, lib
    T = 3 * PASS[dim] + 17
    o, res, _ = inputs(dim, T, False)
    Wd = dev_weights(ops, dim)
    do, dres = o.to(DEV), res.to(DEV)
    out, _, _ = fused(ops, Wd, do, dres)
    buf = dres.clone()
    p = lambda t: t.data_ptr()
    check(lib().msam2_proj_ln_mlp_residual_fwd(p(do), p(Wd["wp"]), p(Wd["bp"]), p(buf), T, dim, p(Wd["lw"]), p(Wd["lb"]), 1e-6, p(Wd["w1p"]), p(Wd["b1"]),
                                               p(Wd["w2p"]), p(Wd["b2"]), p(buf), None, None, None, 0.0, None, torch.cuda.current_stream().cuda_stream))
    assert torch.equal(buf, out)


@pytest.mark.parametrize("dim", [96, 192])
def test_side_outputs(ops, dim):
    """out16 = the fp32 rows rounded, bit for bit; the next-norm rows = ops.layernorm of the kernel's own fp32 rows within one unit in the
    last place of the operand type; the fp32 rows do not depend on which side outputs are asked for"""
    T = 3 * PASS[dim] + 17
    o, res, _ = inputs(dim, T, True)
    Wd = dev_weights(ops, dim)
    do, dres = o.to(DEV), res.to(DEV)
    plain, _, _ = fused(ops, Wd, do, dres)
    for also16, nxt in [(True, False), (False, True), (True, True)]:
        out, o16, xn = fused(ops, Wd, do, dres, also16=also16, next_ln=nxt)
        assert torch.equal(out, plain), (also16, nxt)
        if also16:
            assert o16.dtype == ops.OP16 and torch.equal(o16, out.to(ops.OP16))
        if nxt:
            want = ops.layernorm(out, Wd["nw"], Wd["nb"], 1e-6)
            assert xn.dtype == ops.OP16 and xn.shape == want.shape
            # one unit in the last place: the bit patterns, mapped to one monotonic integer line, are neighbours
            line = lambda v: (lambda i: torch.where(i < 0, -(i & 0x7FFF), i))(v.view(torch.int16).int())
            bad = (line(xn) - line(want)).abs() > 1
            rows = bad.any(dim=1).nonzero().flatten().tolist()
            print(f"dim {dim}: {int((xn != want).sum())} of {want.numel()} next-norm values differ from ops.layernorm by one ulp, {len(rows)} rows beyond")
            assert not rows, f"next-norm rows beyond one ulp of ops.layernorm: {rows[:20]}"


@pytest.mark.parametrize("dim", [96, 192])
def test_batch_independence_bitwise(ops, dim):
    n = 1024 + 32                                              # tokens of one slice: a pass boundary falls inside every slice
    o, res, _ = inputs(dim, 3 * n, True)
    Wd = dev_weights(ops, dim)
    do, dres = o.to(DEV), res.to(DEV)
    full = fused(ops, Wd, do, dres, also16=True, next_ln=True)
    one = fused(ops, Wd, do[n:2 * n].contiguous(), dres[n:2 * n].contiguous(), also16=True, next_ln=True)
    for f, s in zip(full, one):
        assert torch.equal(f[n:2 * n], s)


def test_gate(ops):
    assert not ops.proj_ln_mlp_residual_supported(384) and not ops.proj_ln_mlp_residual_supported(112)
    Wd = dev_weights(ops, 96)
    o, res, _ = inputs(96, 31, False)
    with pytest.raises(RuntimeError):                          # dim 384 is not built: an error, no other path
        ops.proj_ln_mlp_residual(bf(rnd(31, 384)).to(DEV), bf(rnd(384, 384)).to(DEV), rnd(384).to(DEV), rnd(31, 384).to(DEV), rnd(384).to(DEV),
                                 rnd(384).to(DEV), 1e-6, bf(rnd(1536, 384)).to(DEV), rnd(1536).to(DEV), bf(rnd(384, 1536)).to(DEV), rnd(384).to(DEV))
    with pytest.raises(ValueError):                            # o of another width
        fused(ops, Wd, bf(rnd(31, 192)).to(DEV), res.to(DEV))


# ---- block level -------------------------------------------------------------------------------------------------------------------
def _block(dim, dim_out, heads, ws, pool, seed, act=torch.nn.GELU):
    from medical_sam2_amd.modeling.encoder import MultiScaleBlock
    torch.manual_seed(seed)
    blk = MultiScaleBlock(dim=dim, dim_out=dim_out, num_heads=heads, q_stride=(2, 2) if pool else None, window_size=ws, act_layer=act)
    return blk.to(DEV).eval()


def _run(blk, t, B, H, W, switch, monkeypatch, request_it=True, next_norm=None):
    import medical_sam2_amd.modeling.encoder as enc
    monkeypatch.setattr(enc, "_FUSED_PROJ_MLP", switch)
    with torch.no_grad():
        out = blk.run(t, B, H, W, emit16=True, fused_qkv_attn=request_it, fused_gemm_ln=request_it, next_norm=next_norm)[0]
    return out, blk.out16, blk.next_xn


def _count(ops, monkeypatch):
    calls = []
    real = ops.proj_ln_mlp_residual
    monkeypatch.setattr(ops, "proj_ln_mlp_residual", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


# the three stage 1-2 block forms of hiera_s at 32 x 32 tokens per slice behind the block (the pooling form starts from 64 x 64)
@pytest.mark.parametrize("dim,dim_out,heads,ws,pool,side", [(96, 96, 1, 8, False, 32), (96, 192, 2, 8, True, 64), (192, 192, 2, 4, False, 32)])
def test_block_fused_vs_switched_off(ops, monkeypatch, dim, dim_out, heads, ws, pool, side):
    B = 2
    blk = _block(dim, dim_out, heads, ws, pool, 3)
    t = rnd(B * side * side, dim, seed=5).to(DEV)
    nn_ = (1 + 0.1 * rnd(dim_out, seed=8).to(DEV), 0.1 * rnd(dim_out, seed=9).to(DEV), 1e-6)
    off, off16, off_xn = _run(blk, t, B, side, side, False, monkeypatch, next_norm=nn_)
    assert off_xn is None                                      # today's launches leave the next norm1 to the next block
    calls = _count(ops, monkeypatch)
    import medical_sam2_amd.modeling.encoder as enc
    monkeypatch.setattr(enc, "_FUSED_PROJ_MLP_NEXT_LN_DIMS", frozenset())          # the norm1 rows have a list of their own
    on, on16, on_xn = _run(blk, t, B, side, side, True, monkeypatch, next_norm=nn_)
    assert len(calls) == 1 and on_xn is None, "the trunk's call did not take the fused kernel"
    close(on, off, btol(4e-3), btol(2e-3), "block, proj in the MLP kernel vs switched off")
    assert torch.equal(on16, on.to(ops.OP16))
    monkeypatch.setattr(enc, "_FUSED_PROJ_MLP_NEXT_LN_DIMS", frozenset((dim_out,)))
    on2, _, on_xn = _run(blk, t, B, side, side, True, monkeypatch, next_norm=nn_)
    assert torch.equal(on2, on) and on_xn is not None and on_xn.shape == on.shape and on_xn.dtype == ops.OP16
    del calls[:]
    plain, _, plain_xn = _run(blk, t, B, side, side, True, monkeypatch, request_it=False)   # the training forwards' call form
    off_plain, _, _ = _run(blk, t, B, side, side, False, monkeypatch, request_it=False)
    assert not calls and plain_xn is None and torch.equal(plain, off_plain)


@pytest.mark.parametrize("form", ["dim384", "width", "relu"])
def test_block_refused_forms_take_todays_path(ops, monkeypatch, form):
    """dim 384, a padded head width (width != dim_out: hiera_b+'s 56-channel heads) and a non-GELU MLP: refused, today's launches, same bits"""
    dim, heads, ws, act = {"dim384": (384, 4, 8, torch.nn.GELU), "width": (112, 2, 8, torch.nn.GELU), "relu": (96, 1, 8, torch.nn.ReLU)}[form]
    B, side = 1, 32
    blk = _block(dim, dim, heads, ws, False, 4, act=act)
    t = rnd(B * side * side, dim, seed=6).to(DEV)
    off, _, _ = _run(blk, t, B, side, side, False, monkeypatch)
    calls = _count(ops, monkeypatch)
    on, _, _ = _run(blk, t, B, side, side, True, monkeypatch)
    assert not calls and torch.equal(on, off)


def test_trunk_takes_it_three_times_and_training_forward_never(ops, monkeypatch):
    """hiera_s at 256 x 256 (64 x 64 and 32 x 32 tokens in stages 1-2): Hiera.forward takes the call in blocks 0, 1, 2; inside
    frozen_forward_image it is never taken and the features have the bits of the switched-off path"""
    import medical_sam2_amd.build_sam as bs
    import medical_sam2_amd.modeling.encoder as enc
    import medical_sam2_amd.weights as wts
    m = bs.build_sam2("sam2_hiera_s", device="cpu", hydra_overrides_extra=["++model.image_size=256"])
    m.load_state_dict(wts.init_weights("hiera_s", 0), strict=True)
    m = m.to(DEV).eval()
    img = rnd(1, 3, 256, 256, seed=11).to(DEV)
    calls = _count(ops, monkeypatch)
    with torch.no_grad():
        monkeypatch.setattr(enc, "_FUSED_PROJ_MLP", True)
        fwd = m.forward_image(img)
        assert len(calls) == 3
        del calls[:]
        kept = enc.frozen_forward_image(m, img)
        assert not calls
        monkeypatch.setattr(enc, "_FUSED_PROJ_MLP", False)
        kept_off = enc.frozen_forward_image(m, img)
        off = m.forward_image(img)
        assert not calls
    assert torch.equal(kept["vision_features"], kept_off["vision_features"])
    for a, b in zip(kept["backbone_fpn"], kept_off["backbone_fpn"]):
        assert torch.equal(a, b)
    # 16-bit outputs move by an ulp with the proj sum's order; the bound is the FPN's own 16-bit output step on |features| ~ 1
    d = (fwd["vision_features"].float() - off["vision_features"].float()).abs()
    print(f"trunk on vs off: max |d| {d.max().item():.4g}, mean {d.mean().item():.4g}")
    assert fwd["vision_features"].shape == off["vision_features"].shape and torch.isfinite(fwd["vision_features"].float()).all()
