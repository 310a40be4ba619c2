"""Variant matrix of the patch embed, implicit-GEMM convolution and token-head kernels (GPU): patch_embed_kernel<NT,NTOK> (12
instantiations), im2col_patch_kernel and token_mlp3_kernel (csrc/conv.hip) and conv3x3s2_mfma_kernel<CIN,COUT,WR,WC,SKINNY> (5,
csrc/conv_mfma.hip), every instantiation reached on purpose, in the style of tests/test_rowtile_variants_gpu.py:
  * each case names the instantiation it must reach; torch.profiler asserts that exactly that one ran (conv_cases' tables are compared
    with literal lists in tests/test_conv_cases_cpu.py);
  * every operand lies between NaN guards or in NaN padding (the packed conv weight with ldw = KP + 8, hs as a strided view), vectors have
    their exact length and are followed by NaN, outputs lie in sentinel-filled buffers whose sentinels must be bit-identical afterwards;
  * pass 1, exact: operands built so that the output is known to the bit (conv_cases), compared with == against float64 values;
  * pass 2, random: float64 references of the operand-rounded inputs, inside error_bound() of tests/test_gemm_variants_gpu.py (the conv
    through pointwise_bounds.ln_tail and act_store as tests/test_mask_ds_fused_gpu.py does, plus the bits of the three launches; the token
    heads composed over the three layers).  The worst ratio to every limit is printed ("RATIO ...");
  * token order of the patch embedding: two images exchanged in the batch give the same rows, exchanged, bit for bit.
The C entries are called directly where the ops wrapper cannot express a case (an output inside a sentinel buffer, strided hs).  The
16-bit type is ops.OP16 throughout; the file runs once more in a child process on the bf16 library.
"""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_cases as CC  # noqa: E402
import pointwise_bounds as PB  # noqa: E402
import test_mask_ds_fused_gpu as MD  # noqa: E402
import test_rowtile_variants_gpu as RV  # noqa: E402
from helpers import ROOT, SENT32, Canvas, Flat, nan_guarded, nan_padded, op16_is_fp16, reached, same_bits, within  # noqa: E402
from test_gemm_variants_gpu import error_bound  # noqa: E402

DEV = "cuda"
F32 = torch.float32
bits_equal, inside = RV.bits_equal, RV.inside


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import medical_sam2_amd.ops as ops_mod
    return ops_mod


@pytest.fixture(scope="module")
def L(ops):
    return ops.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def p(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. patch embedding
class PatchEmbedLaunch:
    """msam2_patch_embed7x7s4 on the operands X: image, w_perm and pos between NaN guards, bias exactly E floats followed by NaN, the
    output in a Flat"""

    def __init__(self, ops, X, with_pos):
        self.B, self.S, self.E = X["B"], X["S"], X["E"]
        self.img = nan_guarded(X["img"].to(F32))
        self.wp = nan_guarded(X["wp"].to(ops.OP16))
        self.bias = nan_guarded(X["bias"].to(F32))
        self.pos = nan_guarded(X["pos"].to(F32)) if with_pos else None
        self.out = Flat((self.B * (self.S // 4) ** 2, self.E), F32)

    def call(self, L):
        return L.msam2_patch_embed7x7s4(p(self.img), p(self.wp), p(self.bias), p(self.pos), p(self.out.view), self.B, self.S, self.E, stream())

    def run(self, L, expect=None):
        if expect is not None:
            reached(L, expect, "patch_embed_kernel", [lambda: self.call(L)])
        else:
            assert self.call(L) == 0, L.msam2_last_error().decode()
        torch.cuda.synchronize()
        assert self.out.sentinels_intact(), "wrote before or behind the output"
        return self.out.view


@pytest.mark.parametrize("c", CC.PE_CASES, ids=CC.pe_id)
def test_patch_embed_variant(ops, L, c):
    cid = CC.pe_id(c)
    # ---- pass 1: exact, and the kernel by name; the position table present and null
    X = CC.pe_exact(c, DEV)
    wp = X["wp"].view(-1, 22, 8)
    assert bool((wp[c["E"]:] == 0).all()) and bool((wp[:, :, 0] == 0).all()) and bool((wp[:, 21] == 0).all()), "w_perm's documented zero taps and rows"
    for with_pos in (True, False):
        out = PatchEmbedLaunch(ops, X, with_pos).run(L, expect=c["expect"])
        bits_equal(out, (X["ref"] if with_pos else X["pre"]).to(F32), f"{cid} exact pass, pos {'present' if with_pos else 'null'}")
    if not c["random"]:
        return
    del X
    # ---- pass 2: random operands against float64
    X = CC.pe_random(c, ops.OP16, DEV)
    out = PatchEmbedLaunch(ops, X, True).run(L)
    inside(out, X["ref"], error_bound(X["Sabs"], 176, X["pre"], X["ref"]), f"{cid} patch embed + pos vs float64")
    out = PatchEmbedLaunch(ops, X, False).run(L)
    inside(out, X["pre"], error_bound(X["Sabs"], 176, X["pre"], X["pre"]), f"{cid} patch embed vs float64")


@pytest.mark.parametrize("c", [CC.pe_case(2, 128, 33, "small"), CC.pe_case(2, 256, 96, "small"), CC.pe_case(2, 512, 112, "small")], ids=CC.pe_id)
def test_patch_embed_token_order(ops, L, c):
    """a token's arithmetic does not depend on its image's place in the batch: images 0 and 1 exchanged -> the same rows, exchanged"""
    assert CC.pe_id(c) in {CC.pe_id(d) for d in CC.PE_SMALL}
    X = CC.pe_random(c, ops.OP16, DEV)
    a = PatchEmbedLaunch(ops, X, True).run(L)
    b = PatchEmbedLaunch(ops, CC.swap_images(X, 0, 1), True).run(L, expect=c["expect"])
    n = a.shape[0] // 2
    assert not torch.equal(a[:n], a[n:])
    bits_equal(b[:n], a[n:], f"{CC.pe_id(c)} images exchanged, first half")
    bits_equal(b[n:], a[:n], f"{CC.pe_id(c)} images exchanged, second half")


@pytest.mark.parametrize("c", CC.IM2COL_CASES, ids=lambda c: f"b{c['B']}-s{c['S']}")
def test_im2col_patch(ops, L, c):
    """pure data movement: the bits of the restated index map applied to the operand-rounded image; columns 147..159 zero"""
    B, S = c["B"], c["S"]
    g = torch.Generator(device=DEV).manual_seed(S)
    img = nan_guarded(torch.randn(B, 3, S, S, generator=g, device=DEV))
    out = Flat((B * (S // 4) ** 2, 160), ops.OP16)
    reached(L, CC.IM2COL, "im2col_patch", [lambda: L.msam2_im2col_patch7x7s4(p(img), p(out.view), B, S, stream())])
    torch.cuda.synchronize()
    assert out.sentinels_intact(), "wrote before or behind the output"
    same_bits(out.view, CC.im2col_restate(img, ops.OP16), f"im2col_patch B={B} S={S}")
    assert bool((out.view[:, 147:] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. implicit-GEMM convolution
class ConvLaunch:
    """ops.conv3x3s2_mfma_ln_gelu with X between NaN guards, the packed weight with ldw = KP + 8 and NaN beyond KP, bias / ln_w / ln_b of
    exact length followed by NaN, Y in a Canvas with ldy > COUT"""

    def __init__(self, ops, x16, wp, bias, ln_w, ln_b, B, H, W):
        self.ops, self.shape = ops, (B, H, W)
        cout, KP = wp.shape
        self.cin = x16.numel() // (B * H * W)
        assert KP == (9 * self.cin + 7) // 8 * 8
        self.x = nan_guarded(x16.to(ops.OP16))
        self.w = nan_padded(cout, KP, KP + 8, ops.OP16, wp)
        self.bias, self.ln_w, self.ln_b = (nan_guarded(t.to(F32)) for t in (bias, ln_w, ln_b))
        self.y = Canvas(CC.conv_M(B, H, W), cout, ops.OP16)
        assert self.y.view.stride(0) > cout

    def call(self):
        B, H, W = self.shape
        self.ops.conv3x3s2_mfma_ln_gelu(self.x.reshape(B * H * W, self.cin), B, H, W, self.w, self.bias, self.ln_w, self.ln_b, CC.CONV_EPS, out=self.y.view)
        return 0

    def run(self, L, expect=None):
        if expect is not None:
            reached(L, expect, "conv3x3s2_mfma_kernel", [self.call])
        else:
            self.call()
        torch.cuda.synchronize()
        assert self.y.sentinels_intact(), "wrote outside the output view (padding columns, or rows past the last pixel)"
        return self.y.view


@pytest.mark.parametrize("cin,shape", [(cin, s) for cin in (4, 16, 64) for s in CC.CONV_SHAPES], ids=lambda v: str(v).replace(" ", ""))
def test_conv_exact(ops, L, cin, shape):
    """pass 1 on Y16: impulse inputs behind an exact LayerNorm, every sweep case of the shape (the kernel by name at the first)"""
    cases = [c for c in CC.CONV_EXACT if c["cin"] == cin and (c["B"], c["H"], c["W"]) == shape]
    assert cases and cases[0]["v"] == 0
    for c in cases:
        E = CC.conv_exact(c, DEV)
        K = 9 * cin
        assert bool((E["Wp"][:, K:E["KP"]] == 0).all()), "columns 9 CIN .. KP are zero"
        run = ConvLaunch(ops, E["X"], E["Wp"][:, :E["KP"]], E["bias"], E["ln_w"], E["ln_b"], *shape)
        y = run.run(L, expect=c["expect"] if c["v"] == 0 else None)
        bits_equal(y, E["y"].to(ops.OP16), f"{CC.conv_id(c)} exact pass, Y16")


@pytest.mark.parametrize("c", CC.CONV_RANDOM, ids=CC.conv_id)
def test_conv_random(ops, L, c):
    """pass 2: tests/test_mask_ds_fused_gpu.py's operands and bound, unchanged, at this file's shapes and guards, and the bits of the
    three launches"""
    cin, B, H, W = c["cin"], c["B"], c["H"], c["W"]
    cout = 4 * cin
    x, w, wp, bias, gamma, beta = MD.inputs(ops, B, H, W, cin)
    y16 = ConvLaunch(ops, x, wp, bias, gamma, beta, B, H, W).run(L, expect=c["expect"]).contiguous()
    same_bits(y16, MD.three_launches(ops, x, B, H, W, wp, bias, gamma, beta), f"{CC.conv_id(c)} against im2col + gemm + layernorm")
    x64 = x.double().permute(0, 3, 1, 2)
    nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(-1, cout)
    pre = nhwc(F.conv2d(x64, w.double(), bias.double(), stride=2, padding=1))
    S = nhwc(F.conv2d(x64.abs(), w.double().abs(), None, stride=2, padding=1))
    dpre = error_bound(S, (9 * cin + 7) // 8 * 8, pre, pre, fp16=op16_is_fp16())
    pre2, dpre2 = PB.ln_tail(pre, dpre, gamma.double(), beta.double(), MD.EPS)
    ref, bound = PB.act_store(pre2, dpre2, 1, True, op16_is_fp16())
    print(f"RATIO {CC.conv_id(c)} Y16 vs float64: {float(((y16.double() - ref).abs() / bound).max()):.4f}")
    within(y16, ref, bound, f"{CC.conv_id(c)} against float64")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. token heads
def guarded_i32(values):
    return nan_guarded(torch.tensor(values, dtype=torch.int32, device=DEV))


class TokenHeadsLaunch:
    """msam2_token_mlp3 / _packed: hs a strided view inside NaN (batch and token strides above contiguous), every table between guards, b3
    NaN past out_dim, the output in a Flat"""

    def __init__(self, ops, X, packed):
        B, T, C, G = X["B"], CC.TH_T, CC.TH_C, CC.TH_G
        self.B, self.packed = B, packed
        self.hs_ts, self.hs_bs = CC.TH_HS_TS, T * CC.TH_HS_TS + CC.TH_HS_PAD
        buf = torch.full((128 + B * self.hs_bs,), float("nan"), dtype=F32, device=DEV)
        self.hs = torch.as_strided(buf, (B, T, C), (self.hs_bs, self.hs_ts, 1), 64)
        self.hs.copy_(X["hs"].to(F32))
        self.w = [nan_guarded(w.to(ops.OP16)) for w in X["Ws"]]
        b3 = X["bs"][2].clone()
        for g, od in enumerate(CC.TH_OUT_DIM):
            b3[g, od:] = float("nan")
        self.b = [nan_guarded(t.to(F32)) for t in (X["bs"][0], X["bs"][1], b3)]
        self.tok, self.od, self.sg = guarded_i32(CC.TH_TOK), guarded_i32(CC.TH_OUT_DIM), guarded_i32(CC.TH_SIGMOID)
        off, ld, total = CC.th_packed_layout(B)
        self.off, self.ld = guarded_i32(off), guarded_i32(ld)
        self.out = Flat((total,) if packed else (B * G * C,), F32)

    def call(self, L):
        w, b = self.w, self.b
        head = (p(self.hs), self.hs_bs, self.hs_ts, p(self.tok), p(w[0]), p(b[0]), p(w[1]), p(b[1]), p(w[2]), p(b[2]), p(self.od), p(self.sg), p(self.out.view))
        if self.packed:
            return L.msam2_token_mlp3_packed(*head, p(self.off), p(self.ld), CC.TH_G, self.B, CC.TH_C, stream())
        return L.msam2_token_mlp3(*head, CC.TH_G, self.B, CC.TH_C, stream())

    def run(self, L, X):
        reached(L, CC.TOKEN_MLP3, "token_mlp3", [lambda: self.call(L)])
        torch.cuda.synchronize()
        assert self.out.sentinels_intact(), "wrote before or behind the output"
        want, allowed = CC.th_expected(X, self.packed)
        kept = self.out.view.view(torch.int32)[~allowed] == SENT32
        assert bool(kept.all()), f"{int((~kept).sum())} elements past out_dim (or between the packed regions) lost their sentinel"
        return self.out.view, want, allowed


def th_heads(B, allowed, sigmoid):
    """mask over the flat output of the elements that belong to heads with (without) sigmoid"""
    m = torch.zeros_like(allowed)
    off, ld, _ = CC.th_packed_layout(B)
    packed = allowed.numel() != B * CC.TH_G * CC.TH_C
    for g, od in enumerate(CC.TH_OUT_DIM):
        if bool(CC.TH_SIGMOID[g]) == sigmoid:
            for b in range(B):
                base = off[g] + b * ld[g] if packed else (b * CC.TH_G + g) * CC.TH_C
                m[base:base + od] = True
    return m


def th_flat(X, t, packed):
    """a [B, G, 256] tensor in the layout of the flat output"""
    return CC.th_expected(dict(X, ref=t), packed)[0]


@pytest.mark.parametrize("packed", [False, True], ids=["plain", "packed"])
@pytest.mark.parametrize("B", CC.TH_B)
def test_token_heads(ops, L, B, packed):
    # ---- pass 1: exact
    X = CC.th_exact(B, DEV)
    out, want, allowed = TokenHeadsLaunch(ops, X, packed).run(L, X)
    lin, sg = th_heads(B, allowed, False), th_heads(B, allowed, True)
    bits_equal(out[lin][None], want[lin].to(F32)[None], f"token heads B={B} exact pass, heads without sigmoid")
    x2 = X["pres"][1].clamp_min(0)
    S3 = torch.einsum("bgk,gok->bgo", x2.abs(), X["Ws"][2].abs())
    bound = th_flat(X, error_bound(S3, CC.TH_C, X["pres"][2], X["ref"], act=3), packed)
    inside(out[sg][None], want[sg][None], bound[sg][None], f"token heads B={B} exact pass, sigmoid heads vs the float64 sigmoid of the integer")
    # ---- pass 2: random
    X = CC.th_random(B, ops.OP16, DEV)
    out, want, allowed = TokenHeadsLaunch(ops, X, packed).run(L, X)
    bound = th_flat(X, CC.th_bound(X, error_bound), packed)
    print(f"RATIO token heads B={B} composed bound, worst: {float(((out.double() - want).abs() / bound)[allowed].max()):.3e}")
    inside(out[allowed][None], want[allowed][None], bound[allowed][None], f"token heads B={B} {'packed' if packed else 'plain'} vs float64")


def test_token_heads_packed_equals_plain(ops, L):
    X = CC.th_random(3, ops.OP16, DEV)
    a = TokenHeadsLaunch(ops, X, False).run(L, X)[0]
    b = TokenHeadsLaunch(ops, X, True).run(L, X)[0]
    off, ld, _ = CC.th_packed_layout(3)
    for g, od in enumerate(CC.TH_OUT_DIM):
        rows = torch.stack([b[off[g] + i * ld[g]:off[g] + i * ld[g] + od] for i in range(3)])
        bits_equal(rows, a.view(3, CC.TH_G, CC.TH_C)[:, g, :od].contiguous(), f"token heads, packed against plain, head {g}")


def test_same_file_on_the_bf16_library(ops):
    """the operand type is a property of the loaded library: the tests of this file once more in a child process on libmsam2_hip_bf16.so"""
    if os.environ.get("MSAM2_LIB_PATH"):
        assert str(ops.OP16).endswith(os.environ.get("MSAM2_EXPECT_OP16", "")), ops.OP16
        return                                              # this IS a run on a chosen library
    lib = os.path.join(ROOT, "medical-sam2_amd", "libmsam2_hip_bf16.so")
    assert os.path.exists(lib), "libmsam2_hip_bf16.so is built by __graft_entry__.build()"
    env = dict(os.environ, MSAM2_LIB_PATH=lib, MSAM2_EXPECT_OP16="bfloat16", PYTHONUNBUFFERED="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-30:])
    print(tail)
    assert r.returncode == 0 and " passed" in tail and "failed" not in tail, tail
