"""Variant matrix of the Hiera stage 1-2 fused kernels (GPU): attn_winproj_kernel (csrc/attn_winproj.hip) and mlp_fused_kernel /
mlp_fused384_kernel (csrc/mlp_fused.hip), every instantiation reached on purpose through the C entries of the library, in the style of
tests/test_attention_variants_gpu.py and tests/test_pointwise_variants_gpu.py:
  * each case names the instantiation it must reach; torch.profiler asserts that exactly that one ran (fused_cases.instantiations() is
    compared with a literal list in tests/test_fused_cases_cpu.py); the 4-wave forms of the plain entry (MSAM2_MLP_WAVES4=1, read once
    per process) run the plain-form cases in a child process;
  * every input, weight, bias and LayerNorm parameter has NaN on either side, every output lies inside a sentinel-filled buffer whose
    sentinels must be bit-identical afterwards (out16 / the attention output 8 bytes off a 16-byte boundary where the entry admits it);
  * pass 1, exact: operands built so that the output is known to the bit (fused_cases: every query selects its keys; integers all the way
    through the MLP) -- same_bits, no tolerance; a mismatch names token, head and channel;
  * pass 2, random: float64 references run on the GPU from the operand-rounded inputs.  Attention: the derived bound of
    fused_cases.attn_reference AND the project's 0.02 + 0.01 |ref|.  MLP: the project's own statement, btol(6e-3) + btol(4e-3) |ref|
    against the float64 reference and btol(4e-3) + btol(2e-3) |ref| against the three launches (test_kernels_gpu.py::
    test_ln_mlp_residual_fused); the sharpness is pass 1's.  The worst ratio to every limit is printed ("RATIO ...");
  * token order: out(x[perm]) == out(x)[perm] bit for bit (a token's arithmetic does not depend on its lane, wave or pass); for the
    attention kernel the same per window;
  * the PROJ form in place (out == res) gives the exact pass's bits; refusals return an error and launch nothing.
The 16-bit type is ops.OP16 throughout, so the bf16 build runs the file unchanged.
"""
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fused_cases as FC  # noqa: E402
from helpers import Flat, btol, kernels_launched, nan_guarded, reached  # noqa: E402

DEV = "cuda"
F32 = torch.float32
EPS = 1e-6


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import medical_sam2_amd.ops as ops_mod
    return ops_mod


@pytest.fixture(scope="module")
def L(ops):
    from medical_sam2_amd import _lib
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def p(t):
    return None if t is None else t.data_ptr()


def bits_equal(got, want, what, heads=None):
    """same_bits that names the first element that went wrong: token, (head,) channel"""
    it = {2: torch.int16, 4: torch.int32}[got.dtype.itemsize]
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    ne = got.contiguous().view(it) != want.contiguous().view(it)
    if bool(ne.any()):
        i = int(ne.flatten().nonzero()[0])
        t, ch = divmod(i, got.shape[1])
        where = f"token {t}, head {ch // FC.HD}, channel {ch % FC.HD}" if heads else f"token {t}, channel {ch}"
        rows = ne.any(1).nonzero().flatten()
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} elements in {len(rows)} rows differ in their bits; first at {where}: "
                             f"got {float(got.flatten()[i])}, expected {float(want.flatten()[i])}; rows {rows[:12].tolist()}")


def inside(got, ref, bound, what):
    """|got - ref| <= bound element by element (a NaN fails); prints and returns the worst ratio"""
    d = (got.double() - ref).abs()
    ratio = d / bound
    worst = float(ratio.max())
    print(f"RATIO {what}: {worst:.4f} (max |err| {float(d.max()):.4g})")
    bad = ~(d <= bound)
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        t, ch = divmod(i, got.shape[1])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound, worst ratio {worst:.3f}; first at token {t}, "
                             f"channel {ch}: got {float(got.flatten()[i])}, reference {float(ref.flatten()[i])}")
    return worst


def one_ulp(got, want, what):
    """16-bit rows whose bit patterns, mapped to one monotonic integer line, are equal or neighbours"""
    line = lambda v: (lambda i: torch.where(i < 0, -(i & 0x7FFF), i))(v.contiguous().view(torch.int16).int())
    bad = (line(got) - line(want)).abs() > 1
    assert got.dtype == want.dtype and not bool(bad.any()), f"{what}: {int(bad.sum())} values beyond one ulp, rows {bad.any(1).nonzero().flatten()[:12].tolist()}"


# =================================================================================================================================
# window attention with the qkv projection inside
def attn_call(L, c, xn, w, b, o):
    return L.msam2_window_qkv_attention_fwd(p(xn), p(w), p(b), p(o), c["B"], c["H"], c["W"], c["dim"], c["heads"], c["ws"], int(c["pool"]),
                                            1.0 / math.sqrt(FC.HD), stream())


def attn_run(L, c, ops, xn, w, b, offset, expect=None):
    """launch on NaN-guarded copies of the float64 holders into a sentinel buffer; returns the output view (sentinels checked)"""
    gx, gw, gb = nan_guarded(xn.to(ops.OP16)), nan_guarded(w.to(ops.OP16)), nan_guarded(b.to(F32))
    Hq, Wq, _ = FC.out_geometry(c)
    out = Flat((c["B"] * Hq * Wq, c["heads"] * FC.HD), ops.OP16, offset=offset)
    if expect is not None:
        reached(L, expect, "attn_winproj", [lambda: attn_call(L, c, gx, gw, gb, out.view)])
    else:
        assert attn_call(L, c, gx, gw, gb, out.view) == 0, L.msam2_last_error().decode()
    torch.cuda.synchronize()
    assert out.sentinels_intact(), "the kernel wrote outside its output"
    return out.view


@pytest.mark.parametrize("c", FC.ATTN_CASES, ids=FC.attn_id)
def test_attention_variant(ops, L, c):
    assert ops.window_qkv_attention_supported(c["dim"], c["heads"] * FC.HD, c["heads"], c["ws"], c["pool"], c["H"], c["W"])
    cid = FC.attn_id(c)
    # ---- pass 1: exact.  The output sits 8 bytes off a 16-byte boundary (what the entry's check admits)
    xn, w, b, exp = FC.attn_exact(c, DEV)
    got = attn_run(L, c, ops, xn, w, b, 4, expect=c["expect"])
    bits_equal(got, exp.to(ops.OP16), f"{cid} exact pass", heads=c["heads"])
    # ---- pass 2: random operands against the float64 reference
    xn, w, b = FC.attn_random(c, ops.OP16, DEV)
    ref, bound = FC.attn_reference(c, xn, w, b, ops.OP16)
    got = attn_run(L, c, ops, xn, w, b, 0)
    inside(got, ref, bound, f"{cid} derived bound")
    inside(got, ref, 0.02 + 0.01 * ref.abs(), f"{cid} 0.02 + 0.01 |ref|")
    # ---- window order: the windows of the token image permuted (other units, other pair mates, other passes) -> the same rows, permuted
    B, H, W, ws = c["B"], c["H"], c["W"], c["ws"]
    Hq, Wq, wq = FC.out_geometry(c)
    sigma = torch.randperm(B * c["nw"], generator=torch.Generator().manual_seed(3)).to(DEV)
    xw = FC.to_windows(xn.reshape(B, H, W, c["dim"]), ws)
    got2 = attn_run(L, c, ops, FC.from_windows(xw[sigma], B, H, W, ws), w, b, 0)
    ow = FC.to_windows(got.reshape(B, Hq, Wq, -1), wq)
    bits_equal(got2, FC.from_windows(ow[sigma], B, Hq, Wq, wq), f"{cid} windows permuted", heads=c["heads"])


def refused(L, prefix, fn, what):
    """fn returns an error code and launches no kernel of the family"""
    def go():
        assert fn() != 0, f"{what}: accepted"
    assert kernels_launched(go, prefix) == set(), what
    assert L.msam2_last_error()


@pytest.mark.parametrize("r", FC.ATTN_REFUSED, ids=lambda r: "d{}-h{}-ws{}-{}x{}".format(r[0], r[1], r[2], r[4], r[5]))
def test_attention_gate_refuses(ops, L, r):
    dim, heads, ws, pool, H, W = r
    assert not ops.window_qkv_attention_supported(dim, heads * FC.HD, heads, ws, pool, H, W)
    c = dict(dim=dim, heads=heads, ws=ws, pool=pool, B=1, H=H, W=W)
    xn = torch.zeros(H * W, dim, dtype=ops.OP16, device=DEV)
    w = torch.zeros(3 * heads * FC.HD, dim, dtype=ops.OP16, device=DEV)
    b = torch.zeros(3 * heads * FC.HD, device=DEV)
    o = Flat((H * W, heads * FC.HD), ops.OP16)
    refused(L, "attn_winproj", lambda: attn_call(L, c, xn, w, b, o.view), str(r))
    assert o.sentinels_intact()


def test_attention_refuses_odd_height_with_pool_and_misaligned_pointers(ops, L):
    assert not ops.window_qkv_attention_supported(96, 96, 1, 8, True, 8, 8 + 1)
    c = FC.attn(96, 1, True, 1, 8, 8)
    xn, w, b, _ = FC.attn_exact(c, DEV)
    xn, w, b = nan_guarded(xn.to(ops.OP16)), nan_guarded(w.to(ops.OP16)), nan_guarded(b.to(F32))
    o = Flat((16, FC.HD), ops.OP16, offset=2)                  # 4 bytes off
    good = Flat((16, FC.HD), ops.OP16)
    call = lambda xx, ww, bb, oo: L.msam2_window_qkv_attention_fwd(xx, ww, bb, oo, 1, 8, 8, 96, 1, 8, 1, 1.0 / math.sqrt(FC.HD), stream())
    for what, args in (("xn", (p(xn) + 4, p(w), p(b), p(good.view))), ("w", (p(xn), p(w) + 4, p(b), p(good.view))),
                       ("bias", (p(xn), p(w), p(b) + 4, p(good.view))), ("o", (p(xn), p(w), p(b), p(o.view)))):
        refused(L, "attn_winproj", lambda a=args: call(*a), f"{what} 4 bytes off its alignment")
    assert o.sentinels_intact() and good.sentinels_intact()


# =================================================================================================================================
# LayerNorm + MLP + residual in one kernel (plain, dual, PROJ forms; dim 384)
_WEIGHTS = {}


def mlp_weights(ops, dim, kind):
    """device weights of a width, built once, every tensor NaN-guarded: kind "exact" / "random" """
    key = (dim, kind)
    if key not in _WEIGHTS:
        P = FC.mlp_exact_weights(dim, DEV) if kind == "exact" else FC.mlp_random_weights(dim, ops.OP16, DEV)
        R = P                                                        # (the exact pass has next-norm parameters of its own)
        w1, w2 = P["w1"].to(ops.OP16), P["w2"].to(ops.OP16)
        Wd = {k: nan_guarded(P[k].to(F32)) for k in ("ln_w", "ln_b", "b1", "b2", "bp")}
        Wd.update(nln_w=nan_guarded(R["nln_w"].to(F32)), nln_b=nan_guarded(R["nln_b"].to(F32)), w1=nan_guarded(w1), w2=w2,
                  w2p=nan_guarded(ops.mlp_fused_permute_w2(w2)), wp=nan_guarded(P["wp"].to(ops.OP16)))
        if dim != 384:
            Wd["w1p"] = nan_guarded(ops.mlp_fused_permute_w1(w1))
        _WEIGHTS[key] = Wd
    return _WEIGHTS[key]


class MlpRun:
    """one launch of a case's entry: inputs NaN-guarded, outputs in sentinel buffers (the dual entry's out16 8 bytes off a 16-byte
    boundary); in_place: out == res (PROJ)"""

    def __init__(self, L, ops, c, Wd, x, o=None, res=None, in_place=False):
        self.L, self.c, self.Wd = L, c, Wd
        T, dim, form, side = c["T"], c["dim"], c["form"], c["side"]
        self.proj = form == "proj"
        self.out16 = Flat((T, dim), ops.OP16, offset=4 if form == "dual" else 0) if (form == "dual" or side & 1) else None
        self.xn16 = Flat((T, dim), ops.OP16) if side & 2 else None
        self.out = Flat((T, dim), F32)
        if self.proj:
            self.o = nan_guarded(o.to(ops.OP16))
            if in_place:
                self.out.view.copy_(res.to(F32))
                self.res = self.out.view
            else:
                self.res = nan_guarded(res.to(F32))
        else:
            self.x = nan_guarded(x.to(F32))

    def launch(self):
        L, c, W = self.L, self.c, self.Wd
        T, dim = c["T"], c["dim"]
        o16 = self.out16.view if self.out16 else None
        if self.proj:
            xn = self.xn16.view if self.xn16 else None
            return L.msam2_proj_ln_mlp_residual_fwd(p(self.o), p(W["wp"]), p(W["bp"]), p(self.res), T, dim, p(W["ln_w"]), p(W["ln_b"]), EPS, p(W["w1p"]),
                                                    p(W["b1"]), p(W["w2p"]), p(W["b2"]), p(self.out.view), p(o16), p(W["nln_w"]) if xn is not None else None,
                                                    p(W["nln_b"]) if xn is not None else None, EPS, p(xn), stream())
        args = (p(self.x), T, dim, p(W["ln_w"]), p(W["ln_b"]), EPS, p(W["w1"]), p(W["b1"]), p(W["w2p"]), p(W["b2"]), p(self.out.view))
        if c["form"] == "dual":
            return L.msam2_ln_mlp_residual_fwd_dual(*args, p(o16), stream())
        return L.msam2_ln_mlp_residual_fwd(*args, stream())

    def run(self, expect=None):
        if expect is not None:
            reached(self.L, expect, "mlp_fused", [self.launch])
        else:
            assert self.launch() == 0, self.L.msam2_last_error().decode()
        torch.cuda.synchronize()
        for f in (self.out, self.out16, self.xn16):
            assert f is None or f.sentinels_intact(), "the kernel wrote outside an output"
        return self

    def check_side_outputs(self, ops, what, ulp):
        """out16 = the fp32 rows rounded, bit for bit.  xn16 = LayerNorm of the kernel's own fp32 rows: inside the derived bound of
        fused_cases.next_norm_reference around the float64 LayerNorm of those rows, and (ulp: the exact pass, the project's statement of
        tests/test_proj_mlp_fused_gpu.py::test_side_outputs) within one 16-bit ulp of ops.layernorm.  The latter needs next-norm
        parameters that keep the result away from zero (fused_cases.mlp_exact_weights) and is not asked of the random pass: two correct
        fp32 evaluations are further apart than a 16-bit ulp where the result cancels to near zero and on the row with mean = 1000 std.
        Measured with parameters (1 + 0.1 randn, 0.1 randn): 11 of 12.6 M values beyond one ulp on the random pass at dim 96 under fp16,
        5 (dim 96) and 7 (dim 192) of 12.6 M on the exact pass's rows under bf16 -- every one of them inside the derived bound."""
        if self.out16:
            bits_equal(self.out16.view, self.out.view.to(ops.OP16), f"{what} out16")
        if self.xn16:
            ref, bound = FC.next_norm_reference(self.out.view, self.Wd["nln_w"], self.Wd["nln_b"], EPS, ops.OP16)
            inside(self.xn16.view, ref, bound, f"{what.split()[0]} xn16 derived bound")
            if ulp:
                one_ulp(self.xn16.view, ops.layernorm(self.out.view.contiguous(), self.Wd["nln_w"], self.Wd["nln_b"], EPS), f"{what} xn16")


def three_launches(ops, Wd, x1):
    xn = ops.layernorm(x1, Wd["ln_w"], Wd["ln_b"], EPS)
    hid = ops.gemm(xn, Wd["w1"], Wd["b1"], act=ops.ACT_GELU)
    return ops.gemm(hid, Wd["w2"], Wd["b2"], residual=x1, out_dtype=F32)


@pytest.mark.parametrize("c", FC.MLP_CASES, ids=FC.mlp_id)
def test_mlp_variant(ops, L, c):
    dim, T, proj = c["dim"], c["T"], c["form"] == "proj"
    cid = FC.mlp_id(c)
    # ---- pass 1: exact
    Wd = mlp_weights(ops, dim, "exact")
    P = FC.mlp_exact(dim, T, DEV)
    want = P["out"].to(F32)
    r = MlpRun(L, ops, c, Wd, P["x"], P["o"], P["res"]).run(expect=c["expect"])
    bits_equal(r.out.view, want, f"{cid} exact pass")
    r.check_side_outputs(ops, f"{cid} exact pass", ulp=True)
    if proj and c["side"] == 0:                                   # in place: nothing is re-read in the store
        r = MlpRun(L, ops, c, Wd, P["x"], P["o"], P["res"], in_place=True).run()
        bits_equal(r.out.view, want, f"{cid} exact pass, out == res")
    del P, r
    # ---- pass 2: random rows (GELU's curved range, real LayerNorm rows, a row with mean = 1000 std, a constant row)
    Wd = mlp_weights(ops, dim, "random")
    P = FC.mlp_random(dim, T, ops.OP16, DEV)
    ref = FC.mlp_reference(P, proj)
    r = MlpRun(L, ops, c, Wd, P["x"], P["o"], P["res"]).run()
    inside(r.out.view, ref, btol(6e-3) + btol(4e-3) * ref.abs(), f"{cid} vs float64")
    x1 = ops.gemm(r.o, Wd["wp"], Wd["bp"], residual=r.res, out_dtype=F32) if proj else r.x
    three = three_launches(ops, Wd, x1)
    inside(r.out.view, three.double(), btol(4e-3) + btol(2e-3) * three.double().abs(), f"{cid} vs three launches")
    r.check_side_outputs(ops, f"{cid} random pass", ulp=False)
    # ---- token order
    perm = torch.randperm(T, generator=torch.Generator().manual_seed(9)).to(DEV)
    r2 = MlpRun(L, ops, c, Wd, P["x"][perm], P["o"][perm], P["res"][perm]).run()
    bits_equal(r2.out.view, r.out.view[perm], f"{cid} tokens permuted")
    for a, b in ((r2.out16, r.out16), (r2.xn16, r.xn16)):
        if a:
            bits_equal(a.view, b.view[perm], f"{cid} tokens permuted, 16-bit rows")


@pytest.mark.skipif(FC.WAVES4, reason="this IS the child process")
def test_four_wave_forms_in_a_child_process():
    """mlp_fused_kernel<96,192,4,1,4> and <192,96,2,1,4> (MSAM2_MLP_WAVES4=1, read once per process) on the plain-form cases"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    count = sum(1 for c in FC.MLP_CASES if c["form"] in ("plain", "dual") and c["dim"] != 384)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider", "-k",
                        "test_mlp_variant and (plain or dual) and not d384"],
                       env={**os.environ, "MSAM2_MLP_WAVES4": "1"}, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0 and f"{count} passed" in r.stdout, (r.stdout + r.stderr)[-3000:]


@pytest.mark.parametrize("form,dim", [("plain", 96), ("dual", 192), ("plain", 384), ("proj", 96), ("proj", 192)])
def test_mlp_refusals(ops, L, form, dim):
    """a pointer 4 bytes off its required alignment, x == out (plain), xn16 without its parameters (PROJ): an error, nothing launched"""
    T = 33
    c = FC.mlp(form, dim, T, 3 if form == "proj" else 0)
    Wd = mlp_weights(ops, dim, "exact")
    P = FC.mlp_exact(dim, T, DEV)
    r = MlpRun(L, ops, c, Wd, P["x"], P["o"], P["res"])
    assert r.launch() == 0, L.msam2_last_error().decode()         # the form itself is accepted
    torch.cuda.synchronize()

    def shifted(obj, name, is_flat=False):
        """obj.<name> (or its Flat's view) replaced by a view 4 bytes further on for one launch"""
        def go():
            old = getattr(obj, name)
            t = old.view if is_flat else old
            es = t.element_size()
            moved = torch.as_strided(t, t.shape, t.stride(), t.storage_offset() + 4 // es)
            if is_flat:
                old.view, keep = moved, old.view
            else:
                setattr(obj, name, moved)
            try:
                return r.launch()
            finally:
                if is_flat:
                    old.view = keep
                else:
                    setattr(obj, name, old)
        return go

    for name in (("o", "res") if form == "proj" else ("x",)):
        refused(L, "mlp_fused", shifted(r, name), f"{form} {name} 4 bytes off")
    refused(L, "mlp_fused", shifted(r, "out", True), f"{form} out 4 bytes off")
    if r.out16:
        refused(L, "mlp_fused", shifted(r, "out16", True), f"{form} out16 4 bytes off")
    if r.xn16:
        refused(L, "mlp_fused", shifted(r, "xn16", True), f"{form} xn16 4 bytes off")
    for k in ["ln_w", "ln_b", "b1", "b2", "w2p"] + (["w1p", "wp", "bp", "nln_w", "nln_b"] if form == "proj" else ["w1"]):
        old = Wd[k]
        Wd[k] = torch.as_strided(old, old.shape, old.stride(), old.storage_offset() + 4 // old.element_size())
        try:
            refused(L, "mlp_fused", r.launch, f"{form} {k} 4 bytes off")
        finally:
            Wd[k] = old
    if form == "plain":
        x = r.x
        refused(L, "mlp_fused", lambda: L.msam2_ln_mlp_residual_fwd(p(x), T, dim, p(Wd["ln_w"]), p(Wd["ln_b"]), EPS, p(Wd["w1"]), p(Wd["b1"]), p(Wd["w2p"]),
                                                                     p(Wd["b2"]), p(x), stream()), "x == out")
    if form == "proj":
        refused(L, "mlp_fused", lambda: L.msam2_proj_ln_mlp_residual_fwd(p(r.o), p(Wd["wp"]), p(Wd["bp"]), p(r.res), T, dim, p(Wd["ln_w"]), p(Wd["ln_b"]), EPS,
                                                                          p(Wd["w1p"]), p(Wd["b1"]), p(Wd["w2p"]), p(Wd["b2"]), p(r.out.view), None, None, None,
                                                                          EPS, p(r.xn16.view), stream()), "xn16 without its parameters")
    # nothing refused has touched an output
    torch.cuda.synchronize()
    for f in (r.out, r.out16, r.xn16):
        assert f is None or f.sentinels_intact()
