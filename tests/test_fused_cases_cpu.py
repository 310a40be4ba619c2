"""The variant matrix of the stage 1-2 fused kernels (tests/test_fused_variants_gpu.py) must be able to fail.  On the CPU:
  1. every exact builder's operands and expected outputs are exact in fp16 and in bf16, the expected rows of a case are pairwise distinct,
     and an fp32 restatement of the kernel in two summation orders (attention: with the exponent's multiply-add fused or not; MLP: with
     GELU moved by +-(1e-5 relative + 5e-5 absolute)) gives the expected bits in both operand types;
  2. the random pass's bound holds for those fp32 restatements, with room;
  3. every simulated defect of fused_cases.ATTN_DEFECTS / MLP_DEFECTS changes the exact pass of a named case (or writes outside its output);
  4. the case tables cover the literal list of 17 instantiations, and the permutation restated here is ops.mlp_fused_w1_order.
The grid-wrap cases are restated on their second-pass units only (the first pass is what the smaller cases run)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fused_cases as FC  # noqa: E402

OP16S = (torch.float16, torch.bfloat16)
SMALL_ATTN = [c for c in FC.ATTN_CASES if c["units"] <= 64]
WRAP_ATTN = [c for c in FC.ATTN_CASES if c["units"] > FC.GRID * FC.NWV]
ATTN_BY_ID = {FC.attn_id(c): c for c in FC.ATTN_CASES}


def test_tables_cover_the_17_instantiations():
    want = ["attn_winproj_kernel<96,8,false,false,8>", "attn_winproj_kernel<96,8,true,false,8>", "attn_winproj_kernel<192,4,false,true,8>",
            "attn_winproj_kernel<192,4,true,true,8>",
            "mlp_fused_kernel<96,192,2,1,8,false,0>", "mlp_fused_kernel<192,96,1,1,8,false,0>", "mlp_fused384_kernel",
            "mlp_fused_kernel<96,192,2,1,8,true,0>", "mlp_fused_kernel<96,192,2,1,8,true,1>", "mlp_fused_kernel<96,192,2,1,8,true,2>",
            "mlp_fused_kernel<96,192,2,1,8,true,3>", "mlp_fused_kernel<192,96,1,1,8,true,0>", "mlp_fused_kernel<192,96,1,1,8,true,1>",
            "mlp_fused_kernel<192,96,1,1,8,true,2>", "mlp_fused_kernel<192,96,1,1,8,true,3>",
            "mlp_fused_kernel<96,192,4,1,4,false,0>", "mlp_fused_kernel<192,96,2,1,4,false,0>"]
    assert len(want) == 17 and sorted(want) == FC.instantiations()
    ids = [FC.attn_id(c) for c in FC.ATTN_CASES] + [FC.mlp_id(c) for c in FC.MLP_CASES]
    assert len(set(ids)) == len(ids)
    # the paths the shapes are there for
    assert len(WRAP_ATTN) == 10 and {(c["dim"], c["heads"]) for c in WRAP_ATTN} == {(96, 1), (96, 2), (192, 1), (192, 2), (192, 3)}
    assert any(c["units"] % FC.NWV for c in SMALL_ATTN), "a ragged pass: clamped waves"
    assert any(c["dim"] == 192 and (c["W"] // 4) % 2 for c in FC.ATTN_CASES), "a 4 x 4 pair that straddles two window rows"
    assert {c["heads"] for c in FC.ATTN_CASES if c["dim"] == 192} == {1, 2, 3, 4, 8}
    for dim in (96, 192):
        Ts = {c["T"] for c in FC.MLP_CASES if c["dim"] == dim and c["form"] == "plain"}
        assert max(Ts) > FC.GRID * FC.PASS[dim] and {1, FC.PASS[dim] - 1, FC.PASS[dim] + 1} <= Ts
        assert {c["side"] for c in FC.MLP_CASES if c["dim"] == dim and c["form"] == "proj" and c["T"] > FC.GRID * FC.PASS[dim]} == {0, 1, 2, 3}


def test_permutation_is_the_products():
    import medical_sam2_amd.ops as ops
    for dim in (96, 192, 384, 768):
        assert torch.equal(FC.w1_order(dim), ops.mlp_fused_w1_order(dim))
        assert sorted(FC.w1_order(dim).tolist()) == list(range(dim))


def test_gate_refusals_are_what_the_gate_says():
    """msam2_window_qkv_attention_supported restated: every refused shape of the table is refused, every case admitted"""
    def gate(dim, heads, ws, pool, H, W):
        if ws not in (8, 4) or H % ws or W % ws or (pool and (H % 2 or W % 2)) or (ws == 4 and ((H // 4) * (W // 4)) % 2):
            return False
        return (dim == 96 and ws == 8 and heads <= 2) or (dim == 192 and ws == 4 and heads <= 8)
    assert not any(gate(*r) for r in FC.ATTN_REFUSED)
    assert all(gate(c["dim"], c["heads"], c["ws"], c["pool"], c["H"], c["W"]) for c in FC.ATTN_CASES)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SMALL_ATTN, ids=FC.attn_id)
def test_attention_exact_pass(c):
    xn, w, b, exp = FC.attn_exact(c)
    assert all(FC.exact16(t) for t in (xn, w, b, exp))
    assert torch.unique(exp, dim=0).shape[0] == exp.shape[0], "two output rows of the case are equal"
    for h in range(c["heads"]):
        pi = FC.head_perm(c, h)
        assert bool((pi[pi] != torch.arange(len(pi))).any())                  # no involution
    for op16 in OP16S:
        e16 = exp.to(op16)
        for fma, order in ((True, 0), (False, 0), (True, 1)):
            rows, vals = FC.attn_restate(c, xn, w, b, op16, fma=fma, order=order)
            assert sorted(rows.tolist()) == list(range(exp.shape[0])), "every output row is stored exactly once"
            assert FC.attn_verdict(rows, vals, e16) is None, (op16, fma, order)


@pytest.mark.parametrize("c", WRAP_ATTN, ids=FC.attn_id)
def test_attention_exact_pass_second_pass_units(c):
    xn, w, b, exp = FC.attn_exact(c)
    assert all(FC.exact16(t) for t in (xn, w, b, exp))
    units = list(range(FC.GRID * FC.NWV, c["units"]))
    assert units
    for op16 in OP16S:
        rows, vals = FC.attn_restate(c, xn, w, b, op16, units=units)
        assert FC.attn_verdict(rows, vals, exp.to(op16)) is None


@pytest.mark.parametrize("c", [c for c in SMALL_ATTN if c["B"] * c["H"] * c["W"] <= 288], ids=FC.attn_id)
def test_attention_random_bound_holds_for_fp32_evaluations(c):
    for op16 in OP16S:
        xn, w, b = FC.attn_random(c, op16)
        ref, bound = FC.attn_reference(c, xn, w, b, op16)
        worst = 0.0
        for fma, order in ((True, 0), (False, 0), (True, 1)):
            rows, vals = FC.attn_restate(c, xn, w, b, op16, fma=fma, order=order)
            got = torch.zeros_like(ref)
            got[rows] = vals.double()
            ratio = ((got - ref).abs() / bound).max().item()
            worst = max(worst, ratio, ((got - ref).abs() / (0.02 + 0.01 * ref.abs())).max().item())
        assert worst < 1.0, (op16, worst)


# defect -> the case that must see it
ATTN_DEFECT_CASE = {
    "keys 4..7 and 8..11 of a block exchanged": "attn-d96-h1-1x8x8",
    "the two windows of a 4 x 4 pair exchanged": "attn-d192-h2-1x4x8",
    "block-diagonal mask of the pair dropped": "attn-d192-h1-1x4x8",
    "nwx taken for windows per column": "attn-d192-h3-1x8x12",
    "pooled query from the quad's first token": "attn-d96-h2-pool-1x8x24",
    "q and k slabs exchanged": "attn-d192-h8-1x4x8",
    "head h reads head h ^ 1's v slab": "attn-d96-h2-3x16x24",
    "second pass reads every slab from the other ring slot": "attn-d192-h3-17x64x64",
    "a clamped wave's rows stored": "attn-d192-h2-pool-3x8x12",
}


@pytest.mark.parametrize("defect", FC.ATTN_DEFECTS)
def test_attention_defect_is_caught(defect):
    c = ATTN_BY_ID[ATTN_DEFECT_CASE[defect]]
    xn, w, b, exp = FC.attn_exact(c)
    units = list(range(FC.GRID * FC.NWV, c["units"])) if c["units"] > FC.GRID * FC.NWV else None
    for op16 in OP16S:
        e16 = exp.to(op16)
        assert FC.attn_verdict(*FC.attn_restate(c, xn, w, b, op16, units=units), e16) is None
        verdict = FC.attn_verdict(*FC.attn_restate(c, xn, w, b, op16, units=units, defect=defect), e16)
        # (a wrong window map on 2 x 3 windows also leaves the image: its first finding is a store outside the output)
        want = {"a clamped wave's rows stored": "sentinel", "nwx taken for windows per column": "sentinel"}.get(defect, "bits")
        assert verdict == want, (defect, verdict)


def test_attention_also_nwx_defect_on_dim96_and_pool_defect_on_dim192():
    for cid, defect in (("attn-d96-h1-3x16x24", "nwx taken for windows per column"), ("attn-d192-h4-pool-1x4x8", "pooled query from the quad's first token"),
                        ("attn-d192-h1-17x64x64", "second pass reads every slab from the other ring slot")):
        c = ATTN_BY_ID[cid]
        xn, w, b, exp = FC.attn_exact(c)
        units = list(range(FC.GRID * FC.NWV, c["units"])) if c["units"] > FC.GRID * FC.NWV else None
        assert FC.attn_verdict(*FC.attn_restate(c, xn, w, b, torch.bfloat16, units=units, defect=defect), exp.to(torch.bfloat16)) is not None


# ---------------------------------------------------------------------------------------------------------------------------------
MLP_SHAPES = [(dim, T) for dim in (96, 192) for T in (1, 33, FC.PASS[dim] + 1, 3 * FC.PASS[dim] + 17)] + [(384, 1), (384, 229)]


@pytest.mark.parametrize("dim,T", MLP_SHAPES)
def test_mlp_exact_pass(dim, T):
    P = FC.mlp_exact(dim, T)
    assert all(FC.exact16(P[k]) for k in ("ln_w", "ln_b", "w1", "w2", "wp", "o", "hid"))
    assert all(bool((P[k].float().double() == P[k]).all()) for k in ("x", "res", "out", "b1", "b2", "bp"))
    assert bool((P["hid"] == P["hid"].round()).all()) and 8 <= float(P["hid"].min()) and float(P["hid"].max()) <= 255
    if T > 1:
        assert torch.unique(P["out"], dim=0).shape[0] == T, "two output rows of the case are equal"
    for op16 in OP16S:
        for proj in ((False, True) if dim != 384 else (False,)):
            for order, pert in ((0, 0.0), (1, 0.0), (0, 1.0), (1, -1.0)):
                out, out16 = FC.mlp_restate(P, dim, op16, proj, order=order, gelu_pert=pert)
                assert torch.equal(out, P["out"].float()), (op16, proj, order, pert)
                assert torch.equal(out16.view(torch.int16), P["out"].float().to(op16).view(torch.int16))


@pytest.mark.parametrize("dim", [96, 192, 384])
def test_mlp_random_bound_holds_for_fp32_evaluations(dim):
    """the project's statement 6e-3 + 4e-3 |ref| (fp16; 4 x that for bf16) against the float64 reference, both summation orders"""
    T = 300
    for op16, f in ((torch.float16, 1.0), (torch.bfloat16, 4.0)):
        P = FC.mlp_random(dim, T, op16)
        for proj in ((False, True) if dim != 384 else (False,)):
            ref = FC.mlp_reference(P, proj)
            for order in (0, 1):
                out, _ = FC.mlp_restate(P, dim, op16, proj, order=order)
                ratio = ((out.double() - ref).abs() / (f * 6e-3 + f * 4e-3 * ref.abs())).max().item()
                assert ratio < 1.0, (dim, op16, proj, order, ratio)


@pytest.mark.parametrize("dim", [96, 192])
def test_next_norm_bound_holds_for_fp32_evaluations(dim):
    """fp32 LayerNorm of random rows (one with mean = 1000 std, one constant) in two summation orders, rounded to 16 bits: inside
    next_norm_reference's bound -- and not all within one 16-bit ulp of each other, which is why the random pass does not ask for that"""
    g = torch.Generator().manual_seed(dim)
    x = torch.randn(4000, dim, generator=g) * 1.5 + 0.3
    x[1] = 1000.0 + torch.randn(dim, generator=g)
    x[-1] = 2.0
    w, b = 1 + 0.1 * torch.randn(dim, generator=g), 0.1 * torch.randn(dim, generator=g)
    orders = [torch.arange(dim), torch.randperm(dim, generator=g)]
    for op16 in OP16S:
        ref, bound = FC.next_norm_reference(x, w, b, 1e-6, op16)
        for o in orders:
            mean = x[:, o].cumsum(1)[:, -1:] * torch.tensor(1.0 / dim)
            d = x - mean
            rstd = 1.0 / torch.sqrt((d * d)[:, o].cumsum(1)[:, -1:] * torch.tensor(1.0 / dim) + 1e-6)
            got = (d * rstd * w + b).to(op16)
            ratio = ((got.double() - ref).abs() / bound).max().item()
            assert ratio < 1.0, (dim, op16, ratio)


MLP_DEFECT_CASE = {          # defect -> (dim, T, proj) of the case that must see it
    "W2's hidden permutation omitted": (96, 33, False),
    "W1's input permutation omitted (PROJ)": (192, 33, True),
    "the two lane halves' channels exchanged": (96, 1, True),
    "chunk c computed with chunk c - 1's weights": (192, 1, False),
    "b1 offset by one 32-block": (96, 1, False),
    "bp added twice": (192, 33, True),
    "residual taken from the clamped row on a ragged pass": (96, 3 * 512 + 17, False),
    "out16 rounded from the pre-residual value": (192, 33, False),
}


@pytest.mark.parametrize("defect", FC.MLP_DEFECTS)
def test_mlp_defect_is_caught(defect):
    dim, T, proj = MLP_DEFECT_CASE[defect]
    assert any(c["dim"] == dim and c["T"] == T and (c["form"] == "proj") == proj for c in FC.MLP_CASES)
    P = FC.mlp_exact(dim, T)
    for op16 in OP16S:
        want32, want16 = P["out"].float(), P["out"].float().to(op16)
        out, out16 = FC.mlp_restate(P, dim, op16, proj, defect=defect)
        assert not (torch.equal(out, want32) and torch.equal(out16, want16)), defect
        if defect != "out16 rounded from the pre-residual value":
            assert not torch.equal(out, want32)
    # dim 384's chunk-shift too (32-unit chunks)
    if defect == "chunk c computed with chunk c - 1's weights":
        P = FC.mlp_exact(384, 63)
        assert not torch.equal(FC.mlp_restate(P, 384, torch.float16, False, defect=defect)[0], P["out"].float())
