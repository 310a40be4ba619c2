"""The variant matrix of the patch embed, implicit-GEMM convolution and token-head kernels (tests/test_conv_variants_gpu.py) must be able
to fail.  On the CPU:
  1. the case tables cover the literal lists of instantiations (12 + 1, 5 and 1) and the shapes reach the paths they are there for;
  2. every exact builder meets the conditions it asserts, and the restatements of the index walks (conv_cases.pe_restate, conv_restate,
     th_restate, im2col_restate) give the expected bits in fp16 and in bf16;
  3. every simulated defect changes the exact pass of a named case, or stores where the output's sentinels are;
  4. the random pass's bounds hold for the fp32 restatements.
The large patch-embed cases are restated on the segments they are there for (interior, second and third trip, the last one)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_cases as CC  # noqa: E402
from test_gemm_variants_gpu import error_bound  # noqa: E402

OP16S = (torch.float16, torch.bfloat16)


def pe_find(path, S, E=None, B=None):
    for c in CC.PE_CASES:
        if c["path"] == path and c["S"] == S and (E is None or c["E"] == E) and (B is None or c["B"] == B):
            return c
    raise KeyError((path, S, E, B))


def conv_find(cin, shape, v=0):
    for c in CC.CONV_EXACT:
        if (c["cin"], (c["B"], c["H"], c["W"]), c["v"]) == (cin, shape, v):
            return c
    raise KeyError((cin, shape, v))


# ---------------------------------------------------------------------------------------------------------------------------------
def test_every_listed_instantiation_has_a_case():
    pe = [f"patch_embed_kernel<{nt},{ntok}>" for nt in (1, 2, 3, 4) for ntok in (32, 64, 128)] + ["im2col_patch_kernel"]
    assert len(pe) == 13 and sorted(pe) == CC.pe_instantiations()
    conv = ["conv3x3s2_mfma_kernel<4,16,4,1,false>", "conv3x3s2_mfma_kernel<16,64,4,1,false>", "conv3x3s2_mfma_kernel<16,64,4,1,true>",
            "conv3x3s2_mfma_kernel<64,256,2,4,false>", "conv3x3s2_mfma_kernel<64,256,2,4,true>"]
    assert sorted(conv) == CC.conv_instantiations() == sorted({c["expect"] for c in CC.CONV_RANDOM})
    assert CC.th_instantiations() == ["token_mlp3_kernel"]
    ids = [CC.pe_id(c) for c in CC.PE_CASES] + [CC.conv_id(c) for c in CC.CONV_EXACT]
    assert len(set(ids)) == len(ids)


def test_shapes_reach_their_paths():
    small = {(c["E"], c["S"]) for c in CC.PE_SMALL}
    assert small == {(E, S) for E in (8, 32, 33, 64, 96, 97, 112, 128) for S in (128, 256, 512)}
    assert all(c["B"] == 2 and c["per_row"] == 1 and c["trips"] == 1 for c in CC.PE_SMALL)
    assert {E: CC.pe_nt(E) for E in (8, 32, 33, 64, 96, 97, 112, 128)} == {8: 1, 32: 1, 33: 2, 64: 2, 96: 3, 97: 4, 112: 4, 128: 4}
    assert [(c["S"], CC.pe_ntok(c["S"]), c["per_row"]) for c in CC.PE_INTERIOR] == [(384, 32, 3), (768, 64, 3), (1536, 128, 3)]
    assert [c["n_seg"] for c in CC.PE_WRAP] == [1056, 1088, 1152, 2080] and [c["trips"] for c in CC.PE_WRAP] == [2, 2, 2, 3]
    assert all(c["n_seg"] % CC.PE_GRID for c in CC.PE_WRAP), "the last trip is taken by some workgroups only"
    assert [(c["n_seg"], c["trips"], c["E"]) for c in CC.PE_PRODUCT] == [(2048, 2, 96), (2048, 2, 112)]
    for c in CC.IM2COL_CASES:
        assert (c["S"] // 4) % 32 != 0
    assert [c["B"] * (c["S"] // 4) ** 2 * 20 > CC.IM2COL_GRID for c in CC.IM2COL_CASES] == [False, False, False, True]
    # conv: the dispatch edge on both sides, one pixel, and a workgroup count with quotient and remainder
    Ms = [CC.conv_M(*s) for s in CC.CONV_SHAPES]
    assert Ms == [1, 30, 32, 33, 1089]
    for cin, bm in ((4, 128), (16, 128), (64, 64)):
        n = CC.cdiv(1089, bm)
        assert n // 8 > 0 and n % 8 > 0 and 1089 % bm and (66 // 2) % 2 == 1
        order = CC.xcd_tile_order(torch.arange(n), n).tolist()
        assert sorted(order) == list(range(n)) and order != list(range(n))
    assert CC.TH_OUT_DIM == (1, 4, 8, 9, 32, 256) and len(set(CC.TH_TOK)) < CC.TH_G and list(CC.TH_TOK) != sorted(CC.TH_TOK)


def test_conv_impulses_meet_every_k_border_parity_class_and_seam():
    for key in CC.conv_instantiations():
        cin = int(key.split("<")[1].split(",")[0])
        ks, facts = CC.conv_coverage(key)
        assert ks == set(range(9 * cin)), (key, sorted(set(range(9 * cin)) - ks))
        assert {"sees1", "sees2", "sees4", "top", "bottom", "left", "right"} <= facts, (key, facts)
        assert "seam" in facts or all(c["B"] == 1 for c in CC.CONV_EXACT if c["expect"] == key), key
        seen = set()
        for c in CC.CONV_EXACT:                                          # the same, from the operands themselves
            if c["expect"] == key and (c["M"] <= 64):
                seen |= CC.conv_exact(c)["ks_hit"]
        big = [c for c in CC.CONV_EXACT if c["expect"] == key and c["M"] > 64]
        for c in big:
            seen |= CC.conv_exact(c)["ks_hit"]
        assert seen == ks, key


# ---------------------------------------------------------------------------------------------------------------------------------
# patch embedding
@pytest.mark.parametrize("c", [c for c in CC.PE_SMALL if c["S"] == 128 or (c["S"], c["E"]) in ((256, 33), (512, 8))], ids=CC.pe_id)
def test_pe_exact_pass(c):
    X = CC.pe_exact(c)
    assert bool((X["wp"][c["E"]:] == 0).all()) and bool((X["wp"].view(-1, 22, 8)[:, :, 0] == 0).all()) and bool((X["wp"].view(-1, 22, 8)[:, 21] == 0).all())
    want = torch.nn.functional.conv2d(X["img"], X["w"], X["bias"], stride=4, padding=3).permute(0, 2, 3, 1).reshape(-1, c["E"])
    assert torch.equal(want, X["pre"])
    segs = None if c["S"] == 128 else [0, 1, c["n_seg"] // 2 - 1, c["n_seg"] // 2, c["n_seg"] - 1]
    for op16 in OP16S:
        for with_pos in (True, False):
            assert CC.pe_verdict(CC.pe_restate(X, op16, with_pos, segs=segs), X, with_pos) is None, (op16, with_pos)


def test_pe_interior_and_wrap_segments():
    c = pe_find("interior", 384)
    X = CC.pe_exact(c)
    assert CC.pe_verdict(CC.pe_restate(X, torch.float16, segs=[0, 1, 2, 3 * 50 + 1, c["n_seg"] - 2, c["n_seg"] - 1]), X) is None
    c = pe_find("wrap", 128, B=65)
    X = CC.pe_exact(c)
    assert CC.pe_verdict(CC.pe_restate(X, torch.bfloat16, segs=[0, 1023, 1024, 2047, 2048, 2079]), X) is None


PE_DEFECT_CASES = {
    "the zero tap placed behind instead of in front": (pe_find("small", 128, 8), None),
    "a window starting at column 4 t + 4": (pe_find("small", 128, 33), None),
    "x < 0 not zeroed": (pe_find("small", 128, 96), None),
    "y < 0 not zeroed": (pe_find("small", 128, 32), None),
    "the position row taken with the batch offset": (pe_find("small", 128, 64), None),
    "a wave with 32 wave >= NTOK storing": (pe_find("small", 128, 97), None),
    "the second trip computed from the first trip's registers": (pe_find("wrap", 128, B=33), [5, 1023, 1024, 1055]),
    "a channel n >= E stored": (pe_find("small", 128, 33), None),
    "the bias one 32-tile off": (pe_find("small", 128, 112), None),
    "the + 4 h dropped": (pe_find("small", 128, 128), None),
}
PE_SENTINEL = {"a wave with 32 wave >= NTOK storing", "a channel n >= E stored"}


def test_every_defect_has_a_case():
    assert sorted(PE_DEFECT_CASES) == sorted(CC.PE_DEFECTS) and len(CC.PE_DEFECTS) == 10
    assert sorted(CONV_DEFECT_CASES) == sorted(CC.CONV_DEFECTS) and len(CC.CONV_DEFECTS) == 8
    assert sorted(TH_DEFECT_CASES) == sorted(CC.TH_DEFECTS) and len(CC.TH_DEFECTS) == 4


@pytest.mark.parametrize("defect", CC.PE_DEFECTS)
def test_pe_defect_is_caught(defect):
    c, segs = PE_DEFECT_CASES[defect]
    X = CC.pe_exact(c)
    for op16 in OP16S:
        assert CC.pe_verdict(CC.pe_restate(X, op16, segs=segs), X) is None
        got = CC.pe_verdict(CC.pe_restate(X, op16, defect=defect, segs=segs), X)
        assert got == ("sentinel" if defect in PE_SENTINEL else "bits"), (defect, CC.pe_id(c), op16, got)
    if defect == "the position row taken with the batch offset":       # without a table that defect is none: the null-pos launch cannot see it
        assert CC.pe_verdict(CC.pe_restate(X, torch.float16, False, defect=defect), X, False) is None


def test_pe_right_and_bottom_padding_never_occur():
    """Conv2d(k7, s4, p3) on S % 4 == 0 pads on the left and on top only: the kernel's `x < S` and `y < S` tests are dead, and the issue's
    defect "x >= S not zeroed" is none -- its live mirror "x < 0 not zeroed" is in the list instead"""
    for c in CC.PE_SMALL[:3] + [pe_find("interior", 384)]:
        So, nt = c["S"] // 4, CC.pe_ntok(c["S"])
        assert 4 * (So - nt) - 4 + 4 * nt + 3 == c["S"] - 1 and 4 * (So - 1) - 3 + 6 == c["S"] - 1
    X = CC.pe_exact(pe_find("small", 128, 96))
    for dead in CC.PE_DEAD_CHECKS:
        assert CC.pe_verdict(CC.pe_restate(X, torch.float16, defect=dead), X) is None


def test_pe_token_order_of_the_restatement():
    c = pe_find("small", 128, 33)
    X = CC.pe_random(c, torch.float16)
    out, written, outside, _ = CC.pe_restate(X, torch.float16)
    out2 = CC.pe_restate(CC.swap_images(X, 0, 1), torch.float16)[0]
    n = out.numel() // 2
    assert outside == 0 and bool(written.all()) and torch.equal(out2[:n], out[n:]) and torch.equal(out2[n:], out[:n]) and not torch.equal(out[:n], out[n:])


@pytest.mark.parametrize("op16", OP16S)
def test_pe_random_bound_holds_for_the_restatement(op16):
    c = pe_find("small", 128, 97)
    X = CC.pe_random(c, op16)
    out = CC.pe_restate(X, op16)[0].view(-1, c["E"])
    bound = error_bound(X["Sabs"], 176, X["pre"], X["ref"])
    assert float(((out.double() - X["ref"]).abs() / bound).max()) < 1.0


@pytest.mark.parametrize("c", CC.IM2COL_CASES[:3], ids=lambda c: f"b{c['B']}-s{c['S']}")
def test_im2col_restatement_is_unfold(c):
    g = torch.Generator().manual_seed(c["S"])
    img = torch.randn(c["B"], 3, c["S"], c["S"], generator=g)
    for op16 in OP16S:
        got = CC.im2col_restate(img, op16)
        cols = torch.nn.functional.unfold(img.to(op16).float(), 7, padding=3, stride=4).transpose(1, 2).reshape(-1, 147)
        assert torch.equal(got[:, :147].float(), cols) and bool((got[:, 147:] == 0).all()) and got.shape[1] == 160


# ---------------------------------------------------------------------------------------------------------------------------------
# implicit-GEMM convolution
@pytest.mark.parametrize("c", [c for c in CC.CONV_EXACT if c["v"] < 2], ids=CC.conv_id)
def test_conv_exact_pass(c):
    E = CC.conv_exact(c)
    K = 9 * c["cin"]
    assert bool((E["Wp"][:, K:E["KP"]] == 0).all()) and bool(torch.isnan(E["Wp"][:, E["KP"]:]).all())
    x = E["X"].permute(0, 3, 1, 2)
    w = E["Wp"][:, :K].reshape(-1, 3, 3, c["cin"]).permute(0, 3, 1, 2)
    pre = torch.nn.functional.conv2d(x, w, E["bias"], stride=2, padding=1).permute(0, 2, 3, 1).reshape(c["M"], -1)
    assert torch.equal(pre, E["pre"])
    for op16 in OP16S:
        rows, y16 = CC.conv_restate(E, op16)
        assert CC.conv_verdict(rows, y16, E, op16) is None, op16


CONV_DEFECT_CASES = {
    "ky and kx exchanged": [conv_find(4, (2, 6, 10)), conv_find(64, (1, 6, 22))],
    "a window origin of 2 o instead of 2 o - 1": [conv_find(16, (2, 8, 8)), conv_find(4, (1, 66, 66))],
    "a clamped border tap not zeroed": [conv_find(4, (1, 2, 2)), conv_find(16, (2, 6, 10))],
    "b derived with Wo in place of Ho": [conv_find(16, (2, 6, 10)), conv_find(64, (2, 6, 10))],
    "the two taps of a lane half exchanged at CIN = 4": [conv_find(4, (2, 8, 8))],
    "k >= 9 CIN not zeroed": [conv_find(4, (1, 66, 66))],
    "rows past M stored": [conv_find(4, (2, 6, 10)), conv_find(64, (1, 66, 66))],
    "two column quarters exchanged at WC = 4": [conv_find(64, (2, 8, 8)), conv_find(64, (1, 6, 22))],
}
CONV_SENTINEL = {"rows past M stored"}


@pytest.mark.parametrize("defect", CC.CONV_DEFECTS)
def test_conv_defect_is_caught(defect):
    for c in CONV_DEFECT_CASES[defect]:
        E = CC.conv_exact(c)
        for op16 in OP16S:
            got = CC.conv_verdict(*CC.conv_restate(E, op16, defect=defect), E, op16)
            assert got == ("sentinel" if defect in CONV_SENTINEL else "bits"), (defect, CC.conv_id(c), op16, got)


def test_conv_zero_fill_is_guarded_twice():
    """what the exact pass cannot see and why: with the weight's columns 9 CIN .. KP zero by contract and both operands zeroed past KP,
    dropping the zeroing of ONE operand changes nothing -- the defect of the list drops both"""
    E = CC.conv_exact(conv_find(4, (2, 8, 8)))
    assert CC.conv_verdict(*CC.conv_restate(E, torch.float16), E, torch.float16) is None
    # a whole-row scale is invisible behind the LayerNorm: pass 2's float64 comparison and the three-launch bits see it
    E2 = dict(E, X=E["X"] * 2)
    rows, y16 = CC.conv_restate(E2, torch.float16)
    hit = E["patches_hit"][rows]
    assert torch.equal(y16[~hit], E["y"].to(torch.float16)[rows][~hit]) and not torch.equal(y16[hit], E["y"].to(torch.float16)[rows][hit])


# ---------------------------------------------------------------------------------------------------------------------------------
# token heads
TH_DEFECT_CASES = {
    "another head's token": (1, False),
    "layer-3 rows >= out_dim written": (1, False),
    "a packed row stride of out_dim instead of out_ld": (3, True),
    "the activation buffer parity exchanged": (3, False),
}
TH_SENTINEL = {"layer-3 rows >= out_dim written"}


@pytest.mark.parametrize("B", CC.TH_B)
def test_th_exact_pass(B):
    X = CC.th_exact(B)
    for gi, od in enumerate(CC.TH_OUT_DIM):
        assert bool((X["Ws"][2][gi, od:] == 0).all())
        h = X["hs"][:, CC.TH_TOK[gi]]
        for layer in range(3):
            pre = h @ X["Ws"][layer][gi].t() + X["bs"][layer][gi]
            assert torch.equal(pre, X["pres"][layer][:, gi])
            h = pre.clamp_min(0)
    for packed in (False, True):
        res = CC.th_restate(X, packed)
        assert CC.th_verdict(res, X, packed) is None and torch.equal(res[2], CC.th_expected(X, packed)[1])
    off, ld, total = CC.th_packed_layout(B)
    assert all(l > od for l, od in zip(ld, CC.TH_OUT_DIM)) and all(off[g + 1] == off[g] + B * ld[g] + 2 for g in range(5))


@pytest.mark.parametrize("defect", CC.TH_DEFECTS)
def test_th_defect_is_caught(defect):
    B, packed = TH_DEFECT_CASES[defect]
    X = CC.th_exact(B)
    got = CC.th_verdict(CC.th_restate(X, packed, defect=defect), X, packed)
    want = ("sentinel", "bits") if "packed" in defect else (("sentinel",) if defect in TH_SENTINEL else ("bits",))
    assert got in want, (defect, got)
    if defect == "layer-3 rows >= out_dim written":                     # the packed form loses its pad columns and the sentinel behind a region
        assert CC.th_verdict(CC.th_restate(X, True, defect=defect), X, True) == "sentinel"


@pytest.mark.parametrize("op16", OP16S)
def test_th_random_bound_holds_for_the_restatement(op16):
    X = CC.th_random(3, op16)
    out, written, allowed = CC.th_restate(X, False)
    want, _ = CC.th_expected(X, False)
    bound = CC.th_bound(X, error_bound)
    assert bound.shape == X["ref"].shape
    ratio = ((out.double() - want).abs().view(3, CC.TH_G, CC.TH_C) / bound)[allowed.view(3, CC.TH_G, CC.TH_C)]
    assert float(ratio.max()) < 1.0
