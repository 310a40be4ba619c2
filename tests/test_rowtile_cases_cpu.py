"""The variant matrix of the full-row kernels (tests/test_rowtile_variants_gpu.py) must be able to fail.  On the CPU:
  1. the case tables cover the literal list of five instantiations and the shapes reach the paths they are there for (tile boundaries,
     xcd_tile_order with quotient and remainder, prefetch places above 0, a grid that wraps);
  2. every exact builder meets the conditions it asserts, its operands are exact in fp16 and in bf16, and the fp32 restatement of the tile
     walk (rowtile_cases.restate) gives the expected bits of C32 and Y16 in both operand types;
  3. every simulated defect of rowtile_cases.DEFECTS changes the exact pass of a named case of the table, or stores outside the output;
  4. the float64 references agree with a plain torch evaluation, and the random pass's bounds hold for the fp32 restatement.
The two large row counts are restated on the workgroups they are there for (the first, the ones past 256, the ragged last tile)."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowtile_cases as RC  # noqa: E402
from test_gemm_variants_gpu import error_bound  # noqa: E402

OP16S = (torch.float16, torch.bfloat16)


def find(kind, K, M, N=None, splits=None, bias=None):
    """the first case of the table with these fields"""
    for c in RC.CASES:
        if (c["kind"] == kind and c["K"] == K and c["M"] == M and (N is None or c["N"] == N) and (splits is None or c["splits"] == splits)
                and (bias is None or c["bias"] == bias)):
            return c
    raise KeyError((kind, K, M, N, splits, bias))


def test_tables_cover_the_five_instantiations():
    want = ["gemm_rowln_kernel<384,0>", "gemm_rowln_kernel<256,0>", "gemm_rowln_kernel<256,64>", "gemm_rowln_kernel<256,256>",
            "mlp_rowln_kernel<384,0>"]
    assert sorted(want) == RC.instantiations()
    ids = [RC.case_id(c) for c in RC.CASES]
    assert len(set(ids)) == len(ids)
    for key in want:
        mine = [c for c in RC.CASES if c["expect"] == key]
        assert {c["M"] for c in mine} == set(RC.SMALL_M) | set(RC.LARGE_M), key
        assert {c["bias"] for c in mine} == {True, False}, key
        big = [c for c in mine if c["large"]]
        assert len(big) == 2 and all(c["K"] == max(d["K"] for d in mine) for c in big), "the large counts run once, at the largest K / D / H"
    assert {c["K"] for c in RC.PLAIN_CASES if c["N"] == 384} == {64, 128, 384, 1536}
    assert {c["K"] for c in RC.PLAIN_CASES if c["N"] == 256} == {64, 256, 2048}
    assert {c["K"] for c in RC.MLP_CASES} == {128, 256, 1536}
    for D in (64, 256):
        for M in RC.SMALL_M:
            assert {c["splits"] for c in RC.MERGED_CASES if c["K"] == D and c["M"] == M} == {2, 3, 4, 5, 7, 8}
        for s in RC.SPLITS:
            assert {c["bias"] for c in RC.MERGED_CASES if c["K"] == D and c["splits"] == s} == {True, False}
    assert {c["splits"] for c in RC.MERGED_CASES if c["large"]} == {5, 8}


def test_shapes_reach_their_paths():
    assert {63, 64, 65, 127} <= set(RC.SMALL_M) and RC.PERM_M % RC.BM
    n = RC.cdiv(1089, 64)
    assert n == 18 and (n // 8, n % 8) == (2, 2) and RC.prefetch_places(n) == [0, 1, 2]
    n = RC.cdiv(16901, 64)
    assert n == 265 > RC.GRID_WRAP and 16901 - 264 * 64 == 5 and RC.prefetch_places(n) == list(range(32))
    assert (264 >> 3) & 31 == 1, "workgroup 264's place has wrapped"
    for n in (1, 4, 18, 265):
        assert sorted(RC.xcd_tile_order(torch.arange(n), n).tolist()) == list(range(n))
    assert RC.xcd_tile_order(torch.arange(18), 18).tolist() != list(range(18))


# ---------------------------------------------------------------------------------------------------------------------------------
SMALL = [c for c in RC.CASES if not c["large"] and c["M"] in (1, 65, 127, 200) and (c["K"] <= 384 or c["M"] == 65)]


@pytest.mark.parametrize("c", SMALL, ids=RC.case_id)
def test_exact_pass(c):
    E = RC.exact(c)                                              # (the builder asserts its own conditions)
    ops16 = ("A", "W", "W1", "W2", "y", "hid")
    assert all(RC.exact16(E[k]) for k in ops16 if E.get(k) is not None)
    assert all(bool((E[k].float().double() == E[k]).all()) for k in ("x", "R", "b", "b1", "ln_w", "ln_b") if E.get(k) is not None)
    if c["M"] > 1:
        assert torch.unique(E["x"], dim=0).shape[0] == c["M"], "two target rows of the case are equal"
        assert float(E["x"].mean(1).max()) == 1000.0
    for op16 in OP16S:
        rows, c32, y16 = RC.restate(E, op16)
        assert RC.verdict(rows, c32, y16, E, op16) is None, op16


def test_merged_patterns_are_all_there():
    for S in RC.SPLITS:
        for M in (1, 65, 200):
            st = RC.split_states(M, S)
            live = st == RC.LIVE
            assert int(live[:, M - 1].sum()) == 1, "row M - 1 is a single-live row"
            if M < 65:
                continue
            n = live.sum(0)
            assert bool((n == S).any()) and bool((live[0] & (n == 1)).any()) and bool((live[S - 1] & (n == 1)).any())
            assert bool((st == RC.EMPTY).any()) and bool((st == RC.DEAD).any())
            if S >= 5:
                assert bool((live[4] & (n == 1)).any()), "only split 4 live: the first one the upper branch loads"
            alt = (st != RC.EMPTY).all(0) & (st == RC.DEAD).any(0) & (n > 1 if S > 2 else n >= 1)
            assert bool(alt.any()), "live and dead alternating"


# (the builders of the 16901-row cases at K = 2048 / D = 256 take seconds on the CPU: the GPU file builds them on the device)
@pytest.mark.parametrize("c", [c for c in RC.CASES if c["large"] and (c["M"] == 1089 or (c["kind"], c["K"]) in (("merged", 64), ("mlp", 1536)))],
                         ids=RC.case_id)
def test_large_counts_on_their_workgroups(c):
    E = RC.exact(c)
    n = RC.cdiv(c["M"], RC.BM)
    last = int((RC.xcd_tile_order(torch.arange(n), n) == n - 1).nonzero())            # the workgroup that owns the ragged last tile
    blocks = sorted({0, 9, n - 1, last} | ({256, 257, 263} if n > 256 else set()))
    rows, c32, y16 = RC.restate(E, torch.float16, blocks=blocks)
    assert c["M"] - 1 in rows.tolist() and len(rows) < len(blocks) * RC.BM, "the ragged last tile is among them"
    assert RC.verdict(rows, c32, y16, E, torch.float16, whole=False) is None


# ---------------------------------------------------------------------------------------------------------------------------------
# defect -> the cases that must see it, and what the GPU file would see
D = RC.DEFECTS
DEFECT_CASES = {
    "two column quarters exchanged": [find("plain", 64, 1, N=384), find("mlp", 128, 63)],
    "the + 4 h term of the accumulator row map dropped": [find("plain", 64, 63, N=256), find("merged", 64, 65, splits=4)],
    "bias one 32-block off": [find("plain", 256, 64, N=256, bias=True), find("mlp", 128, 1, bias=True)],
    "residual read from the clamped row instead of the own row": [find("plain", 128, 127, N=384), find("mlp", 256, 200)],
    "rows past M stored": [find("mlp", 128, 65), find("plain", 2048, 127)],
    "Y16 computed from the pre-residual value": [find("merged", 64, 63, splits=2), find("plain", 1536, 65)],
    "mean taken over N + 4 (the tile's padding columns)": [find("plain", 64, 200, N=256), find("mlp", 256, 1)],
    "a k-step served from the other ring slot": [find("plain", 128, 64, N=384), find("merged", 256, 65, splits=3)],
    "the last k-step skipped when nk is odd": [find("plain", 64, 65, N=256), find("merged", 64, 127, splits=7)],
    "chunk c using chunk c - 1's b1": [find("mlp", 256, 65, bias=True)],
    "chunk c using chunk c - 1's W1": [find("mlp", 256, 65, bias=False), find("mlp", 1536, 65, bias=True)],
    "fc2's second half reading hidden image 0 again": [find("mlp", 128, 1)],
    "hidden units of the two lane halves exchanged": [find("mlp", 128, 63)],
    "the upper four splits not loaded at splits = 5": [find("merged", 64, 65, splits=5), find("merged", 256, 200, splits=5)],
    "the u < splits test dropped": [find("merged", 64, 64, splits=3), find("merged", 256, 65, splits=5), find("merged", 64, 200, splits=7)],
    "an empty split not skipped": [find("merged", 64, 63, splits=2), find("merged", 256, 127, splits=8)],
    "a dead split given weight l instead of l e": [find("merged", 64, 127, splits=4), find("merged", 256, 65, splits=2)],
    "the split stride taken as 64 rows instead of M": [find("merged", 256, 65, splits=8), find("merged", 64, 200, splits=3)],
}
SENTINEL = {"rows past M stored"}


def test_every_defect_has_a_case():
    assert sorted(DEFECT_CASES) == sorted(D) and len(D) == 18


@pytest.mark.parametrize("defect", D)
def test_defect_is_caught(defect):
    for c in DEFECT_CASES[defect]:
        E = RC.exact(c)
        for op16 in OP16S:
            got = RC.verdict(*RC.restate(E, op16, defect=defect), E, op16)
            assert got == ("sentinel" if defect in SENTINEL else "bits"), (defect, RC.case_id(c), op16, got)


def test_y16_only_defects_leave_c32_alone_and_the_clamp_defect_needs_a_ragged_tile():
    for defect in ("Y16 computed from the pre-residual value", "mean taken over N + 4 (the tile's padding columns)"):
        E = RC.exact(DEFECT_CASES[defect][0])
        rows, c32, y16 = RC.restate(E, torch.bfloat16, defect=defect)
        assert torch.equal(c32, E["x"].float()[rows]) and not torch.equal(y16, E["y"].to(torch.bfloat16)[rows])
    # the padding-column mean shows on the row with m = 1000 in every element
    E = RC.exact(find("plain", 64, 200, N=256))
    rows, c32, y16 = RC.restate(E, torch.float16, defect="mean taken over N + 4 (the tile's padding columns)")
    bad = (y16 != E["y"].to(torch.float16)[rows]).all(1)
    assert bool(bad[E["x"].mean(1)[rows] == 1000].all())
    # a row count of whole tiles has no clamped row: that defect needs the ragged cases
    E = RC.exact(find("plain", 128, 64, N=384))
    assert RC.verdict(*RC.restate(E, torch.float16, defect="residual read from the clamped row instead of the own row"), E, torch.float16) is None


def test_token_order_of_the_restatement():
    for c in (find("plain", 256, RC.PERM_M, N=256), find("merged", 64, RC.PERM_M, splits=5), find("mlp", 256, RC.PERM_M)):
        E = RC.random(c, torch.float16)
        perm = torch.randperm(c["M"], generator=torch.Generator().manual_seed(9))
        rows, c32, y16 = RC.restate(E, torch.float16)
        rows2, c2, y2 = RC.restate(RC.permute_rows(E, perm), torch.float16)
        assert torch.equal(rows, rows2) and torch.equal(rows, torch.arange(c["M"]))
        assert torch.equal(c2.view(torch.int32), c32[perm].view(torch.int32)) and torch.equal(y2.view(torch.int16), y16[perm].view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------------------------
def test_float64_references_agree_with_plain_torch():
    F = torch.nn.functional
    c = find("plain", 256, 65, N=256, bias=True)
    E = RC.random(c, torch.float16)
    assert torch.allclose(E["ref"], F.linear(E["A"], E["W"], E["b"]) + E["R"], rtol=1e-13, atol=1e-13)
    assert torch.allclose(RC.layernorm64(E["ref"], E["ln_w"], E["ln_b"], 1e-5), F.layer_norm(E["ref"], (256,), E["ln_w"], E["ln_b"], 1e-5),
                          rtol=1e-10, atol=1e-10)
    ref, bound = RC.next_norm_reference(E["ref"].float(), E["ln_w"], E["ln_b"], 1e-5, torch.float16)
    assert torch.allclose(ref, F.layer_norm(E["ref"].float().double(), (256,), E["ln_w"], E["ln_b"], 1e-5), rtol=1e-10, atol=1e-10)
    c = find("mlp", 256, 65, bias=True)
    E = RC.random(c, torch.bfloat16)
    want = F.linear(F.gelu(F.linear(E["A"], E["W1"], E["b1"])), E["W2"], E["b"]) + E["R"]
    assert torch.allclose(E["ref"], want, rtol=1e-12, atol=1e-12)
    assert abs(float(E["ref"][1].mean()) - 1000) < 5 and float(E["ref"][-1].std()) < 1e-6, "the mean = 1000 std row and the near-constant row"
    c = find("merged", 64, 65, splits=5)
    E = RC.random(c, torch.float16)
    part, mx, sm = E["part"], E["mx"], E["sm"]
    for row in (0, 3, 64):
        num, den, top = torch.zeros(64, dtype=torch.float64), 0.0, max(float(mx[u, row]) for u in range(5))
        for u in range(5):
            if float(mx[u, row]) != -math.inf:
                w = float(sm[u, row]) * 2.0 ** (float(mx[u, row]) - top)
                num, den = num + w * part[u, row], den + w
        assert torch.allclose(RC.merge_reference(part, mx, sm)[row], num / den, rtol=1e-13, atol=1e-15)
    assert bool(torch.isnan(part).any()) and bool(torch.isfinite(E["ref"]).all())
    for op16, vals in ((torch.float16, (1.0, 1.5, 1e-6, 0.0)), (torch.bfloat16, (1.0, 3.0, 0.3))):
        for v in vals:
            t = torch.tensor([v], dtype=torch.float64)
            up = torch.nextafter(t.to(op16), torch.tensor([math.inf]).to(op16)).double() - t.to(op16).double()
            assert float(RC.ulp16(t.to(op16).double(), op16)) == float(up) or v == 0.0, (op16, v)
    assert float(RC.ulp16(torch.zeros(1, dtype=torch.float64), torch.float16)) == 2.0 ** -24


@pytest.mark.parametrize("c", [find("plain", 384, 65, N=384), find("plain", 2048, 65), find("merged", 64, 65, splits=4), find("merged", 256, 65, splits=7),
                               find("mlp", 128, 65), find("mlp", 1536, 65)], ids=RC.case_id)
def test_random_bounds_hold_for_the_fp32_restatement(c):
    """the bounds the GPU file applies, on the restated walk: error_bound() (merged: widened by one 16-bit ulp of A times |W|) or the MLP's
    6e-3 + 4e-3 |ref| (4 x that under bf16) for C32, next_norm_reference for Y16"""
    for op16, f in ((torch.float16, 1.0), (torch.bfloat16, 4.0)):
        E = RC.random(c, op16)
        rows, c32, y16 = RC.restate(E, op16)
        assert torch.equal(rows, torch.arange(c["M"]))
        if c["kind"] == "mlp":
            bound = f * 6e-3 + f * 4e-3 * E["ref"].abs()
        else:
            bound = error_bound(E["S"], c["K"], E["pre"], E["ref"], fp16=op16 == torch.float16) + E.get("widen", 0.0)
        ratio = float(((c32.double() - E["ref"]).abs() / bound).max())
        yref, ybound = RC.next_norm_reference(c32, E["ln_w"], E["ln_b"], E["eps"], op16)
        yratio = float(((y16.double() - yref).abs() / ybound).max())
        assert ratio < 1.0 and yratio < 1.0, (op16, ratio, yratio)
