"""CPU companion of tests/test_dectok_variants_gpu.py: the builders of tests/dectok_cases.py hold their exactness conditions in fp16 and in
bf16, the fp32 restatement of the four token kernels gives the expected bits, every simulated defect of DEFECTS fails a named case and no
case is blind, the fp32 LayerNorm bound holds over reordered sums, the swapped-eps reference lies outside the bounded pass's bound, and the
producer table reaches every MAXS under the launcher's formula.  No GPU, no library."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dectok_cases as DC  # noqa: E402

OP16 = (torch.float16, torch.bfloat16)
_E = {}


def built(kind, c):
    key = (kind,) + tuple(c)
    if key not in _E:
        _E[key] = {"self": DC.self_exact, "tail": DC.tail_exact, "mlp": DC.mlp_exact}[kind](*c)
    return _E[key]


def cid(kc):
    kind, c = kc
    return kind + "-" + "-".join(str(int(v)) if not isinstance(v, bool) else ("y" if v else "n") for v in c)


def test_case_tables():
    assert all(1 <= T <= DC.MAXT and B * T <= DC.MAXR for B, T in DC.SHAPES)
    assert {(1, 1), (32, 1), (16, 2), (10, 3), (1, 7), (4, 8), (3, 9), (2, 15), (1, 16), (2, 16)} == set(DC.SHAPES)
    assert DC.KERNELS == ["dec_self_kernel", "dec_mlp_kernel", "dec_kv_kernel", "dec_tail_kernel", "attn_fewq16_part_kernel<1>",
                          "attn_fewq16_part_kernel<2>", "attn_fewq16_part_kernel<4>", "attn_fewq16_part_kernel<8>"]
    # every shape: both skip values, inner and last block, rows and partials; every split count 1 .. 8 somewhere
    assert len(DC.SELF_CASES) == 20 and len(DC.MLP_CASES) == 60 and len(DC.TAIL_CASES) == 30
    assert {s for *_, s in DC.MLP_CASES} == set(range(9)) == {s for *_, s in DC.TAIL_CASES}


def test_producer_table_reaches_every_maxs_and_leaves_empty_splits():
    # msam2_attention_fewq_keysplit: steps = cdiv(cdiv(cdiv(Lk, splits), 16), 32); <1> up to 1, <2> up to 2, <4> up to 4, else <8>
    def maxs(Lk, S):
        per_split = -(-Lk // S)
        per_wave = -(-per_split // 16)
        steps = -(-per_wave // 32)
        return 1 if steps <= 1 else 2 if steps <= 2 else 4 if steps <= 4 else 8
    want = {(1, 1): 1, (1, 8): 1, (9, 8): 1, (33, 2): 1, (100, 8): 1, (512, 1): 1, (513, 1): 2, (1025, 1): 4, (2049, 1): 8, (4096, 1): 8,
            (4096, 2): 4, (4096, 4): 2, (4096, 8): 1, (4095, 3): 4}
    assert set(DC.PRODUCER) == set(want)
    for (Lk, S), m in want.items():
        assert maxs(Lk, S) == m == DC.part_maxs(Lk, S), (Lk, S)
        assert Lk <= 16 * 32 * m * S
    assert {DC.part_maxs(*c) for c in DC.PRODUCER} == {1, 2, 4, 8}
    empty = {c: sum(hi <= lo for lo, hi in DC.split_ranges(*c)) for c in DC.PRODUCER}
    assert empty[(1, 8)] == 7 and empty[(9, 8)] == 3 and empty[(33, 2)] == 0 and empty[(4095, 3)] == 0
    assert DC.split_ranges(33, 2) == [(0, 17), (17, 33)] and DC.split_ranges(4095, 3)[-1] == (2730, 4095)
    assert set(DC.LQ) == {1, 7, 16, 32} and all(DC.producer_batch(q) * q <= 32 for q in DC.LQ)


EXACT = ([("self", c) for c in DC.SELF_CASES] + [("tail", c) for c in DC.TAIL_CASES] + [("mlp", c) for c in DC.MLP_CASES])


@pytest.mark.parametrize("kc", EXACT, ids=cid)
def test_builder_conditions_and_restatement(kc):
    """the builder's own assertions (they run inside it) and: the fp32 walk of the kernels gives the expected bits in both operand types"""
    E = built(*kc)
    for op16 in OP16:
        assert DC.verdict(DC.restate(E, op16), E, op16) is None, (cid(kc), op16)


# ---- the defects: which kernels a defect lives in, and the named case that must see it
APPLIES = {1: ("self",), 2: ("mlp",), 3: ("mlp",), 4: ("self",), 5: ("self",), 6: ("self",), 7: ("self",), 8: ("self",), 9: ("self", "tail", "mlp"),
           10: ("self",), 11: ("mlp",), 12: ("mlp",), 13: ("mlp",), 14: ("mlp",), 15: ("mlp",), 16: ("self", "mlp"), 17: ("tail", "mlp"),
           18: ("tail", "mlp"), 19: ("tail", "mlp"), 20: ("tail", "mlp"), 21: ("mlp",), 22: ("self", "tail", "mlp")}
NAMED = {1: ("self", (3, 9, False)), 2: ("mlp", (3, 9, False, 0)), 3: ("mlp", (3, 9, True, 0)), 4: ("self", (3, 9, True)), 5: ("self", (3, 9, True)),
         6: ("self", (10, 3, False)), 7: ("self", (16, 2, False)), 8: ("self", (1, 1, False)), 9: ("tail", (2, 15, 0)), 10: ("self", (1, 7, False)),
         11: ("mlp", (1, 7, False, 0)), 12: ("mlp", (1, 7, False, 0)), 13: ("mlp", (32, 1, False, 0)), 14: ("mlp", (1, 1, False, 0)),
         15: ("mlp", (2, 15, False, 0)), 16: ("self", (2, 15, False)), 17: ("tail", (32, 1, 2)), 18: ("tail", (1, 7, 2)), 19: ("tail", (1, 7, 2)),
         20: ("tail", (1, 1, 1)), 21: ("mlp", (10, 3, False, 0)), 22: ("tail", (1, 16, 0))}
# the MLP walk is the slow one: its full defect list runs on these shapes, every other MLP case on the two cheapest of its defects
MLP_FULL = {(1, 1), (10, 3), (2, 15), (2, 16)}


@pytest.mark.parametrize("i", sorted(DC.D), ids=lambda i: f"defect{i}")
def test_defect_fails_its_named_case(i):
    kind, c = NAMED[i]
    assert kind in APPLIES[i] and (kind, c) in EXACT
    E = built(kind, c)
    for op16 in OP16:
        v = DC.verdict(DC.restate(E, op16, DC.D[i]), E, op16)
        print(f"defect {i} ({DC.D[i]}) on {cid((kind, c))}, {op16}: {v}")
        assert v is not None


def test_no_case_is_blind():
    """every case sees at least one defect of its kernels; every defect is seen in both operand types (above) and by most of its cases"""
    blind, seen_by = [], {i: 0 for i in DC.D}
    for kind, c in EXACT:
        E = built(kind, c)
        todo = [i for i in DC.D if kind in APPLIES[i]]
        if kind == "mlp" and (c[0], c[1]) not in MLP_FULL:
            todo = [14, 21]
        hits = [i for i in todo if DC.verdict(DC.restate(E, torch.bfloat16, DC.D[i]), E, torch.bfloat16) is not None]
        for i in hits:
            seen_by[i] += 1
        if not hits:
            blind.append(cid((kind, c)))
    print("cases that see each defect:", seen_by)
    assert not blind, f"blind cases: {blind}"
    assert all(n >= 4 for n in seen_by.values()), seen_by


def test_exact_pass_sees_what_the_old_bound_hides():
    """the defects the issue lists as hidden under 0.02 + 0.01 |ref| change BITS here: a restated run with `v reads x + pe` differs from
    the expected 16-bit qp in most rows"""
    E = built("self", (3, 9, False))
    got = DC.restated_outputs(E, torch.float16, DC.D[1])
    assert DC.bits_differ(got["qp"], E["qp"].to(torch.float16))


# ---- the fp32 LayerNorm bound
def _ln_orders(x32, w, b, eps):
    """fp32 LayerNorm with the two sums taken in several orders: sequential, reversed, pairwise (torch), 4 per lane then across lanes"""
    f = torch.float32
    n = x32.shape[1]
    seq = lambda v: v.cumsum(1)[:, -1:]
    orders = [seq, lambda v: seq(v.flip(1)), lambda v: v.sum(1, keepdim=True), lambda v: seq(v.view(-1, n // 4, 4).sum(2)),
              lambda v: seq(v[:, torch.randperm(n, generator=torch.Generator().manual_seed(3))])]
    for s in orders:
        mean = s(x32) / n
        d = x32 - mean
        rstd = 1.0 / torch.sqrt(s(d * d) / n + torch.tensor(eps, dtype=f))
        yield d * rstd * w.to(f) + b.to(f)


@pytest.mark.parametrize("kc", [("tail", (2, 16, 0)), ("self", (3, 9, False)), ("self", (3, 9, True)), ("mlp", (10, 3, True, 0))], ids=cid)
def test_ln_bound_holds_over_reordered_sums(kc):
    E = built(*kc)
    rows = [(E["pre"], E["ln_w"], E["ln_b"], E["eps"])] if kc[0] != "mlp" else [(E["pre2"], E["ln2_w"], E["ln2_b"], E["eps2"])]
    for pre, w, b, eps in rows:
        ref, bound = DC.ln_bound_exact(pre, w, b, eps)
        worst = max(float(((y.double() - ref).abs() / bound).max()) for y in _ln_orders(pre.float(), w, b, eps))
        print(f"{cid(kc)}: fp32 LayerNorm in five summation orders uses {worst:.3f} of ln_bound_exact")
        assert worst <= 1.0
        # and the bound is no wider than it has to be to see eps: the row of a = 1 / 4 moves by 1.6e-4 |g| without it
        assert float(bound.max()) < 2e-6
    if kc[0] == "mlp":                                       # norm3: the target row carries norm2's error delta
        ref, bound = DC.ln_bound(E["pre3"], E["ln3_w"], E["ln3_b"], E["eps3"], E["delta"])
        for sgn in (1.0, -1.0):
            pert = (E["pre3"] + sgn * E["delta"] * torch.sign(torch.randn(E["pre3"].shape, generator=torch.Generator().manual_seed(5)))).float()
            for y in _ln_orders(pert, E["ln3_w"], E["ln3_b"], E["eps3"]):
                assert bool(((y.double() - ref).abs() <= bound).all())
                assert bool(((y.double() - E["y3"]).abs() < 2.0 ** -11).all()), "norm3 stays inside half a 16-bit ulp of its integers"


# ---- synthetic partials and the producer's cases
@pytest.mark.parametrize("S", range(1, 9))
def test_synthetic_partials(S):
    for B, T in ((1, 1), (3, 9), (2, 16)):
        o, part, st = DC.partials_exact(B, T, S, DC.gen(7, B, T, S))
        # (float64 keeps the dead splits' weights 2^-200 that fp32 flushes to 0: 1e-57 of a value <= 1000)
        assert float((DC.merge_partials(part, B, T, S) - o).abs().max()) < 1e-50, "the float64 merge of the partials is the expected row"
        p = part.view(B * DC.NH, S, T, 18)
        m = p[..., 0]
        assert bool((p[..., 1:][torch.isinf(m)] == 0).all()), "an empty split is (-inf, 0, zeros): a NaN there would propagate"
        if S >= 2 and B * T > 4:
            assert {DC.LIVE, DC.EMPTY, DC.DEAD} == set(st.unique().tolist())
        for op16 in OP16:                                     # the consumers' merge restated, clamped loads included
            E = dict(B=B, T=T, splits=S, part=part, o=o)
            img = DC.load_attn_rows(E, op16)[:, :T].reshape(B * T, DC.CI)
            assert torch.equal(img.double(), o)


@pytest.mark.parametrize("Lk,S", DC.PRODUCER, ids=lambda v: str(v))
def test_producer_selection_cases(Lk, S):
    """the builder's conditions (inside it) and the expected partials against a float64 attention of every split on its own"""
    for Lq in DC.LQ:
        P = DC.producer_sel(Lq, Lk, S)
        B = P["B"]
        exp, state = P["exp"].view(B, DC.NH, S, Lq, 18), P["state"].view(B, DC.NH, S, Lq)
        c = DC.AC.LOG2E / math.sqrt(DC.DX)
        for s, (lo, hi) in enumerate(DC.split_ranges(Lk, S)):
            if hi <= lo:
                assert bool((state[:, :, s] == 0).all()) and bool((exp[:, :, s, :, 0] == -math.inf).all()) and bool((exp[:, :, s, :, 1:] == 0).all())
                continue
            sc = (P["q"] @ P["k"][:, :, lo:hi].transpose(2, 3)) * c
            m = sc.amax(-1)
            pr = torch.exp2(sc - m[..., None])
            l, O = pr.sum(-1), pr @ P["v"][:, :, lo:hi]
            tgt = state[:, :, s] == 2
            assert torch.equal(tgt, m == 0) and bool((m[~tgt] <= -DC.GAP).all())
            # (float64 keeps the other keys' 2^-204 that fp32 flushes to 0)
            if bool(tgt.any()):
                assert float((exp[:, :, s, :, 1][tgt] - l[tgt]).abs().max()) < 1e-50 and float((exp[:, :, s, :, 2:][tgt] - O[tgt]).abs().max()) < 1e-50
        assert bool(torch.isnan(exp.view(-1, 18)[P["state"] == 1]).all())
        tl = P["t"].unique().tolist()
        assert Lk - 1 in tl or any(b == Lk - 1 for _, b in P["pairs"]), "the last key is a target"
        assert 0 in tl


def test_producer_random_case_builds():
    for op16 in OP16:
        P = DC.producer_rand(7, 100, 8, op16)
        assert P["ref"].shape == (2, DC.NH, 7, DC.DX) and bool((P["bound"] > 0).all()) and bool(torch.isfinite(P["bound"]).all())


# ---- bounded pass
@pytest.mark.parametrize("op16", OP16, ids=str)
def test_bounded_references_hold_for_the_restatement_and_see_eps(op16):
    """the fp32 restatement lies inside every stage's bound; with low-variance rows (eps2 = 1e-3, eps3 = 1e-6) the references of a kernel
    that swaps the two values, or ignores eps, lie many bounds away from the true ones"""
    for low in (False, True):
        for E in (DC.bounded_self(3, 9, False, op16, low), DC.bounded_self(3, 9, True, op16, low), DC.bounded_tail(3, 9, op16, low),
                  DC.bounded_mlp(3, 9, True, op16, low)):
            got = DC.restated_outputs(E, op16)
            checks = DC.bounded_checks(E, got, op16)
            for what, g, ref, b in checks:
                frac = float(((g.double() - ref).abs() / b).max())
                print(f"{op16} lowvar {low} {E['kind']} {what}: {frac:.4f} of the bound")
                assert frac <= 1.0
            if not low or E["kind"] == "self":
                continue
            away = lambda other: {w: float(((r2 - r).abs() / (b + b2)).max()) for (w, _, r, b), (_, _, r2, b2) in zip(checks, other)}
            no_eps = away(DC.bounded_checks(E, got, op16, no_eps=True))
            print("reference without eps, in sums of the two bounds:", no_eps)
            assert no_eps["final norm rows" if E["kind"] == "tail" else "norm2 rows"] > 100
            if E["kind"] == "mlp":
                swapped = away(DC.bounded_checks(E, got, op16, swap=True))
                print("reference with eps2 and eps3 swapped, in sums of the two bounds:", swapped)
                assert swapped["norm2 rows"] > 100 and swapped["norm3 rows"] > 100
                for d in (DC.D[21], DC.D[22]):                # and the restated defects fail the bounded pass
                    bad = DC.restated_outputs(E, op16, d)
                    assert any(not bool(((g.double() - ref).abs() <= b).all()) for _, g, ref, b in DC.bounded_checks(E, bad, op16)), d
