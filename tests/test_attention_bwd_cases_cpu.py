"""The attention-backward variant matrix (tests/test_attention_bwd_variants_gpu.py) must hold for a correct kernel and fail for a wrong one.
For every case of tests/attention_bwd_cases.py, with B * H cut to at most 2, in float64 on the CPU:
  1. the dispatch restatement gives the kernel count, key split and workgroup sizes written next to each shape, and the cases' expected
     kernels add up to the 77 instantiations of csrc/attention_bwd.hip;
  2. an emulation that rounds where the kernels round (fp16 and bf16) stays within attention_bwd_error_bound() of the float64 reference on
     every element of every pass, and still does when dO is left unrounded (that is no defect: a bound that caught it would be a fit);
  3. the closed forms of the selection and tie passes equal the float64 reference, and the fp16 emulation returns them bit for bit (the
     bf16 one within int_slack());
  4. every simulated defect that applies to a case breaks one of its passes: an integer pass by half a quantum of its expected values or
     more, or the bounded pass by at least 4 times its (bf16, the wider) bound on some element.  attention_bwd_cases.applies() says
     where a defect cannot apply, and why.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_bwd_cases as AB  # noqa: E402
from helpers import kernel_key  # noqa: E402

IDS = [AB.case_id(c) for c in AB.CASES]
HALF_QUANTUM = 1.0 / 32            # the integer passes' expected values are multiples of 1 / 16 (scale >= 2^-4 times integers) or 1 / 2


def test_dispatch_restatement_and_kernel_list():
    assert len(AB.ALL_KERNELS) == 77 and len(set(AB.ALL_KERNELS)) == 77
    assert len(set(IDS)) == len(IDS)
    for c in AB.CASES:
        lit = c["lit"]
        got = (AB.dq_key_splits(c["B"], c["H"], c["Lq"], c["Lk"]), AB.role_nw(AB.ROLE_DQ, c["B"], c["H"], c["Lq"], c["Lk"]),
               AB.role_nw(AB.ROLE_DK, c["B"], c["H"], c["Lq"], c["Lk"]))
        assert got == lit, (AB.case_id(c), got, lit)
        assert AB.role_nw(AB.ROLE_DV, c["B"], c["H"], c["Lq"], c["Lk"]) == lit[2]
        assert len(AB.expected_kernels(c, False)) == 4 + (lit[0] > 1)
    reached = {k for c in AB.CASES for no_dma in (False, True) if c["D"] in (128, 256) or not no_dma for k in AB.expected_kernels(c, no_dma)}
    assert reached == set(AB.ALL_KERNELS), sorted(set(AB.ALL_KERNELS) - reached)
    # the edges the table is there for
    assert AB.split_bounds(513, 2, 32) == [0, 288, 513] and AB.split_bounds(2050, 8, 32)[-2:] == [2016, 2050]
    assert AB.workspace_bytes(1, 2, 77, 64) == ((154 * 132 + 255) & ~255) + 8 * 154 * 64 * 4
    # kernels in an unnamed namespace, as the profiler may spell them
    assert kernel_key("void (anonymous namespace)::attn_bwd_kernel<64, 2, 0, false>((anonymous namespace)::AttnBwdParams)") == "attn_bwd_kernel<64,2,0,false>"
    assert kernel_key("_ZN12_GLOBAL__N_115attn_bwd_kernelILi64ELi2ELi0ELb0EEEvNS_13AttnBwdParamsE") == "attn_bwd_kernel<64,2,0,false>"
    assert kernel_key("_ZN12_GLOBAL__N_122attn_bwd_reduce_kernelEPKfPflllliiil") == "attn_bwd_reduce_kernel"


def ratio(err, bound):
    return float((err / bound.clamp_min(1e-300)).max())


@pytest.mark.parametrize("case", AB.CASES, ids=IDS)
def test_emulation_stays_within_the_bound(case):
    c = AB.cut(case)
    for kind in c["passes"]:
        X = AB.build(c, kind)
        ref = AB.reference(X)
        for fp16 in (True, False):
            bound = AB.attention_bwd_error_bound(X, fp16)
            for round_do in (True, False):
                em = AB.emulate(X, fp16, round_do)
                for n in ("dq", "dk", "dv"):
                    err = (em[n] - ref[n]).abs()
                    assert bool((err <= bound[n]).all()), (kind, fp16, round_do, n, ratio(err, bound[n]))
                    if round_do:
                        print(f"RATIO {kind} {'fp16' if fp16 else 'bf16'} {n} {ratio(err, bound[n]):.3f}")
            if kind != "rand":
                # the closed forms are what the kernels' own arithmetic returns
                em, slack = AB.emulate(X, fp16), AB.int_slack(X, fp16)
                for n in ("dv",) if kind == "sel" else ("dq", "dk", "dv"):
                    exp = getattr(X, "exp_" + n)
                    assert float((ref[n] - exp).abs().max()) < HALF_QUANTUM / 2, (kind, n)
                    if fp16:
                        assert torch.equal(em[n], exp), (kind, n, float((em[n] - exp).abs().max()))
                        assert torch.equal(exp.float().double(), exp)
                    else:
                        assert bool(((em[n] - exp).abs() <= slack[n]).all()) and float(slack[n].max()) < HALF_QUANTUM / 2, (kind, n, float(slack[n].max()))


@pytest.mark.parametrize("case", AB.CASES, ids=IDS)
def test_every_defect_breaks_a_pass(case):
    c = AB.cut(case)
    todo = {d for d in AB.DEFECTS if AB.applies(c, d) is None}
    for d in AB.DEFECTS:
        assert AB.applies(c, d) is None or isinstance(AB.applies(c, d), str)
    for kind in c["passes"]:
        X = AB.build(c, kind)
        ref, bound = AB.reference(X), AB.attention_bwd_error_bound(X, False)
        for d in sorted(todo):
            out = AB.reference(X, d)
            for n in ("dq", "dk", "dv"):
                err = (out[n] - ref[n]).abs()
                hit = not bool((err < 4 * bound[n]).all())                       # a NaN counts
                if kind != "rand" and not (kind == "sel" and n != "dv"):
                    hit |= not bool(((out[n] - getattr(X, "exp_" + n)).abs() < HALF_QUANTUM).all())
                if hit:
                    todo.discard(d)
                    break
    assert not todo, f"no pass of this case sees: {sorted(todo)}"


@pytest.mark.parametrize("case", [c for c in AB.CASES if not c["p"] and c["D"] in (64, 256)], ids=lambda c: AB.case_id(c))
def test_builders_place_what_the_passes_lean_on(case):
    c = AB.cut(case)
    Lq, Lk = c["Lq"], c["Lk"]
    X = AB.build(c, "sel")
    hits = torch.zeros(Lk).scatter_add_(0, X.t[0, 0], torch.ones(Lq))
    assert bool((hits == 0).any()) and bool((hits >= 2).any()), "some keys unselected, some shared"
    for key in AB.edge_keys(Lk, c["ksplit"])[:Lq // 2]:
        assert hits[key] >= 1, f"edge key {key} has no query"
    T = AB.build(c, "tie")
    assert len(T.pairs) >= 2 and (Lk <= 32 or any(a // 32 != b // 32 for a, b in T.pairs))
    if Lk % 32 and Lk > 32:
        assert any(b == Lk - 1 and a < Lk // 32 * 32 for a, b in T.pairs), "no pair spans the last full tile and the tail"
    nz = (T.exp_dq != 0).any(2).any(0).any(0)                                     # channels of dQ some query fills
    assert bool(nz.all()) if c["B"] * c["H"] > 1 else int(nz.sum()) == c["D"] - max(1, (Lk - 1).bit_length())
    assert bool((T.exp_dk != 0).any()) and bool((T.exp_dv != T.exp_dv.round()).any()), "halves in dV"
    R = AB.build(c, "rand")
    sc = (R.q @ R.k.transpose(2, 3)) * R.scale
    for row, key in R.dominant.items():
        if row in AB.COLD_ROWS and c["cold"]:
            continue
        top2 = sc[0, 0, row].topk(2)
        assert int(top2.indices[0]) == key and float(top2.values[0] - top2.values[1]) > 4.0, (row, key, top2)
    assert set(AB.edge_keys(Lk, c["ksplit"])) <= set(R.dominant.values()) and set(AB.edge_queries(Lq)) <= set(R.dominant)
    if c["cold"]:
        s = (R.q @ R.k.transpose(2, 3)) * R.scale
        assert float(s[0, 0, list(AB.COLD_ROWS)].max()) < -120 and float(R.lse[0, 0, list(AB.COLD_ROWS)].max()) <= -128
