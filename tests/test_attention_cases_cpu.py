"""The attention kernel-variant matrix (tests/test_attention_variants_gpu.py) must be able to fail: for every case of its tables, in float64
on the CPU,
  1. the selection and tie references equal their closed forms (V[t], the mean of V over the keys that carry the target's K row) to 1e-6,
     the target's score stays GAP bits above every other key's also when Q is pre-multiplied by c and rounded to 16 bits (as
     attn_g96x2_kernel does), and the passes' own bound is below half the smallest change a defect can cause (0.5 / 0.25);
  2. every simulated defect of attention_cases.defects() that applies to the case moves some element of the selection or the tie pass
     beyond that bound (the bf16 one, the wider).  No case is exempt: one that cannot see a defect needs other targets or pairs.
Cases whose [Lq, Lk] scores would take more than about a second here keep their first 160 and last 32 query rows (the targets that matter
sit on the first rows)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_cases as AC  # noqa: E402


def trimmed(c, P):
    if c["Lq"] * c["keys"] <= 4_000_000 or c["Lq"] <= 192:
        return P
    rows = torch.cat((torch.arange(160), torch.arange(c["Lq"] - 32, c["Lq"])))
    P.q, P.expected, P.A, P.t, P.q_valid = P.q[:, :, rows], P.expected[:, :, rows], P.A[:, :, rows], P.t[:, :, rows], P.q_valid[:, rows]
    return P


def test_tables_reach_every_kernel_and_switch():
    want = [AC.FWD(D, NW) for D in (64, 96, 128, 256) for NW in (1, 2, 4)] + [AC.FWD(D, NW, True) for D, NW in
            ((96, 1), (96, 2), (96, 4), (64, 1), (64, 2), (128, 1), (128, 4))] + [AC.GLDS128, AC.GLDS256, AC.GLDS96, AC.G96, AC.KV64, AC.KVX2,
            AC.WIN, AC.TINY1, AC.TINY2, AC.FEWQ16] + [f(D) for f in (AC.FEWKEYS, AC.FEWQ, AC.SMALL) for D in (16, 32)] + [AC.MERGE(D) for D in
            (64, 96, 128, 256)]
    have = {e for c in AC.ALL_CASES for e in c["expect"]}
    assert not [w for w in want if w not in have]
    envs = {k for c in AC.ALL_CASES for k in c["env"]}
    assert envs == {"MSAM2_ATTN_V1", "MSAM2_WIN_V1", "MSAM2_NO_TINYWIN", "MSAM2_TINYWIN_64", "MSAM2_NO_FEWQ16"}
    ids = [AC.case_id(c) for c in AC.ALL_CASES]
    assert len(set(ids)) == len(ids)
    effs = {c["eff"] for c in AC.CASES}
    assert {2, 3, 7, 8, 9, 64} <= effs and any(c["eff"] < c["splits"] for c in AC.CASES)


@pytest.mark.parametrize("case", AC.ALL_CASES, ids=[AC.case_id(c) for c in AC.ALL_CASES])
def test_integer_passes_see_every_defect(case):
    c = case
    unseen = None
    for kind in ("sel", "tie"):
        P = trimmed(c, AC.build(c, kind))
        valid = P.q_valid[:, None, :, None]
        ref, _, _, _ = AC.reference(P.q, P.k, P.v, P.c)
        assert ((ref - P.expected).abs() * valid).max().item() < 1e-6, f"{kind}: the reference is not the closed form"
        # the margin survives Q pre-multiplied by c and rounded to 16 bits
        for dt in (torch.float16, torch.bfloat16):
            s = ((P.q * P.c).to(dt).double() @ P.k.transpose(2, 3))
            top = s.max(-1, keepdim=True).values
            on = torch.gather(s, 3, P.t[..., None])
            assert ((on == top) | ~valid).all(), f"{kind}: a target is not the row maximum after rounding Q to {dt}"
            others = torch.where(s < top, s, torch.full_like(s, -1e30)).max(-1, keepdim=True).values
            assert (((top - others) >= AC.GAP) | ~valid).all(), f"{kind}: margin below {AC.GAP} bits with Q rounded to {dt}"
        bound = AC.integer_bound(P.expected, P.A, c["keys"], c["eff"] > 1, False, P.vmax)
        assert bound.max().item() < (0.5 if kind == "sel" else 0.25) and AC.integer_bound(P.expected, P.A, c["keys"], c["eff"] > 1, True,
                                                                                          P.vmax).max().item() < 0.05
        outs = AC.defects(c, P)
        if unseen is None:
            unseen = set(outs)
        for name, out in outs.items():
            err = (out - P.expected).abs()
            if (~(err <= bound) & valid).any():
                unseen.discard(name)
    assert not unseen, f"no integer pass of this case sees: {sorted(unseen)}"
