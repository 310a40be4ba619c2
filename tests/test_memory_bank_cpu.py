"""The float64 restatement of the 2-D memory bank (tests/bank_restate.py) on cases derivable by hand, and the validity condition of the
seeded fixtures that tests/test_memory_bank_gpu.py runs on the device: every decision of a fixture has a margin >= 1e-3, so fp32 rounding
(1e-6 on a cosine) cannot move it and the fixture has one right answer.

Hand cases: K = 4, axis-aligned vectors, so every cosine is 0, +-1 or 1/sqrt(2)."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bank_restate as R  # noqa: E402

E1, E2, E3, E4 = (1., 0., 0., 0.), (0., 1., 0., 0.), (0., 0., 1., 0.), (0., 0., 0., 1.)
E12 = (1., 1., 0., 0.)
RS2 = 1 / math.sqrt(2)


def vecs(*rows):
    """rows of 4 numbers -> feats [n, 4, 1, 1]"""
    return torch.tensor(rows, dtype=torch.float32).reshape(len(rows), 4, 1, 1)


def bank_of(rows, ious, bank_size):
    """a full bank whose entry n has features rows[n] (scaled by n + 1: raw dots are not cosines), position n and embedding n"""
    b = R.BankRestate(bank_size)
    for n, (r, iou) in enumerate(zip(rows, ious)):
        b.entries.append([vecs(r) * (n + 1), torch.full((1, 4, 1, 1), float(n)), torch.tensor(iou), torch.full((8,), float(n))])
    return b


def step(rows, iou):
    n = len(rows)
    return vecs(*rows), torch.full((n, 4, 1, 1), 100.), torch.full((n, 1), iou), torch.full((n, 2, 2, 2), 100.)


def tags(bank):
    """which entry sits where: the stored position encoding's value (100 = a candidate of `step`)"""
    return [int(e[1].flatten()[0]) for e in bank.entries]


def test_reject_by_similarity():
    # mutually orthogonal bank, orthogonal candidate: every cosine is 0, i = 0 (first of the tie), cos(e_i, e_j) = 0: 0 < 0 is false
    b = bank_of([E1, E2, E3], [0.5, 0.5, 0.5], 3)
    assert b.update(*step([E4], 0.9)) == [False]
    assert tags(b) == [0, 1, 2]
    # candidate (1,1,0,0): cosines 1/sqrt2, 1/sqrt2, 0 -> i = 2, whose neighbours are both at 0: 0 < 0 is false again
    assert b.update(*step([E12], 0.9)) == [False]
    assert tags(b) == [0, 1, 2] and b.margin.value == 0.0


def test_reject_by_iou_gate_then_accept_with_pop_shift():
    # e1, (e1+e2), e3; candidate e4: cosines 0, 0, 0 -> i = 0; cos(e1, .) = [-, 1/sqrt2, 0] -> j = 1; 0 < 1/sqrt2 holds
    b = bank_of([E1, E12, E3], [0.9, 0.9, 0.9], 3)
    assert b.update(*step([E4], 0.5)) == [False]                 # 0.5 > 0.9 - 0.1 fails
    assert tags(b) == [0, 1, 2]
    assert b.update(*step([E4], 0.85)) == [True]                 # 0.85 > 0.8: entry 1 is popped, entry 2 shifts down, the candidate is appended
    assert tags(b) == [0, 2, 100]
    assert float(b.entries[2][2]) == pytest.approx(0.85) and float(b.entries[1][2]) == pytest.approx(0.9)
    assert torch.equal(b.entries[2][0], vecs(E4)) and torch.equal(b.entries[2][3], torch.full((8,), 100.))


def test_negative_cosine_and_candidate_compared_with_one_just_accepted():
    # candidate -e1: cosines -1, -1/sqrt2, 0 -> i = 0, j = 1 (1/sqrt2), -1 < 1/sqrt2: accepted -> [e1, e3, -e1]
    # second candidate of the same step, e1+e2: cosines 1/sqrt2, 0, -1/sqrt2 -> i = 2, the entry accepted a moment ago;
    # cos(-e1, e1) = -1, cos(-e1, e3) = 0 -> j = 1; -1/sqrt2 < 0: accepted -> [e1, -e1, e1+e2]
    b = bank_of([E1, E12, E3], [0.5, 0.5, 0.5], 3)
    f, p, iou, emb = step([(-1., 0., 0., 0.), E12], 0.6)
    p[1] = 200.
    assert b.update(f, p, iou, emb) == [True, True]
    assert tags(b) == [0, 100, 200]
    assert [tuple(e[0].flatten().tolist()) for e in b.entries] == [E1, (-1., 0., 0., 0.), E12]


def test_fill_overshoot():
    # bank_size 3, B = 2: 0 -> 2 -> 4 entries (the rule is "append all B while len < bank_size"), replacement from then on
    b = R.BankRestate(3)
    assert b.update(*step([E1, E2], 0.5)) == [True, True] and len(b.entries) == 2
    assert b.update(*step([E3, E12], 0.5)) == [True, True] and len(b.entries) == 4
    assert b.update(*step([E4, E4], 0.5)) == [True, False] and len(b.entries) == 4
    # e4: cosines 0 0 0 0 -> i = 0 (e1), j = 3 (e1+e2 at 1/sqrt2): accepted -> [e1, e2, e3, e4]; the second e4: cosines 0 0 0 1 -> i = 0,
    # cos(e1, .) = 0 everywhere: rejected
    assert [tuple(e[0].flatten().tolist()) for e in b.entries] == [E1, E2, E3, E4]


def test_step_iou_is_mean_of_row_maxima():
    iou = R.step_iou(torch.tensor([[0.25, 0.5], [0.75, 0.125]]))
    assert float(iou) == 0.625 and iou.dtype == torch.float32


def test_draw_by_hand_and_layout():
    # embeddings e1, e2 against the current features e1: cosines 1, 0 -> p = e / (e + 1) = 0.7311, 0.2689
    emb = torch.tensor([E1, E2]) * 3
    p, cdf = R.draw_cdf(emb, torch.tensor([E1]))
    assert float(p[0, 0]) == pytest.approx(math.e / (math.e + 1), abs=1e-12) and float(cdf[0, 1]) == pytest.approx(1.0, abs=1e-12)
    idx, m = R.draw(emb, torch.tensor([E1]), torch.tensor([[0.5, 0.8, 0.0, 0.7310]]))
    assert idx.tolist() == [[0, 1, 0, 0]] and m.value == pytest.approx(math.e / (math.e + 1) - 0.7310, abs=1e-6)
    # layout: memory[(s * HW + p), b, c] = feats of entry idx[b][s] at channel c, pixel p
    ent = [[torch.arange(8.).reshape(1, 4, 1, 2) + 100 * n, -(torch.arange(8.).reshape(1, 4, 1, 2) + 100 * n), None, None] for n in range(3)]
    ix = torch.tensor([[2, 0], [1, 1]])
    mem, pos = R.gather(ent, ix)
    assert mem.shape == (4, 2, 4)
    for s in range(2):
        for px in range(2):
            for b in range(2):
                for c in range(4):
                    assert float(mem[s * 2 + px, b, c]) == 100 * int(ix[b, s]) + c * 2 + px
    assert torch.equal(pos, -mem)


def test_embedding_order_quirk():
    """The stored embedding is image_embed.reshape(-1), (channel, pixel) order; the current features are flattened token-major, (pixel,
    channel) order; the two flat vectors are multiplied as they are."""
    b = R.BankRestate(1)
    img = torch.zeros(1, 2, 1, 2)                                   # C = 2, HW = 2
    img[0, 0, 0, 1] = 1.0                                           # channel 0, pixel 1 -> flat index 1 of (channel, pixel)
    b.update(torch.ones(1, 4, 1, 2), torch.ones(1, 4, 1, 2), torch.ones(1, 1), img)
    assert b.entries[0][3].tolist() == [0., 1., 0., 0.]
    curr = torch.zeros(2, 1, 2)                                     # [HW, B, C]
    curr[0, 0, 1] = 1.0                                             # pixel 0, channel 1 -> flat index 1 of (pixel, channel)
    e = torch.stack([b.entries[0][3], torch.tensor([0., 0., 1., 0.])])
    p, _ = R.draw_cdf(e, curr.permute(1, 0, 2).reshape(1, -1))
    assert float(p[0, 0]) == pytest.approx(math.e / (math.e + 1), abs=1e-12)


@pytest.mark.parametrize("N,B", sorted(R.SAMPLE_SEEDS))
def test_sample_fixture_is_valid(N, B):
    bank, curr, u, picks = R.sample_fixture(N, B)
    _, _, idx = bank.sample(curr, u)
    assert torch.equal(idx, picks)
    assert bank.margin.value >= 1e-3


@pytest.mark.parametrize("bank_size", sorted(R.UPDATE_SEEDS))
def test_update_fixture_is_valid(bank_size):
    bank, flags = R.run_updates(bank_size, R.update_fixture(bank_size))
    assert bank.margin.value >= 1e-3
    steady = [f for fl in flags[-(-bank_size // R.UPDATE_B):] for f in fl]
    assert sum(steady) >= 8 and len(steady) - sum(steady) >= 8       # both outcomes are exercised
    assert len(bank.entries) == -(-bank_size // R.UPDATE_B) * R.UPDATE_B
