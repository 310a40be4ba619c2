"""The 2-D memory bank on the device (csrc/bank.hip, medical_sam2_amd/memory_bank.py) against the float64 restatement of
tests/bank_restate.py.  Feature maps are 16 x 16; the seeded fixtures are the ones tests/test_memory_bank_cpu.py proves valid (every
decision has a margin >= 1e-3, fp32 rounding of a cosine is 1e-6), so indices, flags, order and stored tensors are compared exactly."""
import ctypes
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bank_restate as R  # noqa: E402

from medical_sam2_amd import memory_bank as MB  # noqa: E402
from medical_sam2_amd import ops  # noqa: E402

DEV = "cuda"
F64 = torch.float64
SENT = 0x7FC0BEEF       # a NaN bit pattern


class Flat:
    """a contiguous fp32 output of n elements inside a sentinel-filled buffer"""

    def __init__(self, n, pad=8):
        self.buf = torch.empty(n + 2 * pad, dtype=torch.float32, device=DEV)
        self.buf.view(torch.int32).fill_(SENT)
        self.view = self.buf[pad:pad + n]
        self.n, self.pad = n, pad

    def sentinels_intact(self):
        b = self.buf.view(torch.int32)
        return bool((b[:self.pad] == SENT).all()) and bool((b[self.pad + self.n:] == SENT).all())

    def bits(self):
        return self.view.view(torch.int32).clone()


def nan_operand(vals, layout):
    """vals [rows, n_ch, n_px] as a view of that shape into a NaN-filled buffer.  contig: pixels contiguous, row pitch padded; token: channels
    contiguous (the nchw_view of a token-major map), pixel pitch padded by 4 (16-byte aligned) or, token_odd, by 3 (no vector loads)."""
    rows, n_ch, n_px = vals.shape
    if layout == "contig":
        buf = torch.full((rows + 1, n_ch, n_px + 4), float("nan"), device=DEV)
        view = buf[:rows, :, :n_px]
    else:
        buf = torch.full((rows + 1, n_px, n_ch + (4 if layout == "token" else 3)), float("nan"), device=DEV)
        view = buf[:rows, :, :n_ch].permute(0, 2, 1)
    view.copy_(vals)
    return view


KSHAPES = {1: (1, 1), 63: (7, 9), 4097: (17, 241), 16384: (64, 256), 65536: (256, 256)}


@pytest.mark.parametrize("layout", ["contig", "token", "token_odd"])
@pytest.mark.parametrize("K", sorted(KSHAPES))
def test_bank_dots(K, layout):
    """Exact on small integers, within gamma_n sum|x_i y_i| on random data (n: the chain length stated at bank_dots_kernel, the larger of
    the scalar and the vector path's), NaN padding never read, sentinels around the outputs untouched, two launches bit-identical."""
    n_ch, n_px = KSHAPES[K]
    n = max(ops.bank_dots_chain(K, 1), ops.bank_dots_chain(K, 4) if K % 4 == 0 else 0)
    u = 2.0 ** -24
    gamma = n * u / (1 - n * u)
    gen = torch.Generator(device=DEV).manual_seed(K)
    for R_ in (1, 4, 5):
        for Cn in (1, 16, 19):
            rows_a = 16 if Cn == 19 else Cn                                 # 19 rows: the bank's 16 and 3 candidates from a second operand
            for integer in (True, False):
                def draw(rows):
                    if integer:
                        return torch.randint(-3, 4, (rows, n_ch, n_px), generator=gen, device=DEV).float()
                    return torch.randn(rows, n_ch, n_px, generator=gen, device=DEV)
                xv, yav = draw(R_), draw(rows_a)
                ybv = draw(Cn - rows_a) if Cn > rows_a else None
                x, ya = nan_operand(xv, layout), nan_operand(yav, layout)
                yb = nan_operand(ybv, layout) if ybv is not None else None
                outs = []
                for _ in range(2):
                    d, xx, yy = Flat(R_ * Cn), Flat(R_), Flat(Cn)
                    ops.bank_dots(x, ya, yb, dots=d.view, xx=xx.view, yy=yy.view)
                    assert d.sentinels_intact() and xx.sentinels_intact() and yy.sentinels_intact(), (R_, Cn, integer)
                    outs.append((d, xx, yy))
                for a, b in zip(*outs):
                    assert torch.equal(a.bits(), b.bits()), ("two launches differ", R_, Cn, integer)
                X = xv.reshape(R_, -1).to(F64)
                Y = torch.cat([yav] + ([ybv] if ybv is not None else [])).reshape(Cn, -1).to(F64)
                d, xx, yy = outs[0]
                for got, ref, bound in ((d.view.view(R_, Cn), X @ Y.t(), X.abs() @ Y.abs().t()), (xx.view, (X * X).sum(1), (X * X).sum(1)),
                                        (yy.view, (Y * Y).sum(1), (Y * Y).sum(1))):
                    err = (got.to(F64) - ref).abs()
                    assert not torch.isnan(got).any(), ("padding was read", R_, Cn, integer)
                    if integer:
                        assert float(err.max()) == 0.0, (R_, Cn, float(err.max()))
                    else:
                        assert bool((err <= gamma * bound).all()), (R_, Cn, float((err / bound).max()), gamma)


# ---- bank_decide on integer tables ----------------------------------------------------------------------------------------------------------
def _pool():
    """vectors whose norms are powers of two (axis vectors and +-1 patterns, scaled by 1, 2, 4): every cosine is exact in fp32 and in float64,
    so exact ties are ties on both sides"""
    out = []
    for a in (1., 2., 4.):
        for k in range(4):
            for s in (1., -1.):
                v = [0.] * 4
                v[k] = s * a
                out.append(v)
        for m in range(16):
            out.append([a * (1. if (m >> k) & 1 else -1.) for k in range(4)])
    return torch.tensor(out, dtype=F64)


def decide_case(seed):
    """(G full Gram [N + B, N + B], iou_bank [N], iou_pred [B, M], N, B) of vectors drawn with repetition from _pool()"""
    gen = torch.Generator().manual_seed(seed)
    N = [2, 3, 5, 16, 19][seed % 5]
    B = [1, 2, 4, 8][(seed // 5) % 4]
    pool = _pool()
    V = pool[torch.randint(0, pool.shape[0] if seed % 2 else 12, (N + B,), generator=gen)]
    iou_bank = torch.randint(2, 8, (N,), generator=gen).float() / 8
    iou_pred = torch.randint(1, 8, (B, 3), generator=gen).float() / 8
    return V @ V.t(), iou_bank, iou_pred, N, B


DECIDE_SEEDS = list(range(40))


def run_decide_case(G, iou_bank, iou_pred, N, B, perm):
    """the kernel on tables laid out by the physical permutation perm (logical n sits in slot perm[n]); returns the device tables"""
    gram = torch.zeros(32, 32)
    iou = torch.zeros(32)
    order = torch.arange(32, dtype=torch.int32)
    order[:N] = perm.to(torch.int32)
    inv = torch.empty(N, dtype=torch.long)
    inv[perm] = torch.arange(N)                                              # slot -> logical
    gram[:N, :N] = G[:N, :N][inv][:, inv].float()
    iou[:N] = iou_bank[inv]
    D = torch.cat([G[N:, :N][:, inv], G[N:, N:]], dim=1).float().contiguous()
    gram, iou, order, D = gram.to(DEV), iou.to(DEV), order.to(DEV), D.to(DEV)
    accept, slot_cand = ops.bank_decide(gram, iou, order, N, 32, D, iou_pred.to(DEV), fill=False)
    return gram.cpu(), iou.cpu(), order.cpu().long(), accept.cpu().tolist(), slot_cand.cpu().tolist()


def test_bank_decide_integer_tables():
    """Ties to the first index, a candidate evicted by a later one of its step, a candidate compared against one just accepted: the logical
    tables after the launch equal the restatement's exactly."""
    evicted_same_step = compared_with_new = ties = 0
    for seed in DECIDE_SEEDS:
        G, iou_bank, iou_pred, N, B = decide_case(seed)
        ids, ious = list(range(N)), iou_bank.tolist()
        m = R.Margin()
        iou = R.step_iou(iou_pred)
        flags = R.replace_loop(G, ids, ious, N, B, iou, m)
        ties += m.value == 0.0
        evicted_same_step += any(f and (N + b) not in ids for b, f in enumerate(flags))
        compared_with_new += sum(flags[:-1]) > 0
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(1000 + seed))
        gram, iou_d, order, accept, slot_cand = run_decide_case(G, iou_bank, iou_pred, N, B, perm)
        assert accept == [int(f) for f in flags], seed
        o = order[:N]
        assert sorted(o.tolist()) == list(range(N)), seed                       # live slots stay 0 .. N-1
        assert torch.equal(gram[o][:, o].to(F64), G[ids][:, ids]), seed
        assert iou_d[o].tolist() == [float(torch.tensor(v, dtype=torch.float32)) for v in ious], seed
        want = [-1] * 32
        for n, a in enumerate(ids):
            if a >= N:
                want[int(o[n])] = a - N
        assert slot_cand == want, seed
    assert ties >= 5 and evicted_same_step >= 1 and compared_with_new >= 5, (ties, evicted_same_step, compared_with_new)


# ---- sample ---------------------------------------------------------------------------------------------------------------------------------
def _dev_entries(entries):
    return [[e[0].to(DEV), e[1].to(DEV), e[2], e[3].to(DEV)] for e in entries]


@pytest.mark.parametrize("N,B", sorted(R.SAMPLE_SEEDS))
def test_sample(N, B):
    ref, curr, u, picks = R.sample_fixture(N, B)
    bank = MB.MemoryBank2D(bank_size=min(N, 16), max_batch=4, mem_dim=R.MEM_DIM, hidden_dim=R.HIDDEN, feat_hw=(R.HW_SIDE, R.HW_SIDE), device=DEV)
    bank.load_entries(_dev_entries(ref.entries))
    assert len(bank) == N
    memory, memory_pos, idx = bank.sample(curr.to(DEV), u=u.to(DEV))
    want_mem, want_pos, want_idx = ref.sample(curr, u)
    assert torch.equal(want_idx, picks)
    assert torch.equal(idx.cpu().long(), want_idx)
    assert torch.equal(memory.cpu(), want_mem) and torch.equal(memory_pos.cpu(), want_pos)


def test_sample_empty_bank_and_default_uniforms():
    bank = MB.MemoryBank2D(bank_size=4, max_batch=2, mem_dim=R.MEM_DIM, hidden_dim=R.HIDDEN, feat_hw=(R.HW_SIDE, R.HW_SIDE), device=DEV)
    curr = torch.randn(R.HW_SIDE ** 2, 2, R.HIDDEN, device=DEV)
    assert bank.sample(curr) is None and len(bank) == 0
    ref, _, _, _ = R.sample_fixture(4, 1)
    bank.load_entries(_dev_entries(ref.entries))
    g = torch.Generator(device=DEV).manual_seed(3)
    a = bank.sample(curr, generator=g)[2].clone()
    g.manual_seed(3)
    b = bank.sample(curr, generator=g)[2].clone()
    assert torch.equal(a, b) and int(a.min()) >= 0 and int(a.max()) < 4


# ---- update sequences -----------------------------------------------------------------------------------------------------------------------
def _as_model_gives(f, p, iou, e):
    """the step's tensors in the layouts the model produces: features as the NCHW view of a token-major map, the embedding as the
    [B, C, H, W] view of seq-first [HW, B, C] features; the position encoding stays contiguous NCHW"""
    B, Ce, H, W = e.shape
    f_d = f.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    e_d = e.to(DEV).flatten(2).permute(2, 0, 1).contiguous().permute(1, 2, 0).view(B, Ce, H, W)
    return f_d, p.to(DEV), iou.to(DEV), e_d


def _assert_same_bank(bank, ref, what):
    got = bank.entries()
    assert len(got) == len(ref.entries) == len(bank), what
    for n, (g, w) in enumerate(zip(got, ref.entries)):
        for k in (0, 1, 3):
            assert torch.equal(g[k].cpu(), w[k]), (what, "entry", n, "field", k)
        assert float(g[2]) == float(w[2]), (what, "entry", n, "iou")


@pytest.mark.parametrize("bank_size", sorted(R.UPDATE_SEEDS))
def test_update_sequence(bank_size):
    steps = R.update_fixture(bank_size)
    ref = R.BankRestate(bank_size)
    bank = MB.MemoryBank2D(bank_size=bank_size, max_batch=R.UPDATE_B, mem_dim=R.MEM_DIM, hidden_dim=R.HIDDEN, feat_hw=(R.HW_SIDE, R.HW_SIDE),
                           device=DEV)
    for s, st in enumerate(steps):
        flags = ref.update(*st)
        bank.update(*_as_model_gives(*st))
        assert bank.accept.cpu().tolist() == [int(f) for f in flags], (s, flags)
        _assert_same_bank(bank, ref, f"step {s}")
        t = bank.tables()
        assert sorted(t["order"].tolist()) == list(range(len(bank))), s
        V = torch.stack([e[0].reshape(-1) for e in ref.entries]).to(F64)
        G = V @ V.t()
        assert bool(((t["gram"].to(F64) - G).abs() <= 1e-5 * G.diagonal().max()).all()), s      # the incremental table is the Gram matrix
    assert ref.margin.value >= 1e-3


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
E2E_SEED = 0            # image / click seeds 100 * E2E_SEED + ...; the seed in use keeps the margin below above 1e-5


@pytest.fixture
def no_grad():
    """inference mode for one test only: the global switch would leak into the files collected after this one"""
    with torch.no_grad():
        yield


def test_step_2d_decisions_match_restatement_on_device_tensors(no_grad):
    """8 steps of hiera_t at 256^2 with the bank live.  The restatement is evaluated on the tensors the device handed to the bank in that
    step, so the model's numerics cannot move a decision; the margin of those decisions is asserted."""
    import medical_sam2_amd.build_sam as bs
    import medical_sam2_amd.synthetic as syn
    import medical_sam2_amd.weights as wts
    m = bs.build_sam2("sam2_hiera_t", device="cpu", hydra_overrides_extra=["++model.image_size=256"])
    m.load_state_dict(wts.init_weights("hiera_t", 0), strict=True)
    m = m.to(DEV).eval()
    B = 4
    bank = MB.MemoryBank2D(bank_size=16, max_batch=B, mem_dim=m.mem_dim, hidden_dim=m.hidden_dim, feat_hw=(16, 16), device=DEV)
    ref = R.BankRestate(16)
    seen = {}
    sample0, update0 = bank.sample, bank.update

    def sample(curr, u=None, generator=None):
        seen["curr"] = curr.detach().float().cpu().clone()
        return sample0(curr, u=u, generator=generator)

    def update(f, p, iou, e):
        p = p[0] if isinstance(p, (list, tuple)) else p
        seen["upd"] = tuple(t.detach().float().cpu().clone() for t in (f, p, iou, e))
        return update0(f, p, iou, e)
    bank.sample, bank.update = sample, update
    gen = torch.Generator().manual_seed(E2E_SEED)
    replaced = 0
    for s in range(8):
        imgs, pts, labels = syn.image_batch([100 * E2E_SEED + 4 * s + i for i in range(B)], 256)
        u = torch.rand(B, B, generator=gen)
        _, _, _, idx = MB.step_2d(m, bank, imgs.to(DEV), pts.to(DEV), labels.to(DEV), u=u.to(DEV))
        want = ref.sample(seen["curr"], u)
        if want is None:
            assert idx is None and s == 0
        else:
            assert torch.equal(idx.cpu().long(), want[2]), s
        flags = ref.update(*seen["upd"])
        assert bank.accept.cpu().tolist() == [int(f) for f in flags], (s, flags)
        replaced += sum(flags) if s >= 4 else 0
        _assert_same_bank(bank, ref, f"step {s}")
    print(f"e2e bank: seed {E2E_SEED}, margin {ref.margin.value:.3e}, {replaced} of 16 steady-state candidates accepted")
    assert ref.margin.value >= 1e-5, f"seed {E2E_SEED}: margin {ref.margin.value:.3e}, pick another seed"


# ---- capture --------------------------------------------------------------------------------------------------------------------------------
def test_three_steps_in_one_graph_match_eager():
    steps = R.update_fixture(16)
    gen = torch.Generator().manual_seed(77)
    HW = R.HW_SIDE ** 2
    currs = [torch.randn(HW, 4, R.HIDDEN, generator=gen) for _ in range(12)]
    us = [torch.rand(4, 4, generator=gen) for _ in range(12)]
    mk = lambda: MB.MemoryBank2D(bank_size=16, max_batch=4, mem_dim=R.MEM_DIM, hidden_dim=R.HIDDEN, feat_hw=(R.HW_SIDE, R.HW_SIDE), device=DEV)
    a, b = mk(), mk()
    for s in range(5):                                   # fill (4 steps) and one replacement step, eagerly: buffers exist, the bank is full
        a.sample(currs[s].to(DEV), u=us[s].to(DEV))
        a.update(*_as_model_gives(*steps[s]))
    start = a.state_dict()
    b.load_state_dict(start)

    def run(bank, inputs, idx_out):
        for k, (c, u, st) in enumerate(inputs):
            idx_out[k].copy_(bank.sample(c, u=u)[2])
            bank.update(*st)
    static = [(currs[s].to(DEV), us[s].to(DEV), _as_model_gives(*steps[s])) for s in (5, 6, 7)]
    idx_a = torch.zeros(3, 4, 4, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(a, static, idx_a)
    # fresh inputs into the captured tensors, the bank back to the start, one replay
    fresh = [(currs[s].to(DEV), us[s].to(DEV), _as_model_gives(*steps[s])) for s in (8, 9, 10)]
    for (c, u, st), (c2, u2, st2) in zip(static, fresh):
        c.copy_(c2)
        u.copy_(u2)
        for t, t2 in zip(st, st2):
            t.copy_(t2)
    a.load_state_dict(start)
    idx_a.zero_()
    graph.replay()
    torch.cuda.synchronize()
    idx_b = torch.zeros_like(idx_a)
    b.sample(fresh[0][0], u=fresh[0][1])                 # allocates b's result buffers; the draw does not change the bank
    run(b, fresh, idx_b)
    assert torch.equal(idx_a, idx_b)
    sa, sb = a.state_dict(), b.state_dict()
    for k in MB.MemoryBank2D._STATE:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(a.accept, b.accept) and torch.equal(a.slot_cand, b.slot_cand)
    assert not torch.equal(sa["order"], start["order"]) or not torch.equal(sa["feats"], start["feats"])   # the replay did replace entries


# ---- argument errors ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_codes():
    from medical_sam2_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    ptr = (ctypes.addressof(buf) + 15) & ~15             # a valid aligned host address; the checks never dereference it
    st = (ctypes.c_int64 * 3)(16, 4, 1)
    neg = (ctypes.c_int64 * 3)(16, -4, 1)
    cases = {
        "bank_dots: R": lambda: L.msam2_bank_dots(ptr, st, 9, ptr, st, 4, None, None, 0, 4, 4, ptr, None, None, ptr, 1 << 20, None),
        "bank_dots: rows": lambda: L.msam2_bank_dots(ptr, st, 4, ptr, st, 30, ptr, st, 3, 4, 4, ptr, None, None, ptr, 1 << 20, None),
        "bank_dots: strides": lambda: L.msam2_bank_dots(ptr, neg, 4, ptr, st, 4, None, None, 0, 4, 4, ptr, None, None, ptr, 1 << 20, None),
        "bank_dots: workspace": lambda: L.msam2_bank_dots(ptr, st, 4, ptr, st, 4, None, None, 0, 4, 4, ptr, None, None, ptr, 16, None),
        "bank_dots: null": lambda: L.msam2_bank_dots(None, st, 4, ptr, st, 4, None, None, 0, 4, 4, ptr, None, None, ptr, 1 << 20, None),
        "bank_sample: N": lambda: L.msam2_bank_sample(ptr, 32, ptr, ptr, ptr, 0, 19, ptr, 4, 4, ptr, None, None),
        "bank_sample: B": lambda: L.msam2_bank_sample(ptr, 32, ptr, ptr, ptr, 4, 19, ptr, 9, 4, ptr, None, None),
        "bank_gather: C": lambda: L.msam2_bank_gather(ptr, ptr, ptr, ptr, 4, 4, 256, 62, 16, 19, ptr, ptr, None),
        "bank_gather: N": lambda: L.msam2_bank_gather(ptr, ptr, ptr, ptr, 4, 4, 256, 64, 20, 19, ptr, ptr, None),
        "bank_decide: capacity": lambda: L.msam2_bank_decide(ptr, ptr, ptr, 30, 32, ptr, ptr, 4, 1, 1, ptr, ptr, None, None),
        "bank_decide: B": lambda: L.msam2_bank_decide(ptr, ptr, ptr, 16, 19, ptr, ptr, 0, 1, 0, ptr, ptr, None, None),
        "bank_commit: capacity": lambda: L.msam2_bank_commit(ptr, 33, ptr, st, ptr, st, 64, ptr, st, 256, 256, 4, ptr, ptr, ptr, None),
        "bank_commit: null": lambda: L.msam2_bank_commit(ptr, 19, ptr, st, None, st, 64, ptr, st, 256, 256, 4, ptr, ptr, ptr, None),
    }
    for what, call in cases.items():
        rc = call()
        msg = L.msam2_last_error().decode()
        assert rc < 0, (what, rc)
        assert what.split(":")[0] in msg, (what, msg)
    assert ops.bank_dots_chain(0, 4) < 0 and ops.bank_dots_chain(63, 4) < 0
    with pytest.raises(RuntimeError, match="bank_decide"):
        ops.bank_decide(torch.zeros(32, 32), torch.zeros(32), torch.arange(32, dtype=torch.int32), 30, 32, torch.zeros(4 * 34), torch.zeros(4, 1), True)
