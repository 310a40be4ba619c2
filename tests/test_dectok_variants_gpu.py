"""Variant matrix of the decoder token kernels (GPU): dec_self_kernel, dec_mlp_kernel, dec_kv_kernel, dec_tail_kernel
(csrc/decoder_tokens.hip) and the key-split producer attn_fewq16_part_kernel<1|2|4|8> (csrc/attention.hip), through the C entries with
this file's own buffers, in the style of tests/test_rowtile_variants_gpu.py (tests/dectok_cases.py has the builders and the why):
  * every output (queries_out, queries_mid, qp, kv, qp_final, the producer's partials) is a contiguous view between sentinels -- the
    entries take no leading dimension, so helpers.Flat and not a strided Canvas -- and the sentinels must be bit-identical afterwards;
    every input lies between NaN guards (q, k, v of the producer: column blocks of a wider NaN-filled map, as the decoder passes them);
    the fc2 workspace is larger than msam2_decoder_tokens_workspace_bytes, NaN-filled, and its guard and tail must still be NaN;
  * exact pass: 16-bit outputs and the workspace slabs == expected bits, fp32 LayerNorm rows inside the derived fp32 bound;
  * synthetic partials at 1 .. 8 splits (live, empty, dead) through dec_tail and dec_mlp: part of the exact tables;
  * producer: selection + ties (the target's split reports m, l, O to the bit, every other live split a maximum >= 200 below, empty
    splits (-inf, 0, 0)), its partials through dec_tail (and dec_mlp) == the same call on the 16-bit rows V[t]; random operands against
    float64 inside attention_error_bound, then through the consumers inside the bounded pass's bounds;
  * bounded pass: randn operands, every stage against float64 (RATIO lines: the fraction of each bound used, and of the older
    0.02 + 0.01 |ref|), low-variance rows with eps2 = 1e-3, eps3 = 1e-6; BITDIFF lines: how many 16-bit outputs differ from the launches
    the kernels replace (a finding, no assertion); token order.
The 16-bit type is ops.OP16 throughout; the file runs once more in a child process on the bf16 library."""
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dectok_cases as DC  # noqa: E402
from helpers import ROOT, Flat, kernels_launched, nan_guarded  # noqa: E402

DEV = "cuda"
F32 = torch.float32
C, NH, CI, HID = DC.C, DC.NH, DC.CI, DC.HID
REACHED = set()
WORST = {}                     # category -> the largest fraction of its bound used in this process


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


def bits_equal(got, want, what):
    it = {2: torch.int16, 4: torch.int32}[got.dtype.itemsize]
    want = want.to(got.device)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    ne = got.contiguous().view(it) != want.contiguous().view(it)
    if bool(ne.any()):
        i = int(ne.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} elements differ in their bits; first at flat index {i}: got "
                             f"{float(got.flatten()[i])}, expected {float(want.flatten()[i])}")


def inside(got, ref, bound, what, old=False, key=None):
    """|got - ref| <= bound element by element (a NaN fails); prints the fraction of the bound used.  old: the bound is the smaller of
    the derived one and the family's older 0.02 + 0.01 |ref| (the self-attention chain's worst-case bound is the wider of the two), and
    the fraction of the older one is printed beside it"""
    ref, bound = ref.to(got.device), bound.to(got.device)
    d = (got.double() - ref).abs()
    frac = float((d / bound).max())
    line = f"RATIO {what}: {frac:.4f} of the bound (max |err| {float(d.max()):.4g})"
    if old:
        lim = 0.02 + 0.01 * ref.abs()
        line += f"; {float((d / lim).max()):.5f} of 0.02 + 0.01 |ref|"
        bound = torch.minimum(bound.expand_as(lim), lim)
    print(line)
    if key is not None:
        WORST[key] = max(WORST.get(key, 0.0), frac)
        if old:
            WORST[key + " (of 0.02 + 0.01 |ref|)"] = max(WORST.get(key + " (of 0.02 + 0.01 |ref|)", 0.0), float((d / lim).max()))
    bad = ~(d <= bound)
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; first at flat index {i}: got "
                             f"{float(got.flatten()[i])}, reference {float(ref.flatten()[i])}, bound {float(bound.expand_as(d).flatten()[i]):.3e}")


class Call:
    """one call of a case's entry: inputs between NaN guards, outputs between sentinels, the workspace NaN-filled with guard and tail"""
    GUARD = 64

    def __init__(self, ops, E):
        self.E, self.op16 = E, ops.OP16
        B, T = E["B"], E["T"]
        R = B * T
        self.f = lambda t: None if t is None else nan_guarded(t.to(F32).to(DEV))
        self.h = lambda t: None if t is None else nan_guarded(t.to(self.op16).to(DEV))
        self.out = {}
        new = lambda name, n, dt: self.out.setdefault(name, Flat((R, n), dt))
        new("queries_out", C, F32)
        if E["kind"] == "self":
            new("qp", CI, self.op16)
        if E["kind"] == "mlp":
            new("queries_mid", C, F32), new("kv", C, self.op16)
            if E["last"]:
                new("qp_final", CI, self.op16)
            self.ws_n = DC.NSLICE * R * C
            self.ws_buf = torch.full((self.GUARD + self.ws_n + DC.WS_TAIL,), math.nan, dtype=F32, device=DEV)

    def _attn(self):
        E = self.E
        if E["part"] is None:
            return self.h(E["o"]), None, 0
        return None, self.f(E["part"]), E["splits"]

    def run(self, L):
        E, B, T = self.E, self.E["B"], self.E["T"]
        o = self.out
        if E["kind"] == "self":
            a = [self.f(E["x"]), self.f(E["pe"]), self.h(E["wqkv"]), self.f(E["bqkv"]), self.h(E["wo"]), self.f(E["bo"]), self.f(E["ln_w"]),
                 self.f(E["ln_b"]), self.h(E["wcq"]), self.f(E["bcq"])]
            rc = L.msam2_decoder_tokens_self(p(a[0]), p(a[1]), int(E["skip"]), p(a[2]), p(a[3]), p(a[4]), p(a[5]), p(a[6]), p(a[7]), E["eps"], p(a[8]),
                                             p(a[9]), p(o["queries_out"].view), p(o["qp"].view), B, T, C, NH, stream())
        elif E["kind"] == "tail":
            o16, part, S = self._attn()
            a = [self.f(E["x"]), self.h(E["wo"]), self.f(E["bo"]), self.f(E["ln_w"]), self.f(E["ln_b"])]
            rc = L.msam2_decoder_tokens_tail(p(o16), p(part), S, p(a[0]), p(a[1]), p(a[2]), p(a[3]), p(a[4]), E["eps"], p(o["queries_out"].view), B, T,
                                             C, NH, stream())
        else:
            o16, part, S = self._attn()
            a = [self.f(E["x"]), self.h(E["wo"]), self.f(E["bo"]), self.f(E["ln2_w"]), self.f(E["ln2_b"]), self.h(E["w1"]), self.f(E["b1"]),
                 self.h(E["w2"]), self.f(E["b2"]), self.f(E["ln3_w"]), self.f(E["ln3_b"]), self.f(E["pe"]), self.h(E["wkv"]), self.f(E["bkv"]),
                 self.h(E["wfq"]), self.f(E["bfq"])]
            ws = self.ws_buf[self.GUARD:]
            need = L.msam2_decoder_tokens_workspace_bytes(B, T)
            assert need == 4 * self.ws_n
            rc = L.msam2_decoder_tokens_mlp(p(o16), p(part), S, p(a[0]), p(a[1]), p(a[2]), p(a[3]), p(a[4]), E["eps2"], p(a[5]), p(a[6]), p(a[7]),
                                            p(a[8]), p(a[9]), p(a[10]), E["eps3"], p(a[11]), p(a[12]), p(a[13]), p(a[14]), p(a[15]),
                                            p(o["queries_mid"].view), p(o["queries_out"].view), p(o["kv"].view),
                                            p(o["qp_final"].view) if E["last"] else None, p(ws), 4 * (self.ws_n + DC.WS_TAIL), B, T, C, NH, HID, stream())
        assert rc == 0, L.msam2_last_error().decode()
        torch.cuda.synchronize()
        del a
        for name, fl in o.items():
            assert fl.sentinels_intact(), f"{name}: a store outside the output (a row >= T of the last image, or in front of the first)"
        got = {name: fl.view for name, fl in o.items()}
        if E["kind"] == "mlp":
            assert bool(torch.isnan(self.ws_buf[:self.GUARD]).all()) and bool(torch.isnan(self.ws_buf[self.GUARD + self.ws_n:]).all()), \
                "the workspace's guard or tail was written"
            got["ws"] = self.ws_buf[self.GUARD:self.GUARD + self.ws_n].view(DC.NSLICE, B * T, C)
        return got


def run_named(L, call, prefix="dec_"):
    """the call under the profiler: (outputs, kernels whose name starts with prefix).  The callers assert that no OTHER kernel of the
    family ran; the profiler now and then returns no record for a launch whose outputs are there, so that every name was seen is
    asserted once, over the whole file (test_all_eight_kernels_were_reached) -- and a kernel that did not run leaves sentinels."""
    res = {}
    names = kernels_launched(lambda: res.update(call.run(L)), prefix)
    REACHED.update(names)
    return res, names


def check_exact(E, got, op16, cid):
    for name, want in DC.expected(E, op16).items():
        if want[0] == "bits":
            bits_equal(got[name], want[1], f"{cid} exact pass, {name}")
        else:
            inside(got[name], want[1], want[2], f"{cid} exact pass, {name} vs the float64 LayerNorm of the exact row",
                   key=f"exact {E['kind']} {name}")


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,skip", DC.SELF_CASES, ids=lambda v: str(v))
def test_self_exact(ops, L, B, T, skip):
    E = DC.self_exact(B, T, skip)
    got, names = run_named(L, Call(ops, E))
    assert names <= {"dec_self_kernel"}, names
    check_exact(E, got, ops.OP16, f"self B{B} T{T} skip {skip}")


@pytest.mark.parametrize("B,T,splits", DC.TAIL_CASES, ids=lambda v: str(v))
def test_tail_exact(ops, L, B, T, splits):
    E = DC.tail_exact(B, T, splits)
    got, names = run_named(L, Call(ops, E))
    assert names <= {"dec_tail_kernel"}, names
    check_exact(E, got, ops.OP16, f"tail B{B} T{T} splits {splits}")


@pytest.mark.parametrize("B,T,last,splits", DC.MLP_CASES, ids=lambda v: str(v))
def test_mlp_exact(ops, L, B, T, last, splits):
    E = DC.mlp_exact(B, T, last, splits)
    got, names = run_named(L, Call(ops, E))
    assert names <= {"dec_mlp_kernel", "dec_kv_kernel"}, names
    assert ("qp_final" in got) == last
    check_exact(E, got, ops.OP16, f"mlp B{B} T{T} last {last} splits {splits}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the producer
def producer_call(ops, L, P):
    """q, k, v as column blocks of wider NaN-filled maps; the partials between sentinels; returns (partials [B NH S Lq, 18], kernel names)"""
    B, Lq, Lk, S = P["B"], P["Lq"], P["Lk"], P["S"]
    qmap = torch.full((B * Lq + 3, 3 * CI), math.nan, dtype=ops.OP16, device=DEV)
    kvmap = torch.full((B * Lk + 3, 3 * CI), math.nan, dtype=ops.OP16, device=DEV)
    rows = lambda t, n: t.permute(0, 2, 1, 3).reshape(B * n, CI).to(ops.OP16).to(DEV)
    qmap[:B * Lq, CI:2 * CI] = rows(P["q"], Lq)
    kvmap[:B * Lk, :CI], kvmap[:B * Lk, CI:2 * CI] = rows(P["k"], Lk), rows(P["v"], Lk)
    q, k, v = qmap[:B * Lq, CI:2 * CI], kvmap[:B * Lk, :CI], kvmap[:B * Lk, CI:2 * CI]
    out = Flat((B * NH * S * Lq, 18), F32)

    def go():
        rc = L.msam2_attention_fewq_keysplit(p(q), Lq * 3 * CI, 3 * CI, p(k), Lk * 3 * CI, 3 * CI, p(v), Lk * 3 * CI, 3 * CI, p(out.view), B, NH, Lq, Lk,
                                             DC.DX, S, 1.0 / math.sqrt(DC.DX), stream())
        assert rc == 0, L.msam2_last_error().decode()
    names = kernels_launched(go, "attn_fewq16")
    REACHED.update(names)
    assert out.sentinels_intact(), "the producer wrote outside its partials"
    return out.view, names


@pytest.mark.parametrize("Lq,Lk,S", DC.PRODUCER_CASES, ids=lambda v: str(v))
def test_producer(ops, L, Lq, Lk, S):
    cid = f"producer Lq{Lq} Lk{Lk} S{S}"
    want_kernel = {f"attn_fewq16_part_kernel<{DC.part_maxs(Lk, S)}>"}
    # ---- selection and ties
    P = DC.producer_sel(Lq, Lk, S)
    part, names = producer_call(ops, L, P)
    assert names <= want_kernel, (names, want_kernel)
    exp, state = P["exp"].to(F32).to(DEV), P["state"].to(DEV)
    known = ~torch.isnan(exp)
    bits_equal(torch.where(known, part, torch.zeros_like(part)), torch.where(known, exp, torch.zeros_like(exp)),
               f"{cid}: (m, l, O) of the target's split and of empty splits")
    other = part[state == 1]
    assert bool(torch.isfinite(other).all()) and bool((other[:, 0] <= -DC.GAP).all()) and bool((other[:, 1] > 0).all()), \
        f"{cid}: a live split without the target reports a finite maximum >= {DC.GAP} below and a positive sum"
    B = P["B"]
    if Lq <= DC.MAXT:                                       # through the consumers: == the same call on the 16-bit rows V[t]
        Er = DC.tail_exact(B, Lq, 0)
        Er["o"] = P["o"]
        Ep = dict(Er, part=part.double().cpu(), splits=S)
        a, _ = run_named(L, Call(ops, Er))
        b, _ = run_named(L, Call(ops, Ep))
        bits_equal(b["queries_out"], a["queries_out"], f"{cid}: dec_tail from the partials against dec_tail from V[t]")
        if Lq == 7:
            Er = DC.mlp_exact(B, Lq, True, 0)
            Er["o"] = P["o"]
            Ep = dict(Er, part=part.double().cpu(), splits=S)
            a, b = Call(ops, Er).run(L), Call(ops, Ep).run(L)
            for name in a:
                bits_equal(b[name], a[name], f"{cid}: dec_mlp from the partials against dec_mlp from V[t], {name}")
    # ---- random operands against float64
    P = DC.producer_rand(Lq, Lk, S, ops.OP16)
    part, names = producer_call(ops, L, P)
    assert names <= want_kernel, (names, want_kernel)
    pp = part.double().view(B, NH, S, Lq, 18)
    m, l, O = pp[..., 0], pp[..., 1], pp[..., 2:]
    w = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp2(m - m.amax(2, keepdim=True)))
    Lsum = (l * w).sum(2)
    inside((O * w[..., None]).sum(2) / Lsum[..., None], P["ref"], P["bound"], f"{cid}: merged O / l vs float64 attention", key="producer O / l")
    inside(m.amax(2) + torch.log2(Lsum), P["lse"], P["lse_bound"], f"{cid}: m + log2 l vs float64", key="producer m + log2 l")
    empty = torch.tensor([hi <= lo for lo, hi in DC.split_ranges(Lk, S)], device=DEV)
    assert bool(torch.isinf(m[:, :, empty]).all()) and bool((pp[:, :, empty][..., 1:] == 0).all()) and bool(torch.isfinite(pp[:, :, ~empty]).all())
    if Lq <= DC.MAXT:
        E = DC.bounded_tail(B, Lq, ops.OP16, part=part.double().cpu(), splits=S)
        got = Call(ops, E).run(L)
        for what, g, ref, b in DC.bounded_checks(E, {k_: v_.cpu() for k_, v_ in got.items()}, ops.OP16):
            inside(g, ref, b, f"{cid}: dec_tail from random partials, {what}", old=True, key=f"partials tail {what}")
        if Lq == 7:
            E = DC.bounded_mlp(B, Lq, True, ops.OP16, part=part.double().cpu(), splits=S)
            got = Call(ops, E).run(L)
            for what, g, ref, b in DC.bounded_checks(E, {k_: v_.cpu() for k_, v_ in got.items()}, ops.OP16):
                inside(g, ref, b, f"{cid}: dec_mlp from random partials, {what}", old=True, key=f"partials mlp {what}")


# ---------------------------------------------------------------------------------------------------------------------------------
# bounded pass
def bounded_cases(B, T, op16, low):
    return [DC.bounded_self(B, T, False, op16, low), DC.bounded_self(B, T, True, op16, low), DC.bounded_tail(B, T, op16, low),
            DC.bounded_mlp(B, T, False, op16, low), DC.bounded_mlp(B, T, True, op16, low)]


def run_bounded(ops, L, E, what):
    got = Call(ops, E).run(L)
    for name, g, ref, b in DC.bounded_checks(E, {k: v.cpu() for k, v in got.items()}, ops.OP16):
        inside(g.to(DEV), ref, b, f"{what} {E['kind']}{' skip' if E.get('skip') else ''}{' last' if E.get('last') else ''}: {name}", old=True,
               key=f"{what.split(' B')[0]} {E['kind']} {name}")
    return got


@pytest.mark.parametrize("B,T", DC.SHAPES, ids=lambda v: str(v))
def test_bounded(ops, L, B, T):
    for E in bounded_cases(B, T, ops.OP16, False):
        run_bounded(ops, L, E, f"bounded B{B} T{T}")


def test_bounded_low_variance_rows_see_eps(ops, L):
    """pre-norm rows of standard deviation ~0.03 with eps1 = eps2 = 1e-3, eps3 = 1e-6: a dropped or swapped eps is hundreds of bounds
    away (tests/test_dectok_cases_cpu.py asserts that on the references)"""
    for B, T in ((3, 9), (2, 16)):
        for E in bounded_cases(B, T, ops.OP16, True):
            run_bounded(ops, L, E, f"low variance B{B} T{T}")


def test_bits_against_the_launches_replaced(ops, L):
    """DESIGN.md 3.10 claims that every GEMM but fc2 keeps the bits of the launch it replaces.  Counted here on the random cases, not
    asserted: BITDIFF lines (DESIGN.md 3.10.1 quotes them)."""
    from test_decoder_tokens_gpu import old_mlp, old_self
    total = {}
    for B, T in DC.SHAPES:
        R = B * T
        b = DC.bounded(B, T, ops.OP16)
        W = {k: v.to(ops.OP16 if v.dim() == 2 else F32).to(DEV) for k, v in b["W"].items()}
        x, pe, o = b["x"].float().to(DEV), b["pe"].float().to(DEV), b["o"].to(ops.OP16).to(DEV)
        for skip in (False, True):
            got = Call(ops, DC.bounded_self(B, T, skip, ops.OP16)).run(L)
            ry, rqp = old_self(ops, x, pe, skip, W, B, T)
            own = ops.gemm_tokens(got["queries_out"].contiguous(), W["wcq"], W["bcq"], addend=pe, add_cols=CI)
            for name, a, r in (("self: norm1 rows (fp32)", got["queries_out"], ry), ("self: qp", got["qp"], rqp),
                               ("self: qp against gemm_tokens on the kernel's OWN norm1 rows", got["qp"], own)):
                n, d = total.get(name, (0, 0))
                total[name] = (n + a.numel(), d + int((a.view(torch.int32 if a.dtype == F32 else torch.int16)
                                                       != r.reshape(a.shape).view(torch.int32 if a.dtype == F32 else torch.int16)).sum()))
        got = Call(ops, DC.bounded_mlp(B, T, True, ops.OP16)).run(L)
        ry, rkv, rfq = old_mlp(ops, o, x, pe, W, True)
        y3 = got["queries_out"].contiguous()
        mid = ops.layernorm(ops.gemm(o, W["wco"], W["bco"], residual=x, out_dtype=F32), W["n2w"], W["n2b"], 1e-5, out_dtype=F32)
        for name, a, r in (("mlp: norm2 rows (fp32: out-projection + residual + LayerNorm)", got["queries_mid"], mid),
                           ("mlp: norm3 rows (fp32, behind fc2)", got["queries_out"], ry), ("mlp: kv", got["kv"], rkv), ("mlp: qp_final", got["qp_final"], rfq),
                           ("mlp: kv against gemm_tokens on the kernel's OWN norm3 rows", got["kv"], ops.gemm_tokens(y3, W["wkv"], W["bkv"], addend=pe, add_cols=CI)),
                           ("mlp: qp_final against gemm_tokens on the kernel's OWN norm3 rows", got["qp_final"],
                            ops.gemm_tokens(y3, W["wfq"], W["bfq"], addend=pe, add_cols=CI))):
            it = torch.int32 if a.dtype == F32 else torch.int16
            n, d = total.get(name, (0, 0))
            total[name] = (n + a.numel(), d + int((a.view(it) != r.reshape(a.shape).view(it)).sum()))
        assert R <= DC.MAXR
    for name, (n, d) in total.items():
        print(f"BITDIFF {name}: {d} of {n} elements differ from the launches replaced")


@pytest.mark.parametrize("B,T", [(3, 9), (2, 16)], ids=lambda v: str(v))
def test_token_order(ops, L, B, T):
    """images permuted: every output's row blocks permuted, bit for bit; the T rows of every image permuted: bit for bit for dec_tail and
    dec_mlp + dec_kv (per-row arithmetic), inside the bound for dec_self (its softmax sums over the keys in another order)"""
    g = torch.Generator().manual_seed(9)
    ip = torch.randperm(B, generator=g)
    rp = torch.randperm(T, generator=g)
    img = (ip[:, None] * T + torch.arange(T)[None, :]).reshape(-1)
    row = (torch.arange(B)[:, None] * T + rp[None, :]).reshape(-1)
    for E in bounded_cases(B, T, ops.OP16, False):
        base = Call(ops, E).run(L)
        for perm, what in ((img, "images"), (row, "rows")):
            E2 = dict(E, **{k: E[k][perm] for k in ("x", "pe", "o") if E.get(k) is not None})
            got = Call(ops, E2).run(L)
            for name in base:
                a, b_ = got[name], (base[name][:, perm.to(DEV)] if name == "ws" else base[name][perm.to(DEV)])
                if E["kind"] == "self" and what == "rows":
                    continue
                bits_equal(a, b_.contiguous(), f"{E['kind']} {what} permuted, {name}")
            if E["kind"] == "self" and what == "rows":
                for name, g_, ref, bnd in DC.bounded_checks(E2, {k: v.cpu() for k, v in got.items()}, ops.OP16):
                    inside(g_, ref, bnd, f"self rows permuted: {name}")


def test_all_eight_kernels_were_reached(ops):
    """by name, under torch.profiler, in the tests above (this test runs behind them)"""
    print("reached:", sorted(REACHED))
    for k in sorted(WORST):
        print(f"SUMMARY {k}: {WORST[k]:.4f}")
    assert set(DC.KERNELS) <= REACHED, sorted(set(DC.KERNELS) - REACHED)


def test_same_file_on_the_bf16_library(ops):
    """the operand type is a property of the loaded library: the tests of this file once more in a child process on libmsam2_hip_bf16.so"""
    if os.environ.get("MSAM2_LIB_PATH"):
        assert str(ops.OP16).endswith(os.environ.get("MSAM2_EXPECT_OP16", "")), ops.OP16
        return                                              # this IS a run on a chosen library
    lib = os.path.join(ROOT, "medical-sam2_amd", "libmsam2_hip_bf16.so")
    assert os.path.exists(lib), "libmsam2_hip_bf16.so is built by __graft_entry__.build()"
    env = dict(os.environ, MSAM2_LIB_PATH=lib, MSAM2_EXPECT_OP16="bfloat16", PYTHONUNBUFFERED="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider", "-s"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    lines = (r.stdout + r.stderr).splitlines()
    print("bf16 library:\n" + "\n".join(ln.lstrip(".") for ln in lines if ln.lstrip(".").startswith(("BITDIFF", "reached:", "SUMMARY"))))
    tail = "\n".join(lines[-30:])
    print(tail)
    assert r.returncode == 0 and " passed" in tail and "failed" not in tail, tail
