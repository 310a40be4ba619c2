"""Case table, dispatch restatement, operand builders, float64 reference, error bound, rounding emulation and simulated defects of the
attention-backward kernel-variant matrix (csrc/attention_bwd.hip: msam2_attention_bwd / msam2_attention_bwd_dropout).

Plain torch, no GPU needed: tests/test_attention_bwd_variants_gpu.py runs the cases on the card (device="cuda"),
tests/test_attention_bwd_cases_cpu.py proves on the CPU that the passes hold for a correct kernel and fail for a wrong one.

A problem X holds q [B, H, Lq, D], k / v [B, H, Lk, D], g = dO [B, H, Lq, D] in float64, already exact in the types the entry takes (q, k, v
in the 16-bit operand type, dO in fp32), the forward's results o (rounded to 16 bits) and lse (log2 domain, rounded to fp32) computed in
float64 from those operands, and the keep mask of the dropout cases reproduced on the host (backward_bounds.dropout_keep_np).  The kernels
are so checked against their own contract
    P = exp2(s scale log2e - lse),  dP = mask o (dO V^T) / (1 - p),  delta = rowsum(dO o O),  dS = P o (dP - delta),
    dQ = scale dS K,  dK = scale dS^T Q,  dV = (mask o P / (1 - p))^T dO
and an error of the forward can neither cause nor hide a failure.

The three passes:
  sel   integer operands as in the forward's selection pass (attention_cases): key j carries the +-1 code of its index in nb channels, query
        i carries s times the code of its target, score margin GAP bits; dO holds integers in [-2, 2].  P is one-hot after the 16-bit
        rounding, so dV[j] is the integer sum of the dO rows of the queries that select j and a zero row for a key nobody selects:
        compared bit for bit (fp16 build; the bf16 type keeps the 2^-GAP probabilities of the other keys, so there the comparison allows
        int_slack()).  dQ and dK are zero up to the bound.
  tie   the same with pairs of keys (j1, j2): K[j2] = K[j1] + w with an integer w in channels where every query is zero, V[j2] = V[j1] +
        4 sigma (sigma: +1 in two channels).  Both scores are equal, P = (1/2, 1/2), O = V[j1] + 2 sigma exactly.  With x_i = dO_i .
        (V[j1] - V[j2]) / 4:  dQ[i] = -scale x_i w,  dK[j1] = -dK[j2] = scale sum_i x_i q_i,  dV[j1] = dV[j2] = sum_i dO_i / 2.  scale is a
        power of two, dO has four non-zero channels per row (so that the other keys' weights round to zero in fp16) and every value is
        a small integer times a power of two: dQ, dK and dV are compared bit for bit (fp16 build; bf16: int_slack()).
        The code channels are [0, nb) in even (batch, head) instances and [D / 2, D / 2 + nb) in odd ones; w fills every other channel
        with values in +-{1, 2, 3}.  With two or more instances every dQ channel is non-zero for some query; in the single-instance
        shapes (C2, C6, C8) the nb code channels of dQ are pinned by the bounded pass only, those of dK by this pass.
  rand  randn operands in which every edge key (edge_keys) is the dominant key of some query by about 8 natural units and every edge query
        row (edge_queries) has a dominant key and a dO row three times the average; with the dropout mask where the case has one.  Every
        element within attention_bwd_error_bound().  C8 makes queries 0, 31 and 39 "cold": every scaled score below -120.

Largest |emulation - float64 reference| / bound over every element of every case (tests/test_attention_bwd_cases_cpu.py,
test_emulation_stays_within_the_bound, B * H cut to 2), fp16 / bf16:
             dq              dk              dv
    sel      0.000 / 0.000   0.004 / 0.824   0.005 / 0.271
    tie      0.005 / 0.874   0.002 / 0.772   0.005 / 0.094
    rand     0.593 / 0.647   0.642 / 0.638   0.839 / 0.933
The bound is judged on the rand pass.  With fp16 operands the integer passes have no rounding error of their own (that is what makes
them exact): what is left is the fp32 rounding of lse against a bound that cannot know that the operands are integers, so their ratios
say nothing about its slack; with bf16 the other keys' 2^-GAP weights survive and the ratios are ordinary.
"""
import math
import os

import numpy as np
import torch

import backward_bounds as BB
from attention_cases import GAP, LOG2E, U, code, split_bounds, u16, v_pattern

NO_DMA = "MSAM2_BWD_NO_DMA" in os.environ          # read once per process by the library: the GPU file runs these cases in child processes
ROLE_DQ, ROLE_DK, ROLE_DV = 0, 1, 2
ALL_D = (64, 96, 128, 256)
SEED, OFFSET = 0x1234567890ABCDEF, (5 << 40) + 1234567          # the dropout cases' counter stream: offset above 2^32
SEED_DEV = 0x1111                                               # the part of SEED that the second launch passes on the device


# ---------------------------------------------------------------------------------------------------------------------------------
# dispatch (dq_key_splits, launch_fill, launch_role_t of csrc/attention_bwd.hip)
def cdiv(a, b):
    return -(-a // b)


def dq_key_splits(B, H, Lq, Lk):
    blocks4 = cdiv(Lq, 128) * H * B
    if blocks4 >= 512:
        return 1
    return max(1, min(8, cdiv(512, blocks4), cdiv(Lk, 32) // 8))


def role_nw(role, B, H, Lq, Lk):
    n_own = Lq if role == ROLE_DQ else Lk
    ksplit = dq_key_splits(B, H, Lq, Lk) if role == ROLE_DQ else 1
    return 4 if cdiv(n_own, 128) * H * B * ksplit >= 256 or n_own <= 32 else 2


def expected_kernels(c, no_dma):
    """kernel keys (helpers.kernel_key) that one call of the case launches"""
    B, H, Lq, Lk, D = c["B"], c["H"], c["Lq"], c["Lk"], c["D"]
    name = "attn_bwd_dma_kernel" if D in (128, 256) and not no_dma else "attn_bwd_kernel"
    drop = "true" if c["p"] else "false"
    out = {f"attn_bwd_prep_kernel<{D}>"} | {f"{name}<{D},{role_nw(r, B, H, Lq, Lk)},{r},{drop}>" for r in (ROLE_DQ, ROLE_DK, ROLE_DV)}
    if dq_key_splits(B, H, Lq, Lk) > 1:
        out.add("attn_bwd_reduce_kernel")
    return out


ALL_KERNELS = ([f"attn_bwd_kernel<{D},{NW},{R},{dr}>" for D in ALL_D for NW in (2, 4) for R in (0, 1, 2) for dr in ("false", "true")] +
               [f"attn_bwd_dma_kernel<{D},{NW},{R},{dr}>" for D in (128, 256) for NW in (2, 4) for R in (0, 1, 2) for dr in ("false", "true")] +
               [f"attn_bwd_prep_kernel<{D}>" for D in ALL_D] + ["attn_bwd_reduce_kernel"])


def workspace_bytes(B, H, Lq, D):
    rows = B * H * Lq
    base = rows * (D * 2 + 4)
    parts = 8 * rows * D * 4 if cdiv(Lq, 128) * H * B < 512 else 0
    return ((base + 255) & ~255) + parts


# ---------------------------------------------------------------------------------------------------------------------------------
# cases: (name, (B, H, Lq, Lk), head dims, layout, then the dispatch worked out by hand: ksplit, NW of the DQ role, NW of the DK / DV roles)
# layout "token": q / k / v / o are [B, H, L, D] views of token-major [B, L, H * D] buffers and dq / dk / dv the three column thirds of
# one [B, L, 3 H D] buffer; "plain": every tensor in a buffer of its own.
SHAPES = [
    ("C1", (1, 2, 77, 100), ALL_D, "token", 1, 2, 2),       # owner tail in the second block (wave 1 wholly invalid); streamed tails 4 and 13
    ("C2", (1, 1, 31, 31), ALL_D, "plain", 1, 4, 4),        # NW = 4 through n_own <= 32; no full streamed tile
    ("C3a", (2, 1, 32, 33), ALL_D, "plain", 1, 4, 2),       # the exact-tile boundary on either side
    ("C3b", (2, 1, 33, 32), ALL_D, "plain", 1, 2, 4),
    ("C4", (8, 32, 97, 97), ALL_D, "plain", 1, 4, 4),       # NW = 4 through blocks4 >= 256; the last wave partly valid
    ("C5", (1, 2, 70, 513), ALL_D, "token", 2, 2, 2),       # 17 tiles in 2 splits of 9 and 8; the last tile holds 1 key
    ("C6", (1, 1, 40, 2050), ALL_D, "plain", 8, 2, 2),      # 65 tiles in 8 splits of 9; split 7 holds 2 tiles, the last with 2 keys
    ("C7", (4, 32, 100, 513), ALL_D, "plain", 2, 4, 4),     # 2 splits with NW = 4 in every role
    ("C8", (1, 1, 40, 45), (64, 96, 128), "plain", 1, 2, 2),  # cold rows
]
COLD_ROWS = (0, 31, 39)


def _case(name, shape, D, layout, ksplit, nwq, nwk, p=0.0):
    B, H, Lq, Lk = shape
    return dict(name=name, B=B, H=H, Lq=Lq, Lk=Lk, D=D, layout=layout, p=p, cold=name == "C8", lit=(ksplit, nwq, nwk),
                ksplit=dq_key_splits(B, H, Lq, Lk), passes=("rand",) if p else ("sel", "tie", "rand"))


CASES = [_case(n, s, D, lay, *lit) for n, s, Ds, lay, *lit in SHAPES for D in Ds]
# C9: the DROP instances on C1, C2 and C5 (the entry takes D = 64 too, although the Python wrapper never sends it there)
CASES += [_case("C9" + n, s, D, lay, *lit, p=p) for n, s, Ds, lay, *lit in SHAPES if n in ("C1", "C2", "C5") for p in (0.1, 0.5) for D in Ds]


def case_id(c):
    return f"{c['name']}-D{c['D']}-{c['B']}x{c['H']}x{c['Lq']}x{c['Lk']}" + (f"-p{c['p']}" if c["p"] else "")


def cut(c):
    """the case with B * H cut to at most 2 (CPU companion); the key split stays the table's"""
    c = dict(c)
    c["B"], c["H"] = (1, min(c["H"], 2)) if c["H"] > 1 else (min(c["B"], 2), 1)
    return c


def tie_scale(D):
    return 2.0 ** -3 if D <= 96 else 2.0 ** -4


# ---------------------------------------------------------------------------------------------------------------------------------
# edges
def edge_keys(Lk, ksplit):
    """first and last key, both sides of every split boundary (split_bounds) and of the first and last tile boundary, the 1- or 2-key tail"""
    out = [Lk - 1, 0]
    for b in split_bounds(Lk, ksplit, 32)[1:-1]:
        out += [b - 1, b]
    last = (Lk - 1) // 32 * 32
    out += [last, last - 1, 31, 32, Lk - 2]
    seen, res = set(), []
    for t in out:
        if 0 <= t < Lk and t not in seen:
            seen.add(t)
            res.append(t)
    return res


def edge_queries(Lq):
    """first and last row and both sides of every 32-row boundary (the NW * 32-row boundaries are among them)"""
    out = [0, Lq - 1]
    for b in range(32, Lq, 32):
        out += [b - 1, b]
    return sorted(set(out))


def tie_pairs(Lk, ksplit):
    """(j1, j2): inside one tile, across the first tile boundary, across every split boundary, the last full tile with the tail"""
    cand = [(4, 9), (31, 32)] + [(b - 1, b) for b in split_bounds(Lk, ksplit, 32)[1:-1]]
    full = Lk // 32 * 32
    cand += [(full - 2, Lk - 1)] if Lk % 32 and full else [(Lk - 3, Lk - 1)]
    pairs, used = [], set()
    for a, b in cand:
        if 0 <= a < b < Lk and a not in used and b not in used:
            pairs.append((a, b))
            used |= {a, b}
    return pairs


class Problem:
    pass


def keep_mask(B, H, Lq, Lk, p, device, transposed=False, shift=0):
    """the forward's keep mask [B, H, Lq, Lk]: element (b, h, i, j) is number OFFSET + ((b H + h) Lq + i) Lk + j of the counter stream.
    transposed / shift: the index a defective kernel would use"""
    bh = np.arange(B * H, dtype=np.uint64)[:, None, None] * np.uint64(Lq * Lk)
    i, j = np.arange(Lq, dtype=np.uint64)[None, :, None], np.arange(Lk, dtype=np.uint64)[None, None, :]
    idx = np.uint64(OFFSET + shift) + bh + (j * np.uint64(Lq) + i if transposed else i * np.uint64(Lk) + j)
    return torch.from_numpy(BB.dropout_keep_np(SEED, idx, BB.dropout_thr(p))).view(B, H, Lq, Lk).to(device)


def finish(X, op16=None):
    """o (16-bit) and lse (fp32, log2 domain) of the float64 forward, with the mask where there is one"""
    s = (X.q @ X.k.transpose(2, 3)) * (X.scale * LOG2E)
    m = s.max(-1, keepdim=True).values
    e = torch.exp2(s - m)
    l = e.sum(-1, keepdim=True)
    X.lse_true = (m + torch.log2(l))[..., 0]
    X.lse = X.lse_true.float().double()
    pm = e / l
    if X.keep is not None:
        pm = pm * X.keep / (1.0 - X.p)
    o = pm @ X.v
    X.o = o.to(op16).double() if op16 is not None else o
    return X


def build(c, kind, device="cpu", op16=torch.float16):
    X = Problem()
    B, H, Lq, Lk, D, ks = c["B"], c["H"], c["Lq"], c["Lk"], c["D"], c["ksplit"]
    X.c, X.kind, X.p, X.ksplit, X.keep = c, kind, float(np.float32(c["p"])), ks, None          # p as the entry's fp32 argument
    X.scale = tie_scale(D) if kind == "tie" else float(np.float32(D ** -0.5))
    n = torch.arange(B, device=device)[:, None] * H + torch.arange(H, device=device)[None, :]          # instance number [B, H]
    i = torch.arange(Lq, device=device)
    if kind == "rand":
        g_ = torch.Generator(device=device).manual_seed(4000 + 7 * Lq + 3 * Lk + D + B * H)
        q = torch.randn(B, H, Lq, D, generator=g_, device=device) * 2.0
        k = torch.randn(B, H, Lk, D, generator=g_, device=device)
        v = torch.randn(B, H, Lk, D, generator=g_, device=device)
        g = torch.randn(B, H, Lq, D, generator=g_, device=device)
        ek, eq = edge_keys(Lk, ks), edge_queries(Lq)
        order = eq + [r for r in range(Lq) if r not in eq]
        assert len(ek) <= Lq, "more edge keys than queries"
        beta = 8.0 / (math.sqrt(D) - 3.5) / (X.scale * math.sqrt(D))
        X.dominant = {}
        for idx in range(max(len(ek), len(eq))):
            row, key = order[idx], ek[idx % len(ek)]
            q[:, :, row] = beta * k[:, :, key] + 0.3 * q[:, :, row]
            X.dominant[row] = key
        for row in eq:
            g[:, :, row] *= 3.0
        if c["cold"]:
            k[..., 0] = 4.0                                     # a channel all keys share shifts every score of a row alike
            for row in COLD_ROWS:
                q[:, :, row, 0] = -150.0 / (X.scale * 4.0)
            g[:, :, COLD_ROWS[1]] = 0.0                         # delta = 0 exactly: inf * 0 before any clamp
        X.q, X.k, X.v = (t.to(op16).double() for t in (q, k, v))
        X.g = g.float().double()
        if c["p"]:
            X.keep = keep_mask(B, H, Lq, Lk, c["p"], device).double()
        return finish(X, op16)
    tie = kind == "tie"
    nb = max(1, (Lk - 1).bit_length())
    s = float(math.ceil(GAP / (2 * LOG2E * X.scale)))
    assert s <= 256 and nb <= D // 2 - 8
    spec = edge_keys(Lk, ks)
    nn = n[:, :, None]
    walk = (37 * (i[None, None, :] // 2) + 5 + 11 * nn) % Lk
    spec_t = torch.tensor(spec, device=device)[(i[None, None, :] + nn) % len(spec)]
    t = torch.where(i[None, None, :] < 2 * len(spec), spec_t, walk)                      # [B, H, Lq]: every edge key twice where Lq allows
    jk = torch.arange(Lk, device=device)
    rep = jk.clone()
    pairs = tie_pairs(Lk, ks) if tie else []
    pair_of = torch.full((Lk,), -1, dtype=torch.long, device=device)
    for pi, (a, b) in enumerate(pairs):
        rep[b] = a
        pair_of[a] = pi
    if tie:
        a_t = torch.tensor([a for a, _ in pairs], device=device)[(i[None, None, :] + nn) % len(pairs)]
        t = torch.where((i[None, None, :] < 3 * len(pairs)) | (i[None, None, :] % 3 == 0), a_t, rep[t])
    off = (n % 2) * (D // 2)                                                            # first code channel [B, H]
    ch = torch.arange(D, device=device)
    is_code = (ch[None, None, :] >= off[..., None]) & (ch[None, None, :] < off[..., None] + nb)      # [B, H, D]
    pos = (ch[None, None, :] - off[..., None]).clamp(0, nb - 1)                          # bit number of a code channel
    kc = torch.gather(code(rep, nb)[None, None].expand(B, H, Lk, nb), 3, pos[:, :, None, :].expand(B, H, Lk, D))
    k = kc * is_code[:, :, None, :]
    qc = torch.gather(code(t, nb), 3, pos[:, :, None, :].expand(B, H, Lq, D))
    q = s * qc * is_code[:, :, None, :]
    v = v_pattern(jk[None, None, :] + 13 * nn, ch, tie)                                  # [B, H, Lk, D]
    if not tie:
        g = ((7 * i[None, None, :, None] + 3 * ch[None, None, None, :] + 5 * nn[..., None]) % 5 - 2).double().expand(B, H, Lq, D).clone()
    else:
        wvals = torch.tensor([1., -2., 3., -1., 2., -3.], dtype=torch.float64, device=device)
        g = torch.zeros(B, H, Lq, D, dtype=torch.float64, device=device)
        pi_q = pair_of[t]                                                               # pair a query looks at, or -1
        sa = (5 * pi_q.clamp_min(0) + 3 * (pi_q < 0) * i[None, None, :]) % D             # sigma's channels: sa and sa + 17
        for dch, val in ((0, 1.0 + (i % 2)), (17, torch.where((i // 2) % 2 == 1, 1.0, -3.0)), (40, 2.0 - (i % 3)), (57, (i % 4) - 1.0)):
            g.scatter_(3, ((sa + dch) % D)[..., None], val.double()[None, None, :, None].expand(B, H, Lq, 1))
        for pi, (a, b) in enumerate(pairs):
            w = wvals[(ch + pi) % 6][None, None, :] * ~is_code                            # [B, H, D]
            k[:, :, b] = k[:, :, a] + w
            sig = torch.zeros(D, dtype=torch.float64, device=device)
            sig[(5 * pi) % D] = sig[(5 * pi + 17) % D] = 1.0
            v[:, :, b] = v[:, :, a] + 4.0 * sig
        X.pairs, X.w_of = pairs, lambda pi: wvals[(ch + pi) % 6][None, None, :] * ~is_code
    X.q, X.k, X.v, X.g, X.t, X.is_code, X.s = q, k, v, g, t, is_code, s
    for tns in (q, k, v):
        assert torch.equal(tns.to(torch.bfloat16).double(), tns), "integer operands must be exact in both 16-bit types"
    finish(X, None)
    o16 = X.o.to(torch.float16).double()                                                # V[t] or V[j1] + 2 sigma: |.| <= 34, exact in both types
    assert float((o16 - X.o).abs().max()) < 1e-6 and torch.equal(o16.to(torch.bfloat16).double(), o16) and torch.equal(o16, o16.round())
    X.o = o16
    # closed forms
    P1 = torch.zeros(B, H, Lq, Lk, dtype=torch.float64, device=device)
    P1.scatter_(3, t[..., None], 1.0)
    x = torch.zeros(B, H, Lq, dtype=torch.float64, device=device)
    for a, b in pairs:
        on = (t == a).double()
        P1[..., a] = 0.5 * on
        P1[..., b] = 0.5 * on
        x = x + on * ((g * (v[:, :, a] - v[:, :, b])[:, :, None, :]).sum(-1) / 4.0)
    X.P = P1
    X.exp_dv = P1.transpose(2, 3) @ g
    X.abs_dv = P1.transpose(2, 3) @ g.abs()                                           # the closed forms' sums of absolute terms
    X.exp_dq, X.exp_dk, X.abs_dq, X.abs_dk = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(q), torch.zeros_like(k)
    for a, b in pairs:
        on = (t == a).double() * x
        X.exp_dq = X.exp_dq + X.scale * on[..., None] * (k[:, :, a] - k[:, :, b])[:, :, None, :]
        X.abs_dq = X.abs_dq + X.scale * on.abs()[..., None] * (k[:, :, a].abs() + k[:, :, b].abs())[:, :, None, :]
        dk1 = X.scale * (on[..., None] * q).sum(2)
        X.exp_dk[:, :, a], X.exp_dk[:, :, b] = dk1, -dk1
        X.abs_dk[:, :, a] = X.abs_dk[:, :, b] = X.scale * (on.abs()[..., None] * q.abs()).sum(2)
    return X


def int_slack(X, fp16):
    """What the bit-for-bit comparisons of the integer passes allow, per element.  fp16: nothing -- the other keys' weights, below
    2^-(GAP-1) times |dP - delta| <= 2 * 4 * 3 * 19 in the tie pass and 2^-(GAP-1) itself in the DV role, lie under half the smallest fp16
    subnormal (2^-25) and round to zero, and every sum is one of integers.  bf16 has fp32's exponent range and keeps them: n weights of at
    most 2^-(GAP-1) T each, T the largest |dP - delta| times the largest streamed operand; and with them in the sum its fp32
    accumulation over the n streamed rows rounds: ((1 + u)^(n + 2) - 1) times the sum of the closed form's absolute terms."""
    if fp16:
        return dict(dq=torch.zeros_like(X.exp_dq), dk=torch.zeros_like(X.exp_dk), dv=torch.zeros_like(X.exp_dv))
    e = 2.0 ** -(GAP - 1)
    Lq, Lk = X.q.shape[2], X.k.shape[2]
    gm, T = float(X.g.abs().max()), 2 * 4 * 3 * 19.0
    aq, ak = (1 + U) ** (32 * cdiv(Lk, 32) + X.ksplit + 2) - 1, (1 + U) ** (32 * cdiv(Lq, 32) + 2) - 1
    return dict(dq=e * Lk * T * 3.0 * X.scale + aq * X.abs_dq, dk=e * Lq * T * X.s * X.scale + ak * X.abs_dk, dv=e * Lq * gm + ak * X.abs_dv)


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 reference (the entry's definition), with the simulated defects
DEFECTS = [
    "last key dropped", "last key counted twice (dQ)", "one key tile skipped (dQ)", "one query tile skipped (dK, dV)",
    "tail tile not masked: zero K rows at weight 2^-lse (dQ)", "one split's partial left out", "one split's partial summed twice",
    "channels 8g+4h and 8g+4(1-h) swapped in dQ", "channels 8g+4h and 8g+4(1-h) swapped in dK", "channels 8g+4h and 8g+4(1-h) swapped in dV",
    "owner row oi written to oi+32 in dQ", "owner row oi written to oi+32 in dK", "owner row oi written to oi+32 in dV",
    "delta taken from the neighbouring row", "delta omitted", "scale missing on dK",
    "dropout mask indexed transposed (dQ)", "dropout mask offset by one key (dK, dV)", "1/(1-p) missing in dV",
]


def applies(c, name):
    """None where defect `name` applies to case c, otherwise the reason why it cannot"""
    Lq, Lk = c["Lq"], c["Lk"]
    if name == "last key counted twice (dQ)" and Lk % 32 == 0:
        return "no partial key tile: nothing is clamped"
    if name == "one key tile skipped (dQ)" and Lk <= 32:
        return "a single key tile"
    if name == "one query tile skipped (dK, dV)" and Lq <= 32:
        return "a single query tile"
    if name.startswith("tail tile not masked") and not c["cold"]:
        return "harmless here: a finite weight times a zero K row"
    if "split" in name and c["ksplit"] == 1:
        return "no key split"
    if name.endswith("in dQ") and name.startswith("owner") and Lq <= 32:
        return "a single 32-row owner block (the write would land outside the view: the sentinels see it)"
    if name.startswith("owner") and not name.endswith("in dQ") and Lk <= 32:
        return "a single 32-row owner block (the write would land outside the view: the sentinels see it)"
    if ("dropout" in name or "1/(1-p)" in name) and not c["p"]:
        return "no dropout"
    return None


def _swap(t):
    """channels 8..11 and 12..15 of the last 32-channel block exchanged (g = 1, h <-> 1 - h of the transposed epilogue)"""
    D = t.shape[-1]
    idx = torch.arange(D, device=t.device)
    b = D - 32
    idx[b + 8:b + 12], idx[b + 12:b + 16] = torch.arange(b + 12, b + 16, device=t.device), torch.arange(b + 8, b + 12, device=t.device)
    return t[..., idx]


def _shift32(t):
    out = t.clone()
    n = t.shape[2]
    out[:, :, 32:min(64, n)] = t[:, :, :min(64, n) - 32]
    out[:, :, :32] = 0.0
    return out


def reference(X, defect=None, lse=None):
    """(dq, dk, dv) in float64 by the entry's definition from X's operands; `defect`: what a kernel with that defect would return"""
    q, k, v, g, o = X.q, X.k, X.v, X.g, X.o
    lse = X.lse if lse is None else lse
    B, H, Lq, D = q.shape
    Lk, ks, dev = k.shape[2], X.ksplit, q.device
    P = torch.exp2((q @ k.transpose(2, 3)) * (X.scale * LOG2E) - lse[..., None])
    M = X.keep / (1.0 - X.p) if X.keep is not None else torch.ones((), dtype=torch.float64, device=dev)
    delta = (g * o).sum(-1, keepdim=True)
    Pq, Pk, Mq, Mk, Mv = P, P, M, M, M
    wk, wq = torch.ones(Lk, dtype=torch.float64, device=dev), torch.ones(Lq, dtype=torch.float64, device=dev)
    b = split_bounds(Lk, ks, 32)
    if defect == "last key dropped":
        wk[-1] = 0.0
        Pq = Pk = P * wk
    elif defect == "last key counted twice (dQ)":
        wk[-1] = 2.0
        Pq = P * wk
    elif defect == "one key tile skipped (dQ)":
        t0 = b[ks - 1] if ks > 1 else (cdiv(Lk, 32) - 2) * 32              # first tile of the last split / the last full tile
        wk[t0:t0 + 32] = 0.0
        Pq = P * wk
    elif defect == "one query tile skipped (dK, dV)":
        t0 = (cdiv(Lq, 32) - 2) * 32
        wq[t0:t0 + 32] = 0.0
        Pk = P * wq[:, None]
    elif defect == "one split's partial left out":
        wk[b[ks - 1]:] = 0.0
        Pq = P * wk
    elif defect == "one split's partial summed twice":
        wk[b[ks - 1]:] = 2.0
        Pq = P * wk
    elif defect == "delta taken from the neighbouring row":
        delta = delta[:, :, (torch.arange(Lq, device=dev) ^ 1).clamp_max(Lq - 1)]
    elif defect == "delta omitted":
        delta = torch.zeros_like(delta)
    elif defect == "dropout mask indexed transposed (dQ)":
        Mq = keep_mask(B, H, Lq, Lk, X.p, dev, transposed=True).double() / (1.0 - X.p)
    elif defect == "dropout mask offset by one key (dK, dV)":
        Mk = Mv = keep_mask(B, H, Lq, Lk, X.p, dev, shift=1).double() / (1.0 - X.p)
    dP = g @ v.transpose(2, 3)
    dq = X.scale * ((Pq * (dP * Mq - delta)) @ k)
    dk = X.scale * ((Pk * (dP * Mk - delta)).transpose(2, 3) @ q)
    dv = (Pk * Mv).transpose(2, 3) @ g
    if defect is not None:
        if defect.startswith("tail tile not masked"):
            w = (torch.exp2(-lse).float() * (0.0 - delta[..., 0]).float())          # fp32: overflows for a cold row
            dq = dq + (w * 0.0).double()[..., None]                                 # inf * 0
        elif defect == "scale missing on dK":
            dk = dk / X.scale
        elif defect == "1/(1-p) missing in dV":
            dv = dv * (1.0 - X.p)
        elif defect.startswith("channels"):
            dq, dk, dv = (_swap(t) if defect.endswith(n) else t for t, n in ((dq, "dQ"), (dk, "dK"), (dv, "dV")))
        elif defect.startswith("owner"):
            dq, dk, dv = (_shift32(t) if defect.endswith(n) else t for t, n in ((dq, "dQ"), (dk, "dK"), (dv, "dV")))
    return dict(dq=dq, dk=dk, dv=dv)


# ---------------------------------------------------------------------------------------------------------------------------------
# The bound.  u = 2^-24, h = u16 (2^-11 fp16, 2^-8 bf16); every factor below is used as a product (1 + a)(1 + b) .. - 1, so no second-order
# term is dropped, and every error multiplies the ABSOLUTE terms of the element it belongs to (computed in float64).
#   exponent   e = fl(fl(s32 * sl2) - lse): s32 is the MFMA's fp32 sum of D exact products, |s32 - s| <= ((1 + u)^D - 1) sabs with sabs =
#              sum_d |q k|; sl2 = fl(scale * 1.44269504f) is c2 = scale log2(e) to within (1 + u)^2; one rounding for the product and one
#              for the difference x = s c2 - lse: |e - x| <= de = ((1 + u)^(D + 3) - 1) c2 sabs + u |x| (+ extra_de: an lse that is itself
#              only known to a bound).
#   P          the hardware exp2 is good to one ulp, a relative 2u: P_kernel = P (1 + rp), rp = 2^de (1 + 2u) - 1.
#   dO         rounded to 16 bits by the pre-pass: the actual differences gerr = |r16(dO) - dO| are known from the input and the type.
#   dP         fp32 sum over D of exact products of 16-bit values: |dP_kernel - dP| <= edp = gerr |V|^T + ((1 + u)^D - 1) (|dO| + gerr) |V|^T;
#              the mask factor 1 / (1 - p) is 1.f / (1.f - p), two roundings, and its product one more: (1 + u)^3.
#   delta      fp32 from the unrounded dO: a product, 3 additions in the lane, 6 shuffle steps: edelta = ((1 + u)^11 - 1) sum_d |dO O|.
#   t          = dP m - delta, one more rounding: et = edpm + edelta + u (|t| + edpm + edelta).
#   wf         the weight tile, rounded to 16 bits: wf = f2op(fl(P_kernel t_kernel)).  |wf - P t| <= ewf = P (1 + rp)(1 + u)(1 + h)(|t| + et) - P |t|
#              + tiny, tiny = 2^-25 in fp16 (half the subnormal spacing: below 2^-14 the conversion's error is absolute) and FLUSH =
#              2^-126 in bf16, whose range is fp32's: what lies below the smallest normal fp32 number may be flushed to zero.  The same
#              FLUSH applies to P (times |t| + et) and to every output element.
#              DV role: wf = f2op(fl(P_kernel m)): ewf = P m ((1 + rp)(1 + u)^3 (1 + h) - 1) + tiny.
#   out        fp32 accumulation over the n streamed rows (32 per tile, zero rows included), in any order, then over the ksplit partial
#              rows, then the factor scale: acc = (1 + u)^(n + ksplit + 1) - 1 on sum |wf| |operand|, where |wf| <= P |t| + ewf and the
#              operand of the DV role is r16(dO), |.| <= |dO| + gerr.
FLUSH = 2.0 ** -126


def attention_bwd_error_bound(X, fp16, extra_de=None):
    """{dq, dk, dv}: largest |kernel - reference(X)| of a correct kernel, element by element"""
    q, k, v, g, o = X.q, X.k, X.v, X.g, X.o
    D, Lq, Lk = q.shape[3], q.shape[2], k.shape[2]
    h, tiny = u16(fp16), (2.0 ** -25 if fp16 else FLUSH)
    c2 = X.scale * LOG2E
    s = q @ k.transpose(2, 3)
    x = s * c2 - X.lse[..., None]
    P = torch.exp2(x)
    de = ((1 + U) ** (D + 3) - 1) * c2 * (q.abs() @ k.abs().transpose(2, 3)) + U * x.abs()
    if extra_de is not None:
        de = de + extra_de[..., None]
    rp1 = torch.exp2(de) * (1 + 2 * U)                                       # 1 + rp
    M = X.keep / (1.0 - X.p) if X.keep is not None else torch.ones((), dtype=torch.float64, device=q.device)
    md = (1 + U) ** 3 if X.keep is not None else 1.0
    gerr = (g.to(torch.float16 if fp16 else torch.bfloat16).double() - g).abs()
    va = v.abs().transpose(2, 3)
    dP = g @ v.transpose(2, 3)
    edp = gerr @ va + ((1 + U) ** D - 1) * ((g.abs() + gerr) @ va)
    edpm = (edp * md + (md - 1) * dP.abs()) * M
    delta = (g * o).sum(-1, keepdim=True)
    edelta = ((1 + U) ** 11 - 1) * (g * o).abs().sum(-1, keepdim=True)
    t = dP * M - delta
    et = edpm + edelta + U * (t.abs() + edpm + edelta)
    ewf = (P * rp1 + FLUSH) * (1 + U) * (1 + h) * (t.abs() + et) - P * t.abs() + tiny
    W = P * t.abs() + ewf
    nk, nq = 32 * cdiv(Lk, 32), 32 * cdiv(Lq, 32)
    out = {}
    acc = (1 + U) ** (nk + X.ksplit + 1) - 1
    out["dq"] = X.scale * (ewf @ k.abs() + acc * (W @ k.abs())) + FLUSH
    acc = (1 + U) ** (nq + 2) - 1
    out["dk"] = X.scale * (ewf.transpose(2, 3) @ q.abs() + acc * (W.transpose(2, 3) @ q.abs())) + FLUSH
    ewv = P * M * (rp1 * md * (1 + h) - 1) + FLUSH * M * md * (1 + h) + tiny
    Wv, ga = P * M + ewv, g.abs() + gerr
    out["dv"] = (Wv.transpose(2, 3) @ ga - (P * M).transpose(2, 3) @ g.abs()) + ((1 + U) ** (nq + 1) - 1) * (Wv.transpose(2, 3) @ ga) + FLUSH
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
def emulate(X, fp16, round_do=True):
    """the kernels' arithmetic in float64 with their roundings at their places (sums are taken exactly and rounded once)"""
    dt = torch.float16 if fp16 else torch.bfloat16
    r32 = lambda a: a.float().double()
    r16 = (lambda a: a.clamp(-65504.0, 65504.0).float().to(dt).double()) if fp16 else (lambda a: a.float().to(dt).double())
    q, k, v, g, o = X.q, X.k, X.v, X.g, X.o
    Lk, ks = k.shape[2], X.ksplit
    g16 = r16(g) if round_do else g
    sl2 = float(np.float32(np.float32(X.scale) * np.float32(1.4426950408889634)))
    pe = r32(torch.exp2(r32(r32(r32(q @ k.transpose(2, 3)) * sl2) - X.lse[..., None])))
    if X.keep is not None:
        m = X.keep * float(np.float32(1.0) / (np.float32(1.0) - np.float32(X.p)))
    else:
        m = torch.ones((), dtype=torch.float64, device=q.device)
    dp = r32(g16 @ v.transpose(2, 3))
    delta = r32((g * o).sum(-1, keepdim=True))
    wf = r16(r32(pe * r32(r32(dp * m) - delta)))
    b = split_bounds(Lk, ks, 32)
    dq = 0.0
    for sp in range(ks):
        dq = r32(dq + r32(X.scale * r32(wf[..., b[sp]:b[sp + 1]] @ k[:, :, b[sp]:b[sp + 1]])))
    dk = r32(X.scale * r32(wf.transpose(2, 3) @ q))
    dv = r32(r16(r32(pe * m)).transpose(2, 3) @ g16)
    return dict(dq=dq, dk=dk, dv=dv)
