"""Case tables, operand builders, exactness conditions, float64 references, bounds and simulated defects of the variant matrix of the
decoder token kernels: dec_self_kernel, dec_mlp_kernel, dec_kv_kernel, dec_tail_kernel (csrc/decoder_tokens.hip) and the
key-split producer attn_fewq16_part_kernel<1|2|4|8> (csrc/attention.hip, msam2_attention_fewq_keysplit), whose partials only they read.

Plain torch on the CPU, no GPU needed: tests/test_dectok_variants_gpu.py moves the operands to the card and runs them,
tests/test_dectok_cases_cpu.py proves that the builders' conditions hold, that the fp32 restatement of the kernels gives the expected bits
and that every simulated defect of DEFECTS fails a case.

Exact pass -- operands for which a correct kernel's 16-bit outputs are known to the bit in fp16 and in bf16:
  * q | k | v: the three weight thirds read RESERVED columns of the token rows only (columns drawn by one seeded permutation, so they
    lie in every 16-wide k-step): KC (the +-1 code of the key's index), QC (per head: SEL times the code of the query's target), VS (the
    source of v).  pe is what puts the codes there (pe = wanted - x), and pe is non-zero in VS, which only `x` may reach.
  * self-attention: D = 32, channel 2 b holds bit b of the code, channel 2 b + 1 an offset (q: -SEL, k: 1), so the fp32 running sum of
    the target's score is +a, 0, +a, 0 ... = 0 exactly and every other key's is <= -2 SEL c ~ -204 in the log2 domain: its probability
    is exactly 0 (2^-204 is no fp32 number), the output is V[t] to the bit.  attention_cases' GAP = 40 leaves 2^-40, which a bf16 V
    element of 0 would show; hence SEL = 400 (25 * 16: exact in bf16) instead of sel_scale(32) = 79.  One tie (K[T - 1] = K[1] in the last
    image, T >= 3): the output is (V[1] + V[T - 1]) / 2.
  * out-projection + residual + LayerNorm: the pre-norm row is m + a s (s balanced +-1: mean and variance exact in any fp32 order), the
    residual is x_target - (o W^T + b).  In dec_self the residual is also the operand of q | k | v, so a is an integer there and W_out
    has no entry in the rows VS (x[VS] is then known before the attention output is).  Under skip_first_layer_pe there is no
    residual: every head targets the same key, V[j] = (a_j / 8) e_j + bias, W_out's column (head, j) is the balanced pattern S_j, and
    the eight heads add up to a_t S_t; b_out absorbs the v bias.  No tie there (a mean of two patterns is no pattern).
  * MLP: hidden units come in quadruples (+-(e_k + r), +-(e_k - r)) with opposite fc2 weights, so relu(t) - relu(-t) = t and fc2 is the
    sparse integer map L = a3 P G^-1 - I of norm2's integers z = s g + b: fc2 + b2 + z = m3 + a3 P s, a target row again -- although
    dec_kv's residual is what norm2 computed (z + delta, |delta| <= 1.7e-4): the builder asserts that norm3 stays inside half a 16-bit
    ulp of its integers.  Hidden pre-activations are integers of both signs in [-87, 87]; every slice's workspace slab is an exact fp32
    matrix and is compared bit for bit, and no two slabs are equal.
  * projections behind a LayerNorm: pe in {-1, 0, 1}, |y + pe| >= 1 (never the rounded value of a cancellation), sparse sign weights,
    bias 70 + a step: every output is a positive integer.
  * the fp32 LayerNorm outputs are compared with the float64 LayerNorm of the exact pre-norm row inside ln_bound_exact() (norm3, whose
    row carries norm2's error: ln_bound()), derived from the operation count of sum_res_ln_rows.
Synthetic partials, producer cases and the bounded pass: see partials_exact, producer_sel / producer_rand and bounded.
"""
import math

import torch

import attention_cases as AC
import rowtile_cases as RC
from fused_cases import exact16, r16
from pointwise_bounds import ln_tail, store16

C, NH, CI, HID, SLICE, NSLICE, MAXT, MAXR = 256, 8, 128, 2048, 128, 16, 16, 32
DS, DX = C // NH, CI // NH                 # head dims of the self-attention and of the cross attentions
F32 = torch.float32
U = 2.0 ** -24
SEL = 400.0                                # q = SEL * code: 2 SEL log2(e) / sqrt(32) = 204 bits between the target and every other key
GAP = 200.0                                # what the builders assert: 2^-200 is below the smallest fp32 denormal
EPS = 1e-5
LIVE, EMPTY, DEAD = RC.LIVE, RC.EMPTY, RC.DEAD

# (B, T): T <= 16, B T <= 32 -- a lone token; 32 images of one; 16 lanes with 14 / 13 dead; ragged; half a tile; one over; 15; the T limit
SHAPES = [(1, 1), (32, 1), (16, 2), (10, 3), (1, 7), (4, 8), (3, 9), (2, 15), (1, 16), (2, 16)]
SELF_CASES = [(B, T, skip) for B, T in SHAPES for skip in (False, True)]
# attention output as 16-bit rows (splits 0) or as partials; every split count 1 .. 8 occurs, each shape has rows and two counts
ATTN_FORMS = {bt: (0, 1 + i % 8, 1 + (i + 5) % 8) for i, bt in enumerate(SHAPES)}
MLP_CASES = [(B, T, last, s) for B, T in SHAPES for last in (False, True) for s in ATTN_FORMS[(B, T)]]
TAIL_CASES = [(B, T, s) for B, T in SHAPES for s in ATTN_FORMS[(B, T)]]
assert {s for v in ATTN_FORMS.values() for s in v} == set(range(9))

KERNELS = ["dec_self_kernel", "dec_mlp_kernel", "dec_kv_kernel", "dec_tail_kernel"] + [f"attn_fewq16_part_kernel<{m}>" for m in (1, 2, 4, 8)]

_P = torch.randperm(C, generator=torch.Generator().manual_seed(310))
KC, QC, VS, FREE = _P[:4], _P[4:36].view(NH, 4), _P[36:100], _P[100:]
RESERVED = _P[:100]
assert len(set((RESERVED // 16).tolist())) == 16, "the reserved columns lie in every k-step"


def cdiv(a, b):
    return (a + b - 1) // b


def gen(*key):
    seed = 977
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def ri(g, lo, hi, *s):
    return torch.randint(lo, hi + 1, s, generator=g).double()


def pz(t):
    """-0.0 -> +0.0 (a sum of products that cancel is +0 in every fp32 order)"""
    return t + 0.0


def subset_signs(rows, cols, nnz, g):
    """[rows, C] with nnz entries of +-1 per row, all in the columns `cols`"""
    idx = torch.rand(rows, len(cols), generator=g).argsort(1)[:, :nnz]
    sg = torch.randint(0, 2, (rows, nnz), generator=g).double() * 2 - 1
    return torch.zeros(rows, C, dtype=torch.float64).scatter_(1, cols[idx], sg)


def positive_bias(n):
    """70 + a step with the column and its 32-block: with |a| <= 8 and 8 signs per row every projection is an integer in [6, 137]"""
    return 71.0 + RC.stepped_bias(n, "cpu")


def ln_vectors(g, n=C):
    return (2 * ri(g, 0, 1, n) - 1) * ri(g, 1, 2, n), (2 * ri(g, 0, 1, n) - 1) * ri(g, 4, 5, n)


def ln_dev(a, ln_w, eps):
    """|LayerNorm value - its integer| of a row m + a s: |g| |1 - a / sqrt(a^2 + eps)|"""
    a = torch.as_tensor(a, dtype=torch.float64)
    return float(ln_w.abs().max()) * float((1 - a / torch.sqrt(a * a + eps)).abs().max())


def unit_rows(R, eps, g, a=None, m=None):
    """rowtile_cases.target_rows with integer a in {1, 2, 4} (the rows are 16-bit operands as well) and without the row of mean 1000:
    (x, y, ln_w, ln_b)"""
    s = (torch.rand(R, C, generator=g).argsort(1) < C // 2).double() * 2 - 1
    a = 2.0 ** ri(g, 0, 2, R, 1) if a is None else a
    m = ri(g, -3, 3, R, 1) if m is None else m
    ln_w, ln_b = ln_vectors(g)
    x, y = m + a * s, s * ln_w + ln_b
    assert bool((s.sum(1) == 0).all()) and exact16(x) and exact16(y) and 2 <= float(y.abs().min()) and float(y.abs().max()) <= 7
    assert ln_dev(a, ln_w, eps) < 1.7e-4 < 2.0 ** -9 / 8
    return x, y, ln_w, ln_b


# ---------------------------------------------------------------------------------------------------------------------------------
# the fp32 LayerNorm bound of the exact pass
def ln_bound(pre, ln_w, ln_b, eps, dpre=0.0):
    """(ref, bound): float64 LayerNorm of pre-norm rows that carry the error dpre and the largest error of sum_res_ln_rows on them,
    pointwise_bounds.ln_tail's operation count: the mean over 256 values (4 per lane, 6 shuffle additions, the division), d = v - mean,
    the variance likewise, rstd (addition of eps, square root, division), and d * rstd * w + b (three roundings)."""
    return ln_tail(pre, dpre, ln_w, ln_b, eps)


def ln_bound_exact(pre, ln_w, ln_b, eps):
    """(ref, bound) on a target row m + a s, whose statistics are exact in fp32 in any order (the builders assert it: the row sum is N m,
    d = +-a, sum d^2 = N a^2, N a power of two): what is left are the roundings of var + eps (half a unit on rstd), of the square root
    and of the reciprocal (two units each: a correctly rounded form has one), of d * rstd, of * w (one each) -- 6.5 u, taken as 8 u, on
    |d rstd w| -- and of + b, with the result's own, 2 u |y|.  ln_tail's general bound is no use here: it charges the row of mean 1000
    with the 257 u |mean| of a sum that is exact."""
    x = pre.double()
    d = x - x.mean(1, keepdim=True)
    t = d / torch.sqrt((d * d).mean(1, keepdim=True) + eps) * ln_w
    ref = t + ln_b
    return ref, 8 * U * t.abs() + 2 * U * ref.abs()


# ---------------------------------------------------------------------------------------------------------------------------------
# dec_self
def _targets(B, T, g, per_head):
    t = torch.stack([torch.stack([torch.randperm(T, generator=g) for _ in range(NH)]) for _ in range(B)])       # [B, NH, T]
    return t if per_head else t[:, :1].expand(B, NH, T).contiguous()


def attention_expected(v, rep, t, B, T):
    """[R, C]: row (b, i), head h = the mean of V[b, j, h] over the keys j that carry the K row of t[b, h, i]"""
    vv = v.view(B, T, NH, DS)
    match = (rep[:, None, None, :] == t[..., None]).double()                       # [B, NH, query, key]
    o = torch.einsum("bhij,bjhd->bihd", match, vv) / match.sum(-1).permute(0, 2, 1)[..., None]
    return pz(o.reshape(B * T, C))


def self_exact(B, T, skip):
    g = gen(41, B, T, skip)
    R = B * T
    ar = torch.arange
    tok = ar(T).repeat(B)
    rep = ar(T).repeat(B, 1)                                                        # key -> the key whose K row it carries
    tie = (not skip) and T >= 3
    if tie:
        rep[B - 1, T - 1] = 1
    t = torch.gather(rep[:, None, :].expand(B, NH, T), 2, _targets(B, T, g, not skip))
    kcode = AC.code(rep.reshape(R), 4)                                              # [R, 4]
    qcode = SEL * AC.code(t.permute(0, 2, 1).reshape(R, NH), 4).reshape(R, 4 * NH)  # [R, (head, bit)]
    W, bq = torch.zeros(3 * C, C, dtype=torch.float64), torch.zeros(3 * C, dtype=torch.float64)
    hh = ar(NH)
    for b_ in range(4):
        W[hh * DS + 2 * b_, QC[:, b_]] = 1.0
        W[C + hh * DS + 2 * b_, KC[b_]] = 1.0
        bq[hh * DS + 2 * b_ + 1], bq[C + hh * DS + 2 * b_ + 1] = -SEL, 1.0
    # channels the other side holds 0 in: k 8 .. 19, q 20 .. 31 carry small integers of the v source
    ch = ar(DS)
    W[(C + hh[:, None] * DS + ch[None, 8:20]).reshape(-1)] = subset_signs(NH * 12, VS[16:], 2, g)
    W[(hh[:, None] * DS + ch[None, 20:]).reshape(-1)] = subset_signs(NH * 12, VS[16:], 2, g)
    bq[2 * C:] = RC.stepped_bias(C, "cpu")
    if not skip:
        W[2 * C:] = subset_signs(C, VS, 3, g)
        x_t, y, ln_w, ln_b = unit_rows(R, EPS, g)
        bo = RC.stepped_bias(C, "cpu")
        Wo = RC.sparse_rows(C, C, 8, g, "cpu")
        Wo[VS] = 0.0
        x = torch.zeros(R, C, dtype=torch.float64)
        x[:, VS] = x_t[:, VS] - bo[VS]
        v = x @ W[2 * C:].T + bq[2 * C:]
        o = attention_expected(v, rep, t, B, T)
        xv = x[:, VS].clone()
        x = x_t - (o @ Wo.T + bo)
        assert torch.equal(x[:, VS], xv)
        pe = ri(g, -1, 1, R, C)
        pe[:, VS] = ri(g, 1, 3, R, len(VS)) * (2 * ri(g, 0, 1, R, len(VS)) - 1)
        pe[:, KC] = kcode - x[:, KC]
        pe[:, QC.reshape(-1)] = qcode - x[:, QC.reshape(-1)]
        pre = x_t
    else:
        W[(2 * C + hh[:, None] * DS + ch[None, :16]).reshape(-1), VS[:16].repeat(NH)] = 1.0
        W[(2 * C + hh[:, None] * DS + ch[None, 16:]).reshape(-1)] = subset_signs(NH * 16, VS[16:], 2, g)
        alpha = 2.0 ** ri(g, 0, 2, R)                                               # a of the token (b, j)
        S = (torch.rand(MAXT, C, generator=g).argsort(1) < C // 2).double() * 2 - 1
        assert torch.unique(S, dim=0).shape[0] == MAXT
        x = ri(g, -3, 3, R, C)
        x[:, KC], x[:, QC.reshape(-1)] = kcode, qcode
        x[:, VS[:16]] = 0.0
        x[ar(R), VS[tok]] = alpha / 8
        v = x @ W[2 * C:].T + bq[2 * C:]
        o = attention_expected(v, rep, t, B, T)
        Wo = torch.zeros(C, C, dtype=torch.float64)
        for h in range(NH):
            Wo[:, h * DS:h * DS + MAXT] = S.T
        m = 2.0
        bo = m - Wo @ bq[2 * C:]
        pre = o @ Wo.T + bo
        tt = t[:, 0].reshape(R)                                                     # the row's target (every head's)
        a_row = alpha.view(B, T).gather(1, t[:, 0]).reshape(R, 1)
        assert torch.equal(pre, m + a_row * S[tt]), "eight heads of a / 8 add up to the target row m + a S_t"
        ln_w, ln_b = ln_vectors(g)
        y = S[tt] * ln_w + ln_b
        assert ln_dev(a_row, ln_w, EPS) < 1.7e-4 and 2 <= float(y.abs().min())
        pe = ri(g, -1, 1, R, C)
        pe[:, RESERVED] = 0.0
        pe[:, QC[:, 0]] = -2 * x[:, QC[:, 0]]                                       # pe added to q | k would flip bit 0 of every target
    Wcq = RC.sparse_rows(CI, C, 12, g, "cpu")
    Wcq[:, RESERVED] = 0.0
    bcq = positive_bias(CI) + 30.0
    qp = (y + pe) @ Wcq.T + bcq
    # ---- the conditions
    a_qk = x if skip else x + pe
    q, k, vv = a_qk @ W[:C].T + bq[:C], a_qk @ W[C:2 * C].T + bq[C:2 * C], x @ W[2 * C:].T + bq[2 * C:]
    assert torch.equal(vv, v) and exact16(a_qk[:, RESERVED]) and exact16(x[:, VS]) and exact16(W) and exact16(Wo) and exact16(Wcq)
    assert exact16(q) and exact16(k) and exact16(v) and exact16(o) and exact16(qp) and float(qp.min()) >= 1
    assert bool((x.float().double() == x).all()) and bool((pe.float().double() == pe).all())
    sc = torch.einsum("bihd,bjhd->bhij", q.view(B, T, NH, DS), k.view(B, T, NH, DS))
    hit = rep[:, None, None, :] == t[..., None]
    assert bool((sc[hit] == 0).all()) and bool((sc[~hit] <= -2 * SEL).all()) and 2 * SEL * AC.LOG2E / math.sqrt(DS) >= GAP
    assert bool(((y + pe)[:, FREE].abs() >= 1).all()), "no operand of the query projection is the rounded value of a cancellation"
    if not skip:
        assert bool((x[:, VS] + pe[:, VS] != x[:, VS]).all()), "v from x + pe differs from v from x"
        vb = v.view(B, T, NH, DS)
        assert all(torch.unique(vb[b, :, h], dim=0).shape[0] == T for b in range(B) for h in range(NH)), "no two keys share a V row"
    return dict(kind="self", B=B, T=T, skip=skip, x=x, pe=pe, wqkv=W, bqkv=bq, wo=Wo, bo=bo, ln_w=ln_w, ln_b=ln_b, eps=EPS, wcq=Wcq, bcq=bcq,
                pre=pre, y=y, qp=qp, o=o, t=t, rep=rep, tie=tie)


# ---------------------------------------------------------------------------------------------------------------------------------
# the attention output of the cross attentions: 16-bit rows or synthetic key-split partials
def partials_exact(B, T, S, g):
    """(o [R, CI], part [B NH S T 18]): rowtile_cases.merged_exact's states in the producer's layout
    part[((b * 8 + head) * S + s) * T + row] = (m, l, O[16]), O un-normalised.  Live splits of a row share its maximum and carry
    power-of-two sums (PARTS) whose total is a power of two, O = l * small integers: the merged row is a multiple of 1 / 8.  Empty
    splits are what the producer documents, (-inf, 0, zeros) -- a NaN in an empty split's O WOULD propagate (acc += a * 0): that is the
    producer's contract, not a defect of the consumers.  Dead splits: a finite maximum >= 200 below the row's, l > 0, |O| >= 512."""
    M = B * NH * T
    st = RC.split_states(M, S) if S >= 2 else torch.full((1, M), LIVE)
    live = st == LIVE
    rowmax = ri(g, -6, 6, M) + 0.25 * ri(g, 0, 3, M)
    mx = torch.where(live, rowmax, rowmax - 200.0 - ri(g, 0, 50, S, M))
    mx = torch.where(st == EMPTY, torch.full_like(mx, -math.inf), mx)
    n = live.sum(0)
    rank = (live.long().cumsum(0) - 1 + torch.randint(0, 8, (M,), generator=g)) % n
    total = 2.0 ** ri(g, -2, 3, M)
    sm = RC.PARTS[n[None, :].expand(S, M), rank] * total
    sm = torch.where(live, sm, torch.where(st == DEAD, ri(g, 1, 5, S, M), torch.zeros_like(sm)))
    val = torch.where(live[..., None], ri(g, -3, 3, S, M, DX), (512.0 + 64 * ri(g, 0, 7, S, M, DX)) * (2 * ri(g, 0, 1, S, M, DX) - 1))
    O = torch.where((st == EMPTY)[..., None], torch.zeros_like(val), val * sm[..., None])
    L = (sm * live).sum(0)
    A = pz((O * live[..., None]).sum(0) / L[:, None])
    assert bool((A * 8 == (A * 8).round()).all()) and exact16(A) and bool((torch.log2(L) == torch.log2(L).round()).all())
    assert bool((O.float().double() == O).all()) and bool((mx[st == DEAD] <= rowmax.expand(S, M)[st == DEAD] - 200).all())
    assert bool((sm[st == DEAD] > 0).all()) and bool((sm[st == EMPTY] == 0).all()) and bool((O[st == DEAD].abs() >= 512).all())
    o = A.view(B, NH, T, DX).permute(0, 2, 1, 3).reshape(B * T, CI)
    part = torch.cat([mx[..., None], sm[..., None], O], -1).view(S, B * NH, T, 18).permute(1, 0, 2, 3).contiguous()
    return o, part.reshape(-1, 18), st


def attention_rows(B, T, splits, g):
    if splits == 0:
        return ri(g, -3, 3, B * T, CI), None
    o, part, _ = partials_exact(B, T, splits, g)
    return o, part


def merge_partials(part, B, T, S):
    """float64 merge of partials [B NH S T, 18] -> rows [B T, CI] (rowtile_cases.merge_reference's formula, un-normalised O)"""
    p = part.double().view(B, NH, S, T, 18)
    m, l, O = p[..., 0], p[..., 1], p[..., 2:]
    w = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp2(m - m.amax(2, keepdim=True)))
    o = (O * w[..., None]).sum(2) / (l * w).sum(2)[..., None]
    return o.permute(0, 2, 1, 3).reshape(B * T, CI)


# ---------------------------------------------------------------------------------------------------------------------------------
# dec_tail, dec_mlp + dec_kv
def tail_exact(B, T, splits):
    g = gen(42, B, T, splits)
    R = B * T
    x_t, y, ln_w, ln_b = RC.target_rows(R, C, EPS, g, "cpu")
    o, part = attention_rows(B, T, splits, g)
    Wo, bo = RC.sparse_rows(C, CI, 8, g, "cpu"), RC.stepped_bias(C, "cpu")
    x = x_t - (o @ Wo.T + bo)
    assert exact16(o) and exact16(Wo) and bool((x.float().double() == x).all())
    return dict(kind="tail", B=B, T=T, splits=splits, o=o, part=part, x=x, wo=Wo, bo=bo, ln_w=ln_w, ln_b=ln_b, eps=EPS, pre=x_t, y=y)


A3 = 4.0                                   # a of every norm3 row
EPS3 = 1e-6                                # norm3's eps in the exact pass: norm2 with it moves its a = 1 / 4 rows by 1.4e-4, 300 bounds


def mlp_exact(B, T, last, splits):
    g = gen(43, B, T, last, splits)
    R = B * T
    x2t, z, g2, bl2 = RC.target_rows(R, C, EPS, g, "cpu")                           # z: norm2's integers s g + b
    s2 = (z - bl2) / g2
    o, part = attention_rows(B, T, splits, g)
    Wo, bo = RC.sparse_rows(C, CI, 8, g, "cpu"), RC.stepped_bias(C, "cpu")
    x = x2t - (o @ Wo.T + bo)
    # fc1 / fc2: L = a3 P G^-1 - I through 512 entries (n, k, val) of four hidden units each
    ar = torch.arange
    pi = torch.randperm(C, generator=g)                                             # output column pi[k] takes a3 s2[:, k]
    n_idx, k_idx = torch.cat([pi, ar(C)]), torch.cat([ar(C), ar(C)])
    val = torch.cat([A3 / g2, -torch.ones(C, dtype=torch.float64)])
    rr = RC.sparse_rows(2 * C, C, 11, g, "cpu")
    rr[ar(2 * C), k_idx] = 0.0
    ek = torch.nn.functional.one_hot(k_idx, C).double()
    place = torch.randperm(HID, generator=g).view(4, 2 * C)                         # hidden units of (A, -A, B, -B)
    u = ar(HID)
    step = ((u + u // 32 + u // SLICE) % 4).double() - 1.0                          # steps with the unit, its 32-block and its slice
    W1, b1, W2 = torch.zeros(HID, C, dtype=torch.float64), torch.zeros(HID, dtype=torch.float64), torch.zeros(C, HID, dtype=torch.float64)
    for j, (row, sgn) in enumerate(((ek + rr, 1.0), (ek + rr, -1.0), (ek - rr, 1.0), (ek - rr, -1.0))):
        W1[place[j]] = sgn * row
        b1[place[j]] = step[place[j]] if sgn > 0 else -step[place[j - 1]]
        W2[n_idx, place[j]] = sgn * val / 2
    pre1 = z @ W1.T + b1
    hid = pre1.clamp(min=0)
    slabs = pz(torch.stack([hid[:, i * SLICE:(i + 1) * SLICE] @ W2[:, i * SLICE:(i + 1) * SLICE].T for i in range(NSLICE)]))
    m3 = float(ri(g, -3, 3, 1))
    s3 = torch.zeros_like(s2)
    s3[:, pi] = s2
    cb = torch.zeros(C, dtype=torch.float64).index_add_(0, n_idx, val / 2 * (step[place[0]] + step[place[2]]))
    shift = torch.zeros(C, dtype=torch.float64)
    shift[pi] = A3 * bl2 / g2
    b2 = m3 - cb - shift
    pre3 = slabs.sum(0) + b2 + z
    assert torch.equal(pre3, m3 + A3 * s3), "fc2 + b2 + norm2's integers are the target row m3 + a3 P s"
    g3, bl3 = ln_vectors(g)
    y3 = s3 * g3 + bl3
    pe = ri(g, -1, 1, R, C)
    Wkv, bkv = RC.sparse_rows(C, C, 8, g, "cpu"), positive_bias(C)
    kv = torch.cat([(y3 + pe) @ Wkv[:CI].T, y3 @ Wkv[CI:].T], 1) + bkv
    Wfq, bfq = RC.sparse_rows(CI, C, 8, g, "cpu"), positive_bias(CI) + 1.0
    qpf = (y3 + pe) @ Wfq.T + bfq
    # ---- the conditions
    assert exact16(o) and exact16(Wo) and exact16(W1) and exact16(W2) and exact16(Wkv) and exact16(Wfq) and exact16(hid) and exact16(z)
    assert bool((x.float().double() == x).all()) and bool((slabs.float().double() == slabs).all()) and bool((b2.float().double() == b2).all())
    assert float(pre1.min()) <= -8 and float(pre1.max()) >= 8 and float(pre1.abs().max()) <= 87, "integers of both signs: ReLU decides"
    assert torch.unique(slabs.reshape(NSLICE, -1), dim=0).shape[0] == NSLICE, "every slice's fc2 contribution differs from every other's"
    assert bool(((hid > 0).view(R, NSLICE, SLICE).any(2)).all()), "every slice has a live unit in every row"
    # dec_kv's residual is norm2's fp32 output z + delta: delta <= the LayerNorm's distance to its integer + its fp32 error (ln_bound)
    delta = ln_dev(torch.tensor(0.25), g2, EPS) + float(ln_bound_exact(x2t, g2, bl2, EPS)[1].max())
    dev3 = 3 * float(g3.abs().max()) * delta / A3 + ln_dev(A3, g3, EPS3) + float(ln_bound(pre3, g3, bl3, EPS3)[1].max())
    assert dev3 < 2.0 ** -11, "norm3 stays inside half a 16-bit ulp (fp16 at 1 .. 2, the smallest |y3 + pe|) of its integers"
    assert bool(((y3 + pe).abs() >= 1).all()) and exact16(kv) and exact16(qpf) and float(kv.min()) >= 1 and float(qpf.min()) >= 1
    return dict(kind="mlp", B=B, T=T, last=last, splits=splits, o=o, part=part, x=x, wo=Wo, bo=bo, ln2_w=g2, ln2_b=bl2, eps2=EPS, w1=W1, b1=b1,
                w2=W2, b2=b2, ln3_w=g3, ln3_b=bl3, eps3=EPS3, pe=pe, wkv=Wkv, bkv=bkv, wfq=Wfq if last else None, bfq=bfq if last else None,
                pre2=x2t, z=z, slabs=slabs, pre3=pre3, y3=y3, kv=kv, qpf=qpf if last else None, delta=delta)


# ---------------------------------------------------------------------------------------------------------------------------------
# the key-split producer
LQ = (1, 7, 16, 32)
# (Lk, splits): one key; seven empty splits; Lk = 9 in 8 splits of 2 (three empty); a ragged second split; 13 keys a split (one per wave,
# three waves empty); 512 / 513 keys: the step from <1> to <2>; 1025: <4>; 2049 and 4096: <8>; 4096 in 2 / 4 / 8 splits: <8>, <4>, <2>;
# 4095 in 3 splits of 1365: <4>
PRODUCER = [(1, 1), (1, 8), (9, 8), (33, 2), (100, 8), (512, 1), (513, 1), (1025, 1), (2049, 1), (4096, 1), (4096, 2), (4096, 4), (4096, 8),
            (4095, 3)]
PRODUCER_CASES = [(Lq, Lk, S) for Lk, S in PRODUCER for Lq in LQ]


def producer_batch(Lq):
    return 2 if Lq <= MAXT else 1          # B Lq <= 32: the partials go on into dec_tail / dec_mlp


def part_maxs(Lk, S):
    """the launcher's choice: steps = 32-key steps of a wave = ceil(ceil(ceil(Lk / S) / 16) / 32), rounded up to 1, 2, 4 or 8"""
    steps = cdiv(cdiv(cdiv(Lk, S), 16), 32)
    return 1 if steps <= 1 else 2 if steps <= 2 else 4 if steps <= 4 else 8


def split_ranges(Lk, S):
    per = cdiv(Lk, S)
    return [(min(s * per, Lk), min(Lk, (s + 1) * per)) for s in range(S)]


def producer_targets(Lk, S):
    """the last key overall, key 0, then per split its first and last key and the first key of its last wave / last key of its first"""
    out = [Lk - 1, 0]
    for lo, hi in split_ranges(Lk, S):
        if hi > lo:
            pw = cdiv(hi - lo, 16)
            out += [lo, hi - 1, lo + (hi - lo - 1) // pw * pw, min(lo + pw - 1, hi - 1), min(lo + 32, hi - 1)]
    seen = []
    for t in out:
        if t not in seen:
            seen.append(t)
    return seen


def producer_sel(Lq, Lk, S):
    """selection + ties on the producer: (q, k, v [B, NH, L, 16], expected partials [B NH S Lq, 18] with NaN where only a bound holds,
    live [B NH S Lq] 0 empty / 1 other live split / 2 the target's, expected merged rows [B Lq, CI])"""
    B = producer_batch(Lq)
    nb = max(1, (Lk - 1).bit_length())
    spec = producer_targets(Lk, S)
    n = torch.arange(B)[:, None] * NH + torch.arange(NH)[None, :]
    i = torch.arange(Lq)
    nn = n[:, :, None]
    t = torch.where(i[None, None, :] < len(spec), torch.tensor(spec)[(i[None, None, :] + nn) % len(spec)], (37 * i[None, None, :] + 5 + 11 * nn) % Lk)
    rep = torch.arange(Lk)
    rng = split_ranges(Lk, S)
    pairs = ([(1, Lk - 1)] if Lk >= 3 else []) + ([(4, 9)] if Lk > 10 else [])       # across the splits; inside the first wave
    for a, b in pairs:
        rep[b] = a
    t = rep[t]
    k = torch.zeros(B, NH, Lk, DX, dtype=torch.float64)
    q = torch.zeros(B, NH, Lq, DX, dtype=torch.float64)
    k[..., :nb], q[..., :nb] = AC.code(rep, nb), SEL * AC.code(t, nb)
    k[..., 14:] = 1.0
    q[..., 14], q[..., 15] = -SEL * min(nb, 8), -SEL * (nb - min(nb, 8))
    v = AC.v_pattern(torch.arange(Lk)[None, None, :] + 13 * nn, torch.arange(DX), True)
    v = torch.where(v >= 0, v + 1, v)                                              # no zero: 1 .. 16 and -15 .. -1
    match = (rep[None, None, None, :] == t[..., None]).double()                    # [B, NH, Lq, Lk]
    sc = q @ k.transpose(2, 3)
    assert exact16(q) and exact16(k) and exact16(v) and bool((sc[match > 0] == 0).all()) and bool((sc[match == 0] <= -2 * SEL).all())
    assert 2 * SEL * AC.LOG2E / math.sqrt(DX) >= GAP
    exp = torch.full((B, NH, S, Lq, 18), math.nan, dtype=torch.float64)
    state = torch.zeros(B, NH, S, Lq, dtype=torch.long)
    for s, (lo, hi) in enumerate(rng):
        if hi <= lo:
            exp[:, :, s, :, 0], exp[:, :, s, :, 1:] = -math.inf, 0.0
            continue
        cnt = match[..., lo:hi].sum(-1)
        osum = match[..., lo:hi] @ v[:, :, lo:hi]
        has = cnt > 0
        state[:, :, s] = 1 + has.long()
        exp[:, :, s, :, 0] = torch.where(has, torch.zeros_like(cnt), torch.full_like(cnt, math.nan))
        exp[:, :, s, :, 1] = torch.where(has, cnt, torch.full_like(cnt, math.nan))
        exp[:, :, s, :, 2:] = torch.where(has[..., None], pz(osum), torch.full_like(osum, math.nan))
    o = pz((match @ v) / match.sum(-1, keepdim=True))
    assert exact16(o) and bool((state == 2).any(2).all())
    return dict(B=B, Lq=Lq, Lk=Lk, S=S, q=q, k=k, v=v, exp=exp.reshape(-1, 18), state=state.reshape(-1), o=o.permute(0, 2, 1, 3).reshape(B * Lq, CI),
                pairs=pairs, t=t)


def producer_rand(Lq, Lk, S, op16):
    """randn operands rounded to the operand type; float64 reference, bounds of the merged output and of m + log2 l"""
    B = producer_batch(Lq)
    g = gen(44, Lq, Lk, S)
    q = r16(torch.randn(B, NH, Lq, DX, generator=g) * 2.0, op16).double()
    k = r16(torch.randn(B, NH, Lk, DX, generator=g), op16).double()
    v = r16(torch.randn(B, NH, Lk, DX, generator=g), op16).double()
    if Lk >= 40 and Lq >= 6:
        k[0, 0, Lk - 3] = r16(q[0, 0, 5] * 0.75, op16)                             # one key far above the rest in the last wave
    c = AC.LOG2E / math.sqrt(DX)
    ref, A, smax, lse = AC.reference(q, k, v, c)
    fp16 = op16 == torch.float16
    bound = AC.attention_error_bound(ref, A, smax, Lk, DX, c, fp16=fp16, p16=True)
    return dict(B=B, Lq=Lq, Lk=Lk, S=S, q=q, k=k, v=v, ref=ref, bound=bound, lse=lse, lse_bound=AC.lse_bound(lse, smax, DX, c, fp16, False))


# ---------------------------------------------------------------------------------------------------------------------------------
# bounded pass: seeded randn operands as tests/test_decoder_tokens_gpu.py builds them, float64 references stage by stage
def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


_BW = {}


def bounded_weights(op16, lowvar=False):
    """one set of block weights (float64 holders of 16-bit matrices and fp32 vectors), LayerNorm vectors away from (1, 0).  lowvar: the
    out-projections, fc2 and their biases scaled so that, with bounded()'s lowvar rows, every pre-norm row has a standard deviation
    of about 0.03 around 1 -- a variance of the size of eps = 1e-3"""
    key = (op16, lowvar)
    if key not in _BW:
        sc = 0.03 if lowvar else 1.0
        mat = lambda n, k, seed, s=1.0: r16(rnd(n, k, seed=seed, scale=s * k ** -0.5), op16).double()
        vec = lambda n, seed, scale=0.5, base=0.0: (base + rnd(n, seed=seed, scale=scale)).float().double()
        _BW[key] = dict(wqkv=mat(3 * C, C, 1), bqkv=vec(3 * C, 2), wso=mat(C, C, 3, sc), bso=vec(C, 4, 0.5 * sc, 1.0 if lowvar else 0.0),
                        n1w=vec(C, 5, 0.1, 1.0), n1b=vec(C, 6, 0.1), wcq=mat(CI, C, 7), bcq=vec(CI, 8), wco=mat(C, CI, 9, sc),
                        bco=vec(C, 10, 0.5 * sc, 1.0 if lowvar else 0.0), n2w=vec(C, 11, 0.1 * sc, sc), n2b=vec(C, 12, 0.1 * sc, 1.0 if lowvar else 0.0),
                        w1=mat(HID, C, 13), b1=vec(HID, 14), w2=mat(C, HID, 15, sc), b2=vec(C, 16, 0.5 * sc), n3w=vec(C, 17, 0.1, 1.0),
                        n3b=vec(C, 18, 0.1), wkv=mat(C, C, 19), bkv=vec(C, 20), wfq=mat(CI, C, 21), bfq=vec(CI, 22))
    return _BW[key]


EPS_LOW = dict(eps1=1e-3, eps2=1e-3, eps3=1e-6)


def bounded(B, T, op16, lowvar=False):
    """the inputs of the three entries: x, pe fp32 rows, o 16-bit rows.  lowvar: x = 0.03 randn (every residual row then has std 0.03)"""
    R = B * T
    W = bounded_weights(op16, lowvar)
    x = rnd(R, C, seed=30 + R, scale=0.03 if lowvar else 1.0).double()
    pe = rnd(R, C, seed=31 + R).double()
    o = r16(rnd(R, CI, seed=32 + R), op16).double()
    eps = EPS_LOW if lowvar else dict(eps1=EPS, eps2=EPS, eps3=EPS)
    return dict(B=B, T=T, x=x, pe=pe, o=o, W=W, lowvar=lowvar, **eps)


def bounded_self(B, T, skip, op16, lowvar=False):
    """the bounded pass's dec_self call in the exact pass's form"""
    b = bounded(B, T, op16, lowvar)
    W = b["W"]
    return dict(kind="self", B=B, T=T, skip=skip, x=b["x"], pe=b["pe"], wqkv=W["wqkv"], bqkv=W["bqkv"], wo=W["wso"], bo=W["bso"], ln_w=W["n1w"],
                ln_b=W["n1b"], eps=b["eps1"], eps1=b["eps1"], wcq=W["wcq"], bcq=W["bcq"], W=W)


def bounded_tail(B, T, op16, lowvar=False, part=None, splits=0):
    b = bounded(B, T, op16, lowvar)
    W = b["W"]
    return dict(kind="tail", B=B, T=T, splits=splits, o=b["o"], part=part, x=b["x"], wo=W["wco"], bo=W["bco"], ln_w=W["n2w"], ln_b=W["n2b"],
                eps=b["eps2"], W=W)


def bounded_mlp(B, T, last, op16, lowvar=False, part=None, splits=0):
    b = bounded(B, T, op16, lowvar)
    W = b["W"]
    return dict(kind="mlp", B=B, T=T, last=last, splits=splits, o=b["o"], part=part, x=b["x"], wo=W["wco"], bo=W["bco"], ln2_w=W["n2w"],
                ln2_b=W["n2b"], eps2=b["eps2"], w1=W["w1"], b1=W["b1"], w2=W["w2"], b2=W["b2"], ln3_w=W["n3w"], ln3_b=W["n3b"], eps3=b["eps3"],
                pe=b["pe"], wkv=W["wkv"], bkv=W["bkv"], wfq=W["wfq"] if last else None, bfq=W["bfq"] if last else None, W=W)


def error_bound(*a, **k):
    """error_bound of tests/test_gemm_variants_gpu.py (that module imports the oracle package from the repository root)"""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    from test_gemm_variants_gpu import error_bound as eb
    return eb(*a, **k)


def gemm_ref(a, w, b, fp16, out16=False, da=None, extra=None):
    """(ref, bound) of a w^T + b (+ extra, an fp32 residual) for 16-bit operands held in float64: error_bound of
    tests/test_gemm_variants_gpu.py, widened by da |w|^T where the kernel's operand may differ from `a` by da"""
    pre = a @ w.T + b
    ref = pre if extra is None else pre + extra
    e = error_bound(a.abs() @ w.abs().T, a.shape[1], pre, ref, fp16=fp16)
    if da is not None:
        e = e + da @ w.abs().T
    return ref, (store16(ref, e, fp16) if out16 else e)


def op_of(rows32, addend32, op16):
    """the kernels' operand image: f2op(fp32 sum), the sum taken in fp32 as they take it"""
    t = rows32.float() if addend32 is None else rows32.float() + addend32.float()
    return t.to(op16).double()


def self_reference(E, op16, eps=None):
    """(xout ref, bound) of dec_self from the operand-rounded inputs: q | k | v rounded to 16 bits, float64 attention, its output NOT
    rounded (the attention bound covers the kernel's 16-bit output against it), out-projection, residual, LayerNorm.  The attention bound
    is attention_error_bound with fused_cases.attn_reference's widening for q, k and v within one 16-bit ulp of the reference's."""
    W, B, T, skip = E["W"], E["B"], E["T"], E.get("skip", False)
    fp16 = op16 == torch.float16
    a_qk = op_of(E["x"], None if skip else E["pe"], op16)
    a_v = op_of(E["x"], None, op16)
    qkv = r16(torch.cat([a_qk @ W["wqkv"][:2 * C].T, a_v @ W["wqkv"][2 * C:].T], 1) + W["bqkv"], op16)
    q, k, v = (qkv[:, i * C:(i + 1) * C].view(B, T, NH, DS).permute(0, 2, 1, 3) for i in range(3))
    c = AC.LOG2E / math.sqrt(DS)
    ref, A, smax, _ = AC.reference(q, k, v, c)
    h = AC.u16(fp16)
    ds = AC.score_error(smax, DS, c, fp16, False) + c * smax * (4 * h + 4 * h * h)
    e = torch.expm1(2 * math.log(2.0) * ds) * A + (T + 8) * AC.U * A + 2 * h * A
    e = e + h * (ref.abs() + e) + 2.0 ** -25
    back = lambda t_: t_.permute(0, 2, 1, 3).reshape(B * T, C)
    o, do = back(ref), back(e)
    pre, dpre = gemm_ref(o, W["wso"], W["bso"], fp16, da=do, extra=None if skip else E["x"])
    return ln_bound(pre, W["n1w"], W["n1b"], E["eps1"] if eps is None else eps, dpre)


def proj_reference(rows32, pe, w, b, op16, split=None):
    """(ref, bound) of a 16-bit projection behind a LayerNorm from the kernel's OWN fp32 rows: columns < split read f2op(rows + pe), the
    others f2op(rows)"""
    fp16 = op16 == torch.float16
    a_pe = op_of(rows32, pe, op16)
    if split is None:
        return gemm_ref(a_pe, w, b, fp16, out16=True)
    r1, b1 = gemm_ref(a_pe, w[:split], b[:split], fp16, out16=True)
    r2, b2 = gemm_ref(op_of(rows32, None, op16), w[split:], b[split:], fp16, out16=True)
    return torch.cat([r1, r2], 1), torch.cat([b1, b2], 1)


def rows_reference(o, do, x, w, b, ln_w, ln_b, eps, op16):
    """(ref, bound) of out-projection + residual + LayerNorm (dec_tail, norm2 of dec_mlp); do: what the kernel's 16-bit rows may differ
    from o by (merged partials: one 16-bit ulp)"""
    pre, dpre = gemm_ref(o, w, b, op16 == torch.float16, da=do, extra=x)
    return ln_bound(pre, ln_w, ln_b, eps, dpre)


def slabs_reference(mid32, W, op16):
    """(ref [16, R, C], bound) of the fc2 workspace from the kernel's OWN norm2 rows: hidden map rounded to 16 bits (the kernel's may be
    one 16-bit ulp off where its fp32 sum and the float64 sum round apart: ulp16 |w2| per unit, and what ReLU passes of fc1's fp32 error)"""
    fp16 = op16 == torch.float16
    a = op_of(mid32, None, op16)
    pre1, e1 = gemm_ref(a, W["w1"], W["b1"], fp16)
    hid = r16(pre1.clamp(min=0), op16)
    dh = torch.where(pre1 > -e1, RC.ulp16(hid, op16) + e1, torch.zeros_like(e1))
    refs, bounds = [], []
    for i in range(NSLICE):
        sl = slice(i * SLICE, (i + 1) * SLICE)
        r, e = gemm_ref(hid[:, sl], W["w2"][:, sl], 0.0, fp16, da=dh[:, sl])
        refs.append(r)
        bounds.append(e)
    return torch.stack(refs), torch.stack(bounds)


def norm3_reference(slabs32, mid32, W, eps3):
    """(ref, bound) of norm3 from the kernel's OWN workspace slabs and norm2 rows: 17 fp32 additions in front of the LayerNorm"""
    terms = torch.cat([slabs32.double(), W["b2"].expand_as(mid32)[None].double(), mid32.double()[None]])
    pre = terms.sum(0)
    return ln_bound(pre, W["n3w"], W["n3b"], eps3, (NSLICE + 1) * U * terms.abs().sum(0))


def attn_rows64(E, op16):
    """(o, do): the cross attention's 16-bit rows as the consumers see them, and what theirs may differ by: nothing for 16-bit rows, one
    16-bit ulp for partials (the kernel rounds an fp32 merge, the reference a float64 one)"""
    if E["part"] is None:
        return E["o"], None
    o = r16(merge_partials(E["part"], E["B"], E["T"], E["splits"]), op16)
    return o, RC.ulp16(o, op16)


def bounded_checks(E, got, op16, swap=False, no_eps=False):
    """[(what, got, ref, bound)] of a bounded-pass case from the outputs `got` {name: tensor} of the kernels (or of restate): every
    stage against float64 from the operand-rounded inputs or from the kernel's own fp32 rows in front of it.  swap / no_eps: the
    references a kernel with eps2 and eps3 exchanged / without eps would match."""
    ep = lambda e: 0.0 if no_eps else e
    W = E["W"]
    if E["kind"] == "self":
        ref, b = self_reference(E, op16, ep(E["eps1"]))
        r2, b2 = proj_reference(got["queries_out"], E["pe"], W["wcq"], W["bcq"], op16)
        return [("norm1 rows", got["queries_out"], ref, b), ("tokens -> image query projection", got["qp"], r2, b2)]
    o, do = attn_rows64(E, op16)
    if E["kind"] == "tail":
        ref, b = rows_reference(o, do, E["x"], E["wo"], E["bo"], E["ln_w"], E["ln_b"], ep(E["eps"]), op16)
        return [("final norm rows", got["queries_out"], ref, b)]
    e2, e3 = (E["eps3"], E["eps2"]) if swap else (E["eps2"], E["eps3"])
    out = [("norm2 rows",) + (got["queries_mid"],) + rows_reference(o, do, E["x"], E["wo"], E["bo"], E["ln2_w"], E["ln2_b"], ep(e2), op16)]
    out.append(("fc2 workspace", got["ws"]) + slabs_reference(got["queries_mid"], W, op16))
    out.append(("norm3 rows", got["queries_out"]) + norm3_reference(got["ws"], got["queries_mid"], W, ep(e3)))
    out.append(("image -> token k | v", got["kv"]) + proj_reference(got["queries_out"], E["pe"], W["wkv"], W["bkv"], op16, split=CI))
    if E["last"]:
        out.append(("final attention's query projection", got["qp_final"]) + proj_reference(got["queries_out"], E["pe"], W["wfq"], W["bfq"], op16))
    return out


def restated_outputs(E, op16, defect=None):
    """restate()'s stores as full tensors {name: [R, N]}, "ws" as [16, R, C] -- what the GPU file reads back from a call"""
    got, R = restate(E, op16, defect), E["B"] * E["T"]
    out = {}
    for name, val in got.items():
        if name == "ws":
            out[name] = val[:NSLICE * R * C].view(NSLICE, R, C)
            continue
        rows, vals = val
        keep = rows < R
        full = torch.zeros(R, vals.shape[1], dtype=vals.dtype)
        full[rows[keep]] = vals[keep]
        out[name] = full.to(op16) if name in ("qp", "kv", "qp_final") else full
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the four kernels restated in fp32, with simulated defects
DEFECTS = ["v reads x + pe", "k and v halves of dec_kv exchange their operand image", "the final q projection reads the image without pe",
           "a residual is added under skip_first_layer_pe", "pe is added to q | k under skip_first_layer_pe",
           "the dead-lane mask of the softmax is dropped", "the probability broadcast drops lane & 48", "the head offset is one head off for v",
           "+ 4 h is dropped from the row map", "the bias is one unit off (bq[j] of the wrong unit)", "a hidden slice uses the previous slice's b1",
           "a hidden slice uses the previous slice's w2 columns", "the workspace slab stride is T instead of R", "dec_kv sums 15 slabs",
           "the ws store's row < T test is dropped", "store_rows16 writes 16 rows", "the s >= splits mask is dropped",
           "an empty split is given weight 1", "a dead split is not given weight 0", "head = c / D is computed with D = 32",
           "eps2 and eps3 are swapped", "eps is ignored"]
D = {i + 1: d for i, d in enumerate(DEFECTS)}


def _f(t):
    return None if t is None else t.to(F32)


def tok_gemm(a, w, kp, defect=None):
    """TokGemm on the operand images a [B, 16, K] (rows >= T zero): the k range in four parts added in order (KP == 1: four quarter sums in
    registers; KP == 4: four partials in LDS, added by the reader); the accumulator's row (e & 3) + 8 (e >> 2) + 4 h"""
    K = a.shape[-1]
    out = 0
    for p in range(4):
        sl = slice(p * K // 4, (p + 1) * K // 4)
        part = a[..., sl] @ w[:, sl].T
        out = part if p == 0 else out + part
    if defect == D[9]:
        # lanes of half h = 1 write their rows (true rows 4 .. 7, 12 .. 15) over rows 0 .. 3, 8 .. 11; the rows of half 1 are never written
        res = torch.zeros_like(out)
        res[:, [0, 1, 2, 3, 8, 9, 10, 11]] = out[:, [4, 5, 6, 7, 12, 13, 14, 15]]
        return res
    return out


def _image(rows, B, T):
    """[R, K] -> operand images [B, 16, K], rows >= T zero"""
    img = torch.zeros(B, MAXT, rows.shape[1], dtype=F32)
    img[:, :T] = rows.view(B, T, -1)
    return img


def _ln32(v, w, b, eps):
    """sum_res_ln_rows' statistics in fp32: 4 values per lane, then the wave sum"""
    n = v.shape[-1]
    lane = v.reshape(*v.shape[:-1], n // 4, 4)
    mean = ((lane[..., 0] + lane[..., 1] + lane[..., 2] + lane[..., 3]).sum(-1, keepdim=True)) / n
    d = v - mean
    dl = d.reshape(*v.shape[:-1], n // 4, 4)
    var = ((dl[..., 0] * dl[..., 0] + dl[..., 1] * dl[..., 1] + dl[..., 2] * dl[..., 2] + dl[..., 3] * dl[..., 3]).sum(-1, keepdim=True)) / n
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=F32))
    return d * rstd * w + b


def _eps(e, defect):
    return 0.0 if defect == D[22] else e


def _store(vals, B, T, nrows):
    """rows an image's workgroup stores: (row indices into the [R, N] output, values); nrows = T, or 16 for a store without its limit"""
    b = torch.arange(B)[:, None]
    r = torch.arange(nrows)[None, :]
    return (b * T + r).reshape(-1), vals[:, :nrows].reshape(B * nrows, -1)


def restate_self(E, op16, defect=None, order=0):
    """dec_self_kernel: {name: (rows, values)} of queries_out (fp32) and qp (16-bit)"""
    B, T, skip = E["B"], E["T"], E["skip"]
    x, pe = _f(E["x"]), _f(E["pe"])
    W, bq = _f(E["wqkv"]), _f(E["bqkv"])
    add_pe = (not skip) or defect == D[5]
    a_qk = _image(r16(x + pe if add_pe else x, op16), B, T)
    a_v = _image(r16(x, op16), B, T)
    if defect == D[1]:
        a_v = a_qk
    bias = bq.roll(-C) if defect == D[10] else bq
    qkv = torch.cat([tok_gemm(a_qk, W[:2 * C], 1, defect), tok_gemm(a_v, W[2 * C:], 1, defect)], -1) + bias
    qkv = r16(qkv, op16)
    scale = torch.tensor((1.0 / math.sqrt(DS)), dtype=F32) * torch.tensor(1.4426950408889634, dtype=F32)
    q = qkv[..., :C].view(B, MAXT, NH, DS)[:, :T]                                   # [B, T, NH, D]
    k = qkv[..., C:2 * C].view(B, MAXT, NH, DS)
    v = qkv[..., 2 * C:].view(B, MAXT, NH, DS)
    if defect == D[8]:
        v = v.roll(-1, 2)
    l16 = torch.arange(16)
    live = l16 < T
    krow = torch.where(live, l16, torch.zeros_like(l16))
    kk = k[:, krow]                                                                 # [B, 16 lanes, NH, D]
    s = torch.zeros(B, T, NH, 16, dtype=F32)
    dorder = torch.arange(DS) if order == 0 else torch.arange(DS).flip(0)
    for d in dorder.tolist():
        s = s + ((q[..., d] * scale)[..., None]) * kk[..., d].permute(0, 2, 1)[:, None]
    masked = live if defect != D[6] else torch.ones(16, dtype=torch.bool)
    m = torch.where(masked, s, torch.full_like(s, -math.inf)).amax(-1, keepdim=True)
    pk = torch.where(masked, torch.exp2(s - m), torch.zeros_like(s))
    l = pk.sum(-1, keepdim=True)
    pw = pk
    if defect == D[7]:
        pw = pk[:, :, (torch.arange(NH) // 4) * 4]                                  # the wave's first 16-lane group: head & ~3 of the same query
    o = torch.zeros(B, T, NH, DS, dtype=F32)
    for key in (range(T) if order == 0 else reversed(range(T))):
        o = o + pw[..., key, None] * v[:, key][:, None]
    o16 = r16(o * (1.0 / l), op16)
    a_o = _image(o16.reshape(B * T, C), B, T)
    pre = tok_gemm(a_o, _f(E["wo"]), 1, defect) + _f(E["bo"])
    if (not skip) or defect == D[4]:
        pre = pre + _image(x, B, T)
    y = _ln32(pre, _f(E["ln_w"]), _f(E["ln_b"]), _eps(E["eps"], defect))
    a = r16(y + _image(pe, B, T), op16)
    a[:, T:] = 0
    qp = r16(tok_gemm(a, _f(E["wcq"]), 4, defect) + _f(E["bcq"]), op16)
    return {"queries_out": _store(y, B, T, T), "qp": _store(qp, B, T, MAXT if defect == D[16] else T)}


def load_attn_rows(E, op16, defect=None):
    """the operand image of the cross attention's output: the 16-bit rows, or the partials merged in split order with clamped loads"""
    B, T = E["B"], E["T"]
    if E["part"] is None:
        return _image(r16(_f(E["o"]), op16), B, T)
    S = E["splits"]
    Dh = 32 if defect == D[20] else DX                    # (D = 32: channels 16 .. 31 read past the 18 floats, into the next row's record)
    c = torch.arange(CI)
    head, d = c // Dh, c % Dh
    flat = torch.cat([_f(E["part"]).reshape(-1), torch.zeros(64, dtype=F32)])        # (room for the reads of D = 32 behind the last record)
    M = torch.full((B, T, CI), -math.inf, dtype=F32)
    ms, ls, as_ = [], [], []
    for s in range(8):
        sc = min(s, S - 1)
        b_, r_ = torch.arange(B)[:, None, None], torch.arange(T)[None, :, None]
        base = ((((b_ * NH + head[None, None, :]) * S) + sc) * T + r_) * 18
        m, l, a = flat[base], flat[base + 1], flat[base + 2 + d[None, None, :]]
        if s >= S and defect != D[17]:
            m = torch.full_like(m, -math.inf)
        ms.append(m), ls.append(l), as_.append(a)
        M = torch.maximum(M, m)
    L, acc = torch.zeros_like(M), torch.zeros_like(M)
    for m, l, a in zip(ms, ls, as_):
        w = torch.exp2(m - M)
        if defect == D[19]:
            w = torch.where(torch.isinf(m), w, torch.ones_like(w))
        w = torch.where(torch.isinf(m), torch.full_like(w, 1.0 if defect == D[18] else 0.0), w)
        L, acc = L + l * w, acc + a * w
    return _image(r16(acc / L, op16).reshape(B * T, CI), B, T)


def restate_tail(E, op16, defect=None):
    B, T = E["B"], E["T"]
    a_o = load_attn_rows(E, op16, defect)
    pre = tok_gemm(a_o, _f(E["wo"]), 1, defect) + _f(E["bo"]) + _image(_f(E["x"]), B, T)
    y = _ln32(pre, _f(E["ln_w"]), _f(E["ln_b"]), _eps(E["eps"], defect))
    return {"queries_out": _store(y, B, T, T)}


WS_TAIL = 4096                                            # floats behind the workspace the restatement and the GPU file watch


def restate_mlp(E, op16, defect=None):
    """dec_mlp_kernel + dec_kv_kernel: {name: (rows, values)} of queries_mid, queries_out, kv, qp_final and "ws": the workspace as the
    call leaves it (NaN where nothing was stored), WS_TAIL floats longer than msam2_decoder_tokens_workspace_bytes"""
    B, T = E["B"], E["T"]
    R = B * T
    eps2, eps3 = (E["eps3"], E["eps2"]) if defect == D[21] else (E["eps2"], E["eps3"])
    a_o = load_attn_rows(E, op16, defect)
    pre2 = tok_gemm(a_o, _f(E["wo"]), 1, defect) + _f(E["bo"]) + _image(_f(E["x"]), B, T)
    y2 = _ln32(pre2, _f(E["ln2_w"]), _f(E["ln2_b"]), _eps(eps2, defect))
    a_y = r16(y2, op16)
    a_y[:, T:] = 0
    W1, b1, W2 = _f(E["w1"]), _f(E["b1"]), _f(E["w2"])
    ws = torch.full((NSLICE * R * C + WS_TAIL,), math.nan, dtype=F32)
    stride_w = T if defect == D[13] else R
    nst = MAXT if defect == D[15] else T
    for i in range(NSLICE):
        ib = i - 1 if defect == D[11] and i > 0 else i
        iw = i - 1 if defect == D[12] and i > 0 else i
        hid = r16((tok_gemm(a_y, W1[i * SLICE:(i + 1) * SLICE], 4, defect) + b1[ib * SLICE:(ib + 1) * SLICE]).clamp(min=0), op16)
        hid[:, T:] = 0
        slab = tok_gemm(hid, W2[:, iw * SLICE:(iw + 1) * SLICE], 1, defect)
        if stride_w == R and nst == T:
            ws[i * R * C:(i + 1) * R * C] = slab[:, :T].reshape(-1)
            continue
        for b in range(B):                                # dead rows first: a live row of the next image wins the race where both land
            at = ((i * stride_w + b * T) + torch.arange(nst)) * C
            for r in list(range(T, nst)) + list(range(T)):
                if at[r] + C <= ws.numel():
                    ws[at[r]:at[r] + C] = slab[b, r]
    nsum = NSLICE - 1 if defect == D[14] else NSLICE
    rows = (torch.arange(B)[:, None] * T + torch.arange(T)[None, :])
    tot = None
    for i in range(nsum):
        sl = ws[:NSLICE * R * C].view(NSLICE, R, C)[i][rows]
        tot = sl if tot is None else tot + sl
    pre3 = (tot + _f(E["b2"])) + y2[:, :T]
    y3 = _ln32(pre3, _f(E["ln3_w"]), _f(E["ln3_b"]), _eps(eps3, defect))
    pe = _f(E["pe"]).view(B, T, C)
    a_k, a_v = torch.zeros(B, MAXT, C, dtype=F32), torch.zeros(B, MAXT, C, dtype=F32)
    a_k[:, :T], a_v[:, :T] = r16(y3 + pe, op16), r16(y3, op16)
    lo, hi = (a_v, a_k) if defect == D[2] else (a_k, a_v)
    Wkv = _f(E["wkv"])
    kv = r16(torch.cat([tok_gemm(lo, Wkv[:CI], 1, defect), tok_gemm(hi, Wkv[CI:], 1, defect)], -1) + _f(E["bkv"]), op16)
    n16 = MAXT if defect == D[16] else T
    out = {"queries_mid": _store(y2, B, T, T), "queries_out": _store(torch.cat([y3, torch.zeros(B, MAXT - T, C)], 1), B, T, T),
           "kv": _store(kv, B, T, n16), "ws": ws}
    if E["wfq"] is not None:
        src = a_v if defect == D[3] else a_k
        out["qp_final"] = _store(r16(tok_gemm(src, _f(E["wfq"]), 4, defect) + _f(E["bfq"]), op16), B, T, n16)
    return out


def restate(E, op16, defect=None):
    return {"self": restate_self, "tail": restate_tail, "mlp": restate_mlp}[E["kind"]](E, op16, defect)


def expected(E, op16):
    """{name: ("bits", 16-bit tensor) | ("bound", float64 ref, bound)} of a case's outputs, and "ws": the exact slabs"""
    if E["kind"] == "self":
        return {"queries_out": ("bound",) + ln_bound_exact(E["pre"], E["ln_w"], E["ln_b"], E["eps"]), "qp": ("bits", E["qp"].to(op16))}
    if E["kind"] == "tail":
        return {"queries_out": ("bound",) + ln_bound_exact(E["pre"], E["ln_w"], E["ln_b"], E["eps"])}
    ref3, b3 = ln_bound(E["pre3"], E["ln3_w"], E["ln3_b"], E["eps3"], E["delta"])
    out = {"queries_mid": ("bound",) + ln_bound_exact(E["pre2"], E["ln2_w"], E["ln2_b"], E["eps2"]), "queries_out": ("bound", ref3, b3),
           "kv": ("bits", E["kv"].to(op16)), "ws": ("bits", E["slabs"].to(F32))}
    if E["last"]:
        out["qp_final"] = ("bits", E["qpf"].to(op16))
    return out


def bits_differ(a, b):
    it = {2: torch.int16, 4: torch.int32}[a.dtype.itemsize]
    return not torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def verdict(got, E, op16):
    """what the GPU file would see of a restated run: "sentinel" (a store outside an output or behind the workspace), "missing" (an
    output row never stored), "bits", "bound" or None"""
    exp = expected(E, op16)
    R = E["B"] * E["T"]
    for name, want in exp.items():
        if name == "ws":
            ws = got["ws"]
            if not bool(torch.isnan(ws[NSLICE * R * C:]).all()):
                return "sentinel"
            if bits_differ(ws[:NSLICE * R * C].view(NSLICE, R, C), want[1]):
                return "bits"
            continue
        rows, vals = got[name]
        if bool((rows >= R).any()):
            return "sentinel"
        if sorted(set(rows.tolist())) != list(range(R)):
            return "missing"
        full = torch.zeros(R, vals.shape[1], dtype=vals.dtype)
        full[rows] = vals                                 # (a row stored twice: the later image's own store comes last)
        if want[0] == "bits":
            if bits_differ(full.to(op16), want[1]):
                return "bits"
        elif not bool(((full.double() - want[1]).abs() <= want[2]).all()):
            return "bound"
    return None
