"""Case tables, operand builders, exactness conditions, float64 references and simulated defects of the variant matrix of the full-row
kernels on the 64-row, all-columns tile of csrc/rowtile.h: gemm_rowln_kernel<384,0>, <256,0>, <256,64>, <256,256> (csrc/gemm_rowln.hip)
and mlp_rowln_kernel<384,0> (csrc/mlp_rowln.hip).

Plain torch, no GPU needed: tests/test_rowtile_variants_gpu.py runs the cases on the card (device="cuda"), tests/test_rowtile_cases_cpu.py
proves on the CPU that the builders and references do what the GPU file relies on and that every simulated defect fails its case.

Two passes per case:
  exact   operands built so that a correct kernel's C32 AND Y16 are known to the bit in fp16 and in bf16 (no tolerance, no kernel of the
          library in the expected value):
          * target rows x = m + a s (s a balanced +-1 pattern over the N columns, a in {1/4 .. 4}, m a small integer, one row per case with
            m = 1000): mean = m and sum d^2 = N a^2 are exact in any fp32 order, and with ln_w in {+-1, +-2}, ln_b in {+-4, +-5} the
            LayerNorm value lies within 1.7e-4 of the integer s g + b of magnitude 2..7 -- Y16 is that integer;
          * GEMM side: A small integers, W a fixed number of +-1 per row, integer bias, R32 = x - (A W^T + bias): every partial sum is an
            integer (merged form: a multiple of 1/8) below 2^24, (acc + bias) + r is exact in any order and C32 == x;
          * MLP: integers all the way (fused_cases.mlp_exact's construction): hidden pre-activations are integers in [8, 185], where GELU is
            the identity far below half a bf16 ulp;
          * merged A: partials small integers, live splits of a row share one maximum (exp2(0) = 1) and carry power-of-two sums whose total
            is a power of two; empty splits are (-inf, 0) with NaN partials; dead splits have a finite maximum >= 200 below the row's (their
            weight is exactly 0: 2^-200 is below the smallest fp32 denormal), a sum > 0 and large finite partials.
  random  seeded randn operands as the family's older files build them (residual rows offset and scaled over two decades, one row with
          mean = 1000 std, one near-constant row) against float64 references of the operand-rounded inputs, with the project's own bounds.

restate() walks the tile in fp32 as the kernels do (tile order, row clamp, wave -> (row slab, column quarter), the accumulator's
s_frag_key rows, stage and chunk order, hidden-image placement, the merge with its clamped split loads, the epilogue's 16 lanes per row)
and takes a `defect=` switch: every defect of DEFECTS must change the exact pass's bits or store outside the output.
"""
import math

import torch

from fused_cases import exact16, next_norm_reference, r16  # noqa: F401  (next_norm_reference: the Y16 bound of the random pass)

BM = 64                                   # rows of a tile: one workgroup
GRID_WRAP = 256                           # workgroups beyond this: the prefetch place wraps, a CU takes a second workgroup
EPS = {384: 1e-6, 256: 1e-5}              # as the product passes it: Hiera stage 3, the memory attention
F32 = torch.float32


# ---------------------------------------------------------------------------------------------------------------------------------
# kernel keys (helpers.kernel_key spelling) and the case tables
def GEMM(N, MD):
    return f"gemm_rowln_kernel<{N},{MD}>"


MLP = "mlp_rowln_kernel<384,0>"
# M: a lone row; just below, on and above a tile boundary; the same at the second boundary; three full tiles and one of 8 rows
SMALL_M = (1, 63, 64, 65, 127, 200)
# 1089: 18 workgroups = 8 * 2 + 2 (xcd_tile_order with quotient and remainder non-zero, prefetch places 0..2); 16901: 265 workgroups --
# the grid exceeds 256, so the prefetch place wraps, CUs take a second workgroup, and the last tile has 5 rows
LARGE_M = (1089, 16901)
PLAIN_K = {384: (64, 128, 384, 1536), 256: (64, 256, 2048)}
MERGED_D = (64, 256)
SPLITS = (2, 3, 4, 5, 7, 8)               # the branch `splits > 4` changes between 4 and 5
MLP_H = (128, 256, 1536)
PERM_M = 200                              # the ragged M of the token-order test


def case(kind, N, K, M, bias=True, splits=0):
    """kind "plain" (ops.gemm_residual_layernorm; K), "merged" (ops.gemm_merged_residual_layernorm; K = D), "mlp"
    (ops.mlp_residual_layernorm; K = H)"""
    expect = MLP if kind == "mlp" else GEMM(N, K if kind == "merged" else 0)
    return dict(kind=kind, N=N, K=K, M=M, bias=bias, splits=splits, large=M in LARGE_M, expect=expect)


PLAIN_CASES = ([case("plain", N, K, M, b) for N in (384, 256) for K in PLAIN_K[N] for M in SMALL_M for b in (True, False)]
               + [case("plain", N, max(PLAIN_K[N]), M) for N in (384, 256) for M in LARGE_M])
# every D x splits x M; the bias is on and off for every D, every split count and every M
MERGED_CASES = ([case("merged", 256, D, M, (i + k) % 2 == 0, s) for D in MERGED_D for i, s in enumerate(SPLITS) for k, M in enumerate(SMALL_M)]
                + [case("merged", 256, D, M, True, s) for D in MERGED_D for M, s in zip(LARGE_M, (5, 8))])
MLP_CASES = ([case("mlp", 384, H, M, b) for H in MLP_H for M in SMALL_M for b in (True, False)]
             + [case("mlp", 384, max(MLP_H), M) for M in LARGE_M])
CASES = PLAIN_CASES + MERGED_CASES + MLP_CASES


def case_id(c):
    return (f"{c['kind']}-n{c['N']}-k{c['K']}-m{c['M']}" + (f"-s{c['splits']}" if c["kind"] == "merged" else "")
            + ("" if c["bias"] else "-nobias"))


BY_ID = {case_id(c): c for c in CASES}


def instantiations():
    """every kernel instantiation the tables reach"""
    return sorted({c["expect"] for c in CASES})


def _seed(c, salt):
    return salt + 1000003 * c["N"] + 7919 * c["K"] + 31 * c["M"] + 13 * c["splits"] + int(c["bias"])


def cdiv(a, b):
    return (a + b - 1) // b


def xcd_tile_order(idx, n):
    """common.h: workgroup idx of a launch of n -> tile index (every XCD walks one contiguous slice of the tiles)"""
    q, rem = n // 8, n % 8
    xcd = idx % 8
    return torch.where(xcd < rem, xcd * (q + 1), rem * (q + 1) + (xcd - rem) * q) + idx // 8


def prefetch_places(n):
    """the W prefetch's j = (blockIdx.x >> 3) & 31 over a launch of n workgroups"""
    return sorted({(b >> 3) & 31 for b in range(n)})


# ---------------------------------------------------------------------------------------------------------------------------------
# exact pass: builders
def sparse_rows(rows, cols, nnz, g, device):
    """[rows, cols] of {-1, 0, 1} with exactly nnz entries of +-1 per row (fused_cases._sparse_signs with placed entries): entry i of row j
    lies in the 16-wide k-step (j nnz + i) % (cols / 16), so consecutive rows walk the k-steps round-robin -- every 32-row block of the
    matrix (one wave's rows) has signal in every k-step and so in every 64-wide stage -- at a place of the step drawn per row."""
    nks = cols // 16
    assert cols % 16 == 0 and nnz <= 16 * nks and cdiv(nnz, nks) <= 16
    j = torch.arange(rows, device=device)[:, None]
    i = torch.arange(nnz, device=device)[None, :]
    step = (j * nnz + i) % nks
    perm = torch.rand(rows, 16, generator=g, device=device).argsort(1)
    place = perm.gather(1, ((i // nks + i % nks) % 16).expand(rows, nnz))     # entries that share a step differ in i // nks
    sg = torch.randint(0, 2, (rows, nnz), generator=g, device=device).double() * 2 - 1
    w = torch.zeros(rows, cols, dtype=torch.float64, device=device).scatter_(1, step * 16 + place, sg)
    assert bool((w.abs().sum(1) == nnz).all()), "no two entries of a row fell on one place"
    assert float(w.reshape(cdiv(rows, 32), -1, nks, 16).abs().sum((1, 3)).min()) > 0 or rows % 32, "every k-step of every 32-row block carries signal"
    return w


def stepped_bias(n, device):
    """integer bias that steps with the column and with its 32-column block: no shift by whole blocks goes unseen"""
    j = torch.arange(n, device=device)
    return ((j + j // 32) % 4).double() - 1.0


def target_rows(M, N, eps, g, device):
    """(x, y, ln_w, ln_b): the rows a correct kernel must produce -- C32 == x and Y16 == y to the bit.  Asserts its own conditions."""
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g, device=device).double()
    s = (torch.rand(M, N, generator=g, device=device).argsort(1) < N // 2).double() * 2 - 1           # balanced: half +1, half -1
    a = 2.0 ** ri(-2, 2, M, 1)
    m = ri(-3, 3, M, 1)
    m[M // 2] = 1000.0                                                       # one row whose mean is >= 250 standard deviations
    ln_w = (2 * ri(0, 1, N) - 1) * ri(1, 2, N)
    ln_b = (2 * ri(0, 1, N) - 1) * ri(4, 5, N)
    x = m + a * s
    y = s * ln_w + ln_b
    assert bool((s.sum(1) == 0).all()), "balanced: the row sum is N m"
    assert N * (float(m.abs().max()) + float(a.max())) * 4 < 2 ** 24, "every partial sum of a row is a multiple of 1/4 below 2^24: exact in any order"
    assert bool((x.float().double() == x).all()) and exact16(y) and 2 <= float(y.abs().min()) and float(y.abs().max()) <= 7
    # sum d^2 = N a^2 is a power of two times N <= 384: exact; rstd = (a^2 + eps)^-1/2, and |g| |a rstd - 1| is the distance to the integer
    dev = float(ln_w.abs().max()) * float((1 - a / torch.sqrt(a * a + eps)).abs().max())
    assert dev < 1.7e-4 < 2.0 ** -9 / 8, "the LayerNorm value lies far inside half a 16-bit ulp (fp16 at 4..8: 2^-9) of the integer"
    return x, y, ln_w, ln_b


def _gemm_side(c, x, A, g, device, nnz=8):
    """W [N, K] sparse signs, bias (or None), R32 = x - (A W^T + bias)"""
    N, K = c["N"], c["K"]
    W = sparse_rows(N, K, nnz, g, device)
    assert torch.unique(W, dim=0).shape[0] == N, "no two output columns share a pattern"
    bias = stepped_bias(N, device) if c["bias"] else None
    pre = A @ W.T + (bias if c["bias"] else 0.0)
    R = x - pre
    assert float(A.abs().max()) * nnz + 4 < 2 ** 24 and bool((R.float().double() == R).all()), "integer partial sums; R32 is an fp32 value"
    return W, bias, R


def plain_exact(c, device="cpu"):
    g = torch.Generator(device=device).manual_seed(_seed(c, 11))
    M, N, K = c["M"], c["N"], c["K"]
    x, y, ln_w, ln_b = target_rows(M, N, EPS[N], g, device)
    A = torch.randint(-3, 4, (M, K), generator=g, device=device).double()
    W, bias, R = _gemm_side(c, x, A, g, device)
    assert exact16(A) and exact16(W)
    return dict(c, A=A, W=W, b=bias, R=R, x=x, y=y, ln_w=ln_w, ln_b=ln_b, eps=EPS[N])


# power-of-two partitions of 1 into n parts, none below 1/8 (the merged value is then a multiple of 1/8): split the largest part > 1/8
def _partition(n):
    p = [1.0]
    while len(p) < n:
        p.sort(reverse=True)
        assert p[0] > 0.125
        p = p[1:] + [p[0] / 2, p[0] / 2]
    return sorted(p, reverse=True)


PARTS = torch.tensor([[0.0] * 8] + [_partition(n) + [0.0] * (8 - n) for n in range(1, 9)], dtype=torch.float64)
LIVE, EMPTY, DEAD = 0, 1, 2
PATTERNS = ["all live", "only the first live", "only the last live", "only split 4 live (splits >= 5; else live and empty alternating)",
            "live and dead alternating"]


def split_states(M, S, device="cpu"):
    """[S, M] of LIVE / EMPTY / DEAD: the patterns of PATTERNS spread over the rows, row M - 1 always one of the single-live ones; the
    other splits of a single-live row are empty and dead in turn"""
    row = torch.arange(M, device=device)[None, :]
    u = torch.arange(S, device=device)[:, None]
    pat = (row % 5).clone()
    pat[0, M - 1] = (1, 2, 3 if S >= 5 else 1)[M % 3]
    other = torch.where((u + row) % 2 == 1, EMPTY, DEAD)
    st = torch.full((S, M), LIVE, device=device)
    st = torch.where(pat == 1, torch.where(u == 0, LIVE, other), st)
    st = torch.where(pat == 2, torch.where(u == S - 1, LIVE, other), st)
    p3 = torch.where(u == 4, LIVE, other) if S >= 5 else torch.where(u % 2 == 0, LIVE, EMPTY).expand(S, M)
    st = torch.where(pat == 3, p3, st)
    st = torch.where(pat == 4, torch.where(u % 2 == (row // 5) % 2, LIVE, DEAD), st)
    assert bool(((st == LIVE).sum(0) >= 1).all())
    return st


def merged_exact(c, device="cpu"):
    g = torch.Generator(device=device).manual_seed(_seed(c, 12))
    M, N, D, S = c["M"], c["N"], c["K"], c["splits"]
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g, device=device).double()
    x, y, ln_w, ln_b = target_rows(M, N, EPS[N], g, device)
    st = split_states(M, S, device)
    live = st == LIVE
    rowmax = ri(-6, 6, M) + 0.25 * ri(0, 3, M)                                # the maximum varies from row to row (stored log2 domain)
    mx = torch.where(live, rowmax, rowmax - 200.0 - ri(0, 50, S, M))          # dead: >= 200 below
    mx = torch.where(st == EMPTY, torch.full_like(mx, -math.inf), mx)
    n = live.sum(0)
    rank = (live.long().cumsum(0) - 1 + torch.randint(0, 8, (M,), generator=g, device=device)) % n
    total = 2.0 ** ri(-2, 3, M)                                               # the row's live total: a power of two
    sm = PARTS.to(device)[n[None, :].expand(S, M), rank] * total
    sm = torch.where(live, sm, torch.where(st == DEAD, ri(1, 5, S, M), torch.zeros_like(sm)))
    part = torch.where(live[..., None], ri(-3, 3, S, M, D), (512.0 + 64 * ri(0, 7, S, M, D)) * (2 * ri(0, 1, S, M, D) - 1))
    part = torch.where((st == EMPTY)[..., None], torch.full_like(part, math.nan), part)
    L = (sm * live).sum(0)
    A = (torch.where(live[..., None], part, torch.zeros_like(part)) * (sm * live / L)[..., None]).sum(0)
    assert bool((torch.log2(L) == torch.log2(L).round()).all()) and bool((torch.log2(sm[live]) == torch.log2(sm[live]).round()).all())
    assert bool((A * 8 == (A * 8).round()).all()) and exact16(A), "the merged value is a multiple of 1/8, exact in both 16-bit types"
    assert exact16(torch.nan_to_num(part)) and bool((mx[st == DEAD] <= rowmax.expand(S, M)[st == DEAD] - 200).all())
    assert bool((sm[st == DEAD] > 0).all()) and bool((sm[st == EMPTY] == 0).all())
    W, bias, R = _gemm_side(c, x, A, g, device)
    return dict(c, part=part, mx=mx, sm=sm, st=st, A=A, W=W, b=bias, R=R, x=x, y=y, ln_w=ln_w, ln_b=ln_b, eps=EPS[N])


N_OFF7, N_OFF1 = 14, 3          # bias off: 14 columns of A hold 7 and 3 hold 1; W1 turns them into the offset 98 + {0..3}


def mlp_exact(c, device="cpu"):
    """fused_cases.mlp_exact's integer construction on this kernel's operands.  A holds integers in [-7, 7] (the rows are already
    normalised), W1 12 entries of +-1 per row, b1 = 92 + {0..3} stepping with the unit, with its 32-block and with its 128-chunk: hidden
    pre-activations are integers in [8, 179].  Without biases the same offset comes out of fc1 itself: 14 reserved columns of A hold 7 and
    W1 has +1 there (98), three hold 1 and W1 row j has +1 in the first step(j) of them -- integers in [14, 185].  W2 has 24 entries of
    +-1 per row, b2 is integer, R32 = x - (h W2^T + b2)."""
    g = torch.Generator(device=device).manual_seed(_seed(c, 13))
    M, N, H = c["M"], c["N"], c["K"]
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g, device=device).double()
    x, y, ln_w, ln_b = target_rows(M, N, EPS[N], g, device)
    A = ri(-7, 7, M, N)
    W1 = sparse_rows(H, N, 12, g, device)
    j = torch.arange(H, device=device)
    step = (j + j // 32 + j // 128) % 4
    if c["bias"]:
        b1, b2 = 92.0 + step.double(), stepped_bias(N, device) * 3
    else:
        b1 = b2 = None
        cols = torch.rand(N, generator=g, device=device).argsort()[:N_OFF7 + N_OFF1]
        A[:, cols[:N_OFF7]] = 7.0
        A[:, cols[N_OFF7:]] = 1.0
        W1[:, cols[:N_OFF7]] = 1.0
        W1[:, cols[N_OFF7:]] = (torch.arange(N_OFF1, device=device)[None, :] < step[:, None]).double()
    hid = A @ W1.T + (b1 if c["bias"] else 0.0)
    assert bool((hid == hid.round()).all()) and 8 <= float(hid.min()) and float(hid.max()) <= 185 and exact16(hid)
    W2 = sparse_rows(N, H, 24, g, device)
    pre = hid @ W2.T + (b2 if c["bias"] else 0.0)
    R = x - pre
    assert float(pre.abs().max()) < 2 ** 24 and bool((R.float().double() == R).all()) and exact16(A) and exact16(W1) and exact16(W2)
    # every 128-unit chunk's contribution differs: from the others' and between its two halves
    if M >= 8:
        contrib = torch.stack([hid[:64, k:k + 64] @ W2[:, k:k + 64].T for k in range(0, H, 64)])
        assert torch.unique(contrib.reshape(H // 64, -1), dim=0).shape[0] == H // 64
    return dict(c, A=A, W1=W1, b1=b1, W2=W2, b=b2, hid=hid, R=R, x=x, y=y, ln_w=ln_w, ln_b=ln_b, eps=EPS[N])


def exact(c, device="cpu"):
    return {"plain": plain_exact, "merged": merged_exact, "mlp": mlp_exact}[c["kind"]](c, device)


ROW_KEYS = ("A", "R", "x", "y", "hid", "ref", "pre", "S", "widen")        # [M, ...] tensors
SPLIT_KEYS = ("part", "mx", "sm", "st")                          # [splits, M, ...] tensors


def permute_rows(E, perm):
    """the case with its rows (A, the workspace's rows, R32 and the expected rows alike) in the order perm"""
    out = dict(E)
    for k in ROW_KEYS:
        if out.get(k) is not None:
            out[k] = out[k][perm]
    for k in SPLIT_KEYS:
        if out.get(k) is not None:
            out[k] = out[k][:, perm]
    return out


def workspace_bytes(E, op16):
    """the split-KV workspace of the attention ABI for one head and M rows: [splits][M][D] 16-bit partials, then [splits][M][2] fp32
    (max, sum), as a uint8 tensor"""
    pb = E["part"].to(op16).contiguous().view(torch.uint8).flatten()
    mb = torch.stack([E["mx"], E["sm"]], -1).to(F32).contiguous().view(torch.uint8).flatten()
    return torch.cat([pb, mb])


# ---------------------------------------------------------------------------------------------------------------------------------
# random pass: operands (float64 holders of fp32 / 16-bit values) and float64 references
def _row_side(c, g, device):
    M, N = c["M"], c["N"]
    rn = lambda *s: torch.randn(*s, generator=g, device=device)
    scale = 10.0 ** (torch.rand(M, 1, generator=g, device=device) * 2 - 1)
    r = rn(M, N) * scale + rn(M, 1) * 3
    if M > 2:
        r[1] = 1000.0 + rn(N)                                                # a row whose mean is ~1000 standard deviations
    return r, rn(N).double(), rn(N).double()


def _finish(E, pre):
    """R32's last row makes a near-constant C32 row (2 + the kernel's own error: a variance around eps); the float64 reference"""
    r = E.pop("r32")
    if E["M"] > 1:
        r[-1] = (2.0 - pre[-1]).float()
    E["R"] = r.double()
    E["pre"], E["ref"] = pre, pre + E["R"]
    return E


def plain_random(c, op16, device="cpu"):
    g = torch.Generator(device=device).manual_seed(_seed(c, 21))
    M, N, K = c["M"], c["N"], c["K"]
    rn = lambda *s: torch.randn(*s, generator=g, device=device)
    A = r16(rn(M, K), op16).double()
    W = r16(rn(N, K) * K ** -0.5, op16).double()
    bias = (rn(N) * 0.5).double() if c["bias"] else None
    r, ln_w, ln_b = _row_side(c, g, device)
    E = dict(c, A=A, W=W, b=bias, r32=r, ln_w=ln_w, ln_b=ln_b, eps=EPS[N], S=A.abs() @ W.abs().T)
    return _finish(E, A @ W.T + (bias if c["bias"] else 0.0))


def ulp16(t, op16):
    """the spacing of the 16-bit type at |t| (fp16: not below its subnormal spacing 2^-24)"""
    e = torch.frexp(t.abs().double())[1].double() - 1
    if op16 == torch.float16:
        return 2.0 ** (torch.where(t == 0, torch.full_like(e, -14.0), e).clamp(min=-14) - 10)
    return torch.where(t == 0, torch.zeros_like(e), 2.0 ** (e - 7))


def merge_reference(part, mx, sm):
    """float64 merge of split-KV partials (log2-domain maxima): sum_u l_u 2^(m_u - max) O_u / sum_u l_u 2^(m_u - max) over the splits
    with a finite maximum; the partials of the others are never read"""
    top = mx.amax(0, keepdim=True)
    w = torch.where(torch.isinf(mx), torch.zeros_like(sm), sm * torch.exp2(mx - top))
    o = torch.where(torch.isinf(mx)[..., None], torch.zeros_like(part), part)
    return (w[..., None] * o).sum(0) / w.sum(0)[..., None]


def merged_random(c, op16, device="cpu"):
    """tests/test_memattn_tail_gpu.py::fabricated_workspace's content: random partials and pairs with sum > 0; split 1 empty on every row;
    on rows 0, 7 and M - 1 all splits but the last are empty; the partials of empty splits are NaN"""
    g = torch.Generator(device=device).manual_seed(_seed(c, 22))
    M, N, D, S = c["M"], c["N"], c["K"], c["splits"]
    rn = lambda *s: torch.randn(*s, generator=g, device=device)
    part = r16(rn(S, M, D), op16).double()
    mx = (rn(S, M) * 3).double()
    sm = (torch.rand(S, M, generator=g, device=device) * 5 + 0.1).double()
    empty = torch.zeros(S, M, dtype=torch.bool, device=device)
    empty[1] = True
    if S > 2:
        for row in {0, min(7, M - 1), M - 1}:
            empty[:, row] = True
            empty[S - 1, row] = False
    mx[empty], sm[empty], part[empty] = -math.inf, 0.0, math.nan
    mx, sm = mx.float().double(), sm.float().double()
    A = r16(merge_reference(part, mx, sm), op16)                              # the kernel rounds an fp32 sum: within one 16-bit ulp of this
    W = r16(rn(N, D) * D ** -0.5, op16).double()
    bias = (rn(N) * 0.5).double() if c["bias"] else None
    r, ln_w, ln_b = _row_side(c, g, device)
    ua = ulp16(A, op16)
    E = dict(c, part=part, mx=mx, sm=sm, A=A, W=W, b=bias, r32=r, ln_w=ln_w, ln_b=ln_b, eps=EPS[N], S=(A.abs() + ua) @ W.abs().T,
             widen=ua @ W.abs().T)                                           # one 16-bit ulp of each A element times |W|
    return _finish(E, A @ W.T + (bias if c["bias"] else 0.0))


def gelu64(t):
    return 0.5 * t * (1 + torch.erf(t / math.sqrt(2.0)))


def mlp_random(c, op16, device="cpu"):
    g = torch.Generator(device=device).manual_seed(_seed(c, 23))
    M, N, H = c["M"], c["N"], c["K"]
    rn = lambda *s: torch.randn(*s, generator=g, device=device)
    A = r16(rn(M, N), op16).double()
    W1 = r16(rn(H, N) * N ** -0.5, op16).double()
    W2 = r16(rn(N, H) * H ** -0.5, op16).double()
    b1 = (rn(H) * 0.5).double() if c["bias"] else None
    b2 = (rn(N) * 0.5).double() if c["bias"] else None
    r, ln_w, ln_b = _row_side(c, g, device)
    E = dict(c, A=A, W1=W1, b1=b1, W2=W2, b=b2, r32=r, ln_w=ln_w, ln_b=ln_b, eps=EPS[N])
    hid = gelu64(A @ W1.T + (b1 if c["bias"] else 0.0))
    return _finish(E, hid @ W2.T + (b2 if c["bias"] else 0.0))


def random(c, op16, device="cpu"):
    return {"plain": plain_random, "merged": merged_random, "mlp": mlp_random}[c["kind"]](c, op16, device)


def layernorm64(x, g, b, eps):
    x = x.double()
    d = x - x.mean(1, keepdim=True)
    return d / torch.sqrt((d * d).mean(1, keepdim=True) + eps) * g + b


# ---------------------------------------------------------------------------------------------------------------------------------
# the tile walk restated in fp32, with simulated defects
EPILOGUE_DEFECTS = ["two column quarters exchanged", "the + 4 h term of the accumulator row map dropped", "bias one 32-block off",
                    "residual read from the clamped row instead of the own row", "rows past M stored",
                    "Y16 computed from the pre-residual value", "mean taken over N + 4 (the tile's padding columns)"]
RING_DEFECTS = ["a k-step served from the other ring slot", "the last k-step skipped when nk is odd", "chunk c using chunk c - 1's b1",
                "chunk c using chunk c - 1's W1", "fc2's second half reading hidden image 0 again",
                "hidden units of the two lane halves exchanged"]
MERGE_DEFECTS = ["the upper four splits not loaded at splits = 5", "the u < splits test dropped", "an empty split not skipped",
                 "a dead split given weight l instead of l e", "the split stride taken as 64 rows instead of M"]
DEFECTS = EPILOGUE_DEFECTS + RING_DEFECTS + MERGE_DEFECTS


def s_frag_key(e, h):
    return (e & 3) + 8 * (e >> 2) + 4 * h


def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in float64"""
    return (a.double() * b.double() + c.double()).float()


def _merge_tile(E, crow, op16, defect):
    """gemm_rowln_kernel's merged-A prologue for the rows crow [T, 64]: every pair and partial row loaded up front with the split index
    clamped, the upper four only where there are more than four splits (else copies of split 0), then attn_merge_kernel's arithmetic"""
    S, M, D = E["splits"], E["M"], E["K"]
    part = E["part"].to(op16).to(F32).reshape(S * M, D)
    mx, sm = E["mx"].to(F32).reshape(S * M), E["sm"].to(F32).reshape(S * M)
    stride = BM if defect == "the split stride taken as 64 rows instead of M" else M

    def load(u):
        at = (min(u, S - 1) * stride + crow).clamp(max=S * M - 1)
        return mx[at], sm[at], part[at]
    ld = [load(u) for u in range(4)]
    upper = S > (5 if defect == "the upper four splits not loaded at splits = 5" else 4)
    ld += [load(u) for u in range(4, 8)] if upper else [ld[0]] * 4
    counted = lambda u: u < S or defect == "the u < splits test dropped"
    top = torch.full_like(ld[0][0], -math.inf)
    for u in range(8):
        if counted(u):
            top = torch.maximum(top, ld[u][0])
    L = torch.zeros_like(top)
    acc = torch.zeros(*crow.shape, D, dtype=F32)
    for u in range(8):
        m, l, o = ld[u]
        if not counted(u):
            continue
        go = torch.ones_like(m, dtype=torch.bool) if defect == "an empty split not skipped" else m != -math.inf
        ex = torch.exp2(m - top)
        w = l if defect == "a dead split given weight l instead of l e" else l * ex
        L = torch.where(go, _fma(l, ex, L), L)
        acc = torch.where(go[..., None], _fma(w[..., None], o, acc), acc)
    return r16(acc * (1.0 / L)[..., None], op16)


def _steps16(acc, a, w, k0, k1):
    """MFMA steps of 16, k ascending: acc [T, rows, cols] += a[..., k] w[cols, k]^T"""
    for k in range(k0, k1, 16):
        acc = acc + a[..., k:k + 16] @ w[:, k:k + 16].T
    return acc


def _gemm_main(At, W, defect, merged):
    """the two-stage ring of 64-wide stages: stage kt lies in slot kt & 1 (merged: W alone, A is the resident image kt)"""
    K = W.shape[1]
    nk = K // 64
    acc = torch.zeros(At.shape[0], BM, W.shape[0], dtype=F32)
    for kt in range(nk):
        if defect == "the last k-step skipped when nk is odd" and nk % 2 == 1 and kt == nk - 1:
            break
        src = kt
        if defect == "a k-step served from the other ring slot" and kt == 1:
            src = 0                                           # the other slot still holds stage 0 (merged: of W alone)
        a_img = At[..., 64 * (kt if merged else src):][..., :64]
        acc = _steps16(acc, a_img, W[:, 64 * src:64 * src + 64], 0, 64)
    return acc


def _gelu32(t):
    return 0.5 * t * (1 + torch.erf(t * torch.tensor(math.sqrt(0.5), dtype=F32)))


def _mlp_main(E, At, op16, defect):
    """mlp_rowln_kernel's chunk loop: per 128-unit chunk, fc1 transposed (hidden unit x token) over the six resident k images in two
    ring stages, + b1, GELU, rounding, the store into the hidden image; then two fc2 k-steps of 64 against W2's stages"""
    W1, W2 = E["W1"].to(F32), E["W2"].to(F32)
    H, N = W1.shape
    b1 = torch.zeros(H) if E["b1"] is None else E["b1"].to(F32)
    u = torch.arange(128)
    wq, within = u // 32, u % 32
    h = (within >> 2) & 1                                     # the unit's lane half: within = s_frag_key(e, h)
    if defect == "hidden units of the two lane halves exchanged":
        h = 1 - h
    # lane (r, h), register e of wave (ws, wq) stores unit 32 wq + s_frag_key(e, h) of token 32 ws + r into image wq >> 1, 16-byte chunk
    # 4 (wq & 1) + (e >> 2), half h, element e & 3
    dest = (wq >> 1) * 64 + ((wq & 1) * 4 + (within >> 3)) * 8 + 4 * h + (within & 3)
    acc = torch.zeros(At.shape[0], BM, N, dtype=F32)
    for c in range(H // 128):
        cw = c - 1 if defect == "chunk c using chunk c - 1's W1" and c > 0 else c
        cb = c - 1 if defect == "chunk c using chunk c - 1's b1" and c > 0 else c
        acc1 = torch.zeros(At.shape[0], 128, BM, dtype=F32)
        w1c = W1[128 * cw:128 * cw + 128]
        for t in range(2):                                    # ring stage t: k images 3 t .. 3 t + 2
            for k in range(192 * t, 192 * t + 192, 16):
                acc1 = acc1 + w1c[:, k:k + 16] @ At[..., k:k + 16].transpose(1, 2)
        act = r16(_gelu32(acc1 + b1[128 * cb:128 * cb + 128, None]), op16)
        hid = torch.zeros(At.shape[0], BM, 128, dtype=F32)
        hid[:, :, dest] = act.transpose(1, 2)
        for step in range(2):                                 # hidden image `step` against ring slot `step`
            img = 0 if defect == "fc2's second half reading hidden image 0 again" else step
            acc = _steps16(acc, hid[..., 64 * img:64 * img + 64], W2[:, 128 * c + 64 * step:128 * c + 64 * step + 64], 0, 64)
    return acc


def restate(E, op16, defect=None, blocks=None):
    """The case's launch restated: (rows, c32, y16) -- the output rows the kernel stores, as indices into the [M, N] outputs (past their end
    for a defect that stores them), and their fp32 / 16-bit values.  blocks: the workgroup ids to walk (default: all)."""
    kind, M, N = E["kind"], E["M"], E["N"]
    FN, CH, TLD = N // 128, N // 64, N + 4
    nt = cdiv(M, BM)
    blk = torch.arange(nt) if blocks is None else torch.as_tensor(blocks)
    m0 = xcd_tile_order(blk, nt) * BM
    lrow = torch.arange(BM)
    grow = m0[:, None] + lrow                                 # [T, 64]
    crow = grow.clamp(max=M - 1)                              # rows past M are clamped on load
    if kind == "merged":
        At = _merge_tile(E, crow, op16, defect)
    else:
        At = E["A"].to(F32)[crow]
    if kind == "mlp":
        full = _mlp_main(E, At, op16, defect)
    else:
        full = _gemm_main(At, E["W"].to(F32), defect, kind == "merged")
    T = len(blk)
    # the accumulators: wave = 4 ws + wq owns rows 32 ws .., columns wq N / 4 ..; register e of lane (r, h) of accumulator j is row
    # s_frag_key(e, h), column 32 j + r of that block
    wave, j, lane, e = torch.meshgrid(torch.arange(8), torch.arange(FN), torch.arange(64), torch.arange(16), indexing="ij")
    ws, wq, r, h = wave >> 2, wave & 3, lane & 31, lane >> 5
    reg = full[:, ws * 32 + s_frag_key(e, h), wq * (N // 4) + j * 32 + r]                # [T, 8, FN, 64, 16]
    bias = torch.zeros(N) if E["b"] is None else E["b"].to(F32)
    bcol = wq * (N // 4) + j * 32 + r
    if defect == "bias one 32-block off":
        bcol = (bcol - 32) % N
    # acc + bias -> the row-major tile [64][N + 4]
    wq_w = wq ^ 1 if defect == "two column quarters exchanged" else wq
    h_w = 0 * h if defect == "the + 4 h term of the accumulator row map dropped" else h
    trow, tcol = ws * 32 + s_frag_key(e, h_w), wq_w * (N // 4) + j * 32 + r
    tile = torch.zeros(T, BM, TLD, dtype=F32)
    val = reg + bias[bcol]
    for half in (0, 1):                                       # lane half 1 is the later writer where two lanes meet
        sel = h == half
        tile[:, trow[sel], tcol[sel]] = val[:, sel]
    # the walk: 16 lanes per row, lane chunk l16 + 16 j, row ps * 32 + wave * 4 + (lane >> 4) -- every local row once
    rrow = lrow
    if defect == "residual read from the clamped row instead of the own row":
        rrow = lrow.clamp(max=(M - 1) % BM)                   # the ragged tile's row limit applied to every tile
    R = E["R"].to(F32)[(m0[:, None] + rrow).clamp(max=M - 1)]
    pre = tile[:, :, :N]
    v = pre + R                                               # (acc + bias) + r
    src = pre if defect == "Y16 computed from the pre-residual value" else v
    C = N + 4 if defect == "mean taken over N + 4 (the tile's padding columns)" else N
    lanes = src.reshape(T, BM, CH, 16, 4).permute(0, 1, 3, 2, 4).reshape(T, BM, 16, CH * 4)     # a lane's elements in its order
    x16 = torch.arange(16)

    def across(t):                                            # xor-shuffles, widest first
        for o in (8, 4, 2, 1):
            t = t + t[..., x16 ^ o]
        return t
    s = torch.zeros(T, BM, 16, dtype=F32)
    for i in range(CH * 4):
        s = s + lanes[..., i]
    mean = across(s) / C
    d = lanes - mean[..., None]
    q = d[..., 1] * d[..., 1]
    q = _fma(d[..., 0], d[..., 0], q)
    for i in range(2, CH * 4):
        q = _fma(d[..., i], d[..., i], q)
    rstd = 1.0 / torch.sqrt(across(q) / C + torch.tensor(E["eps"], dtype=F32))
    g = E["ln_w"].to(F32).reshape(CH, 16, 4).permute(1, 0, 2).reshape(16, CH * 4)
    b = E["ln_b"].to(F32).reshape(CH, 16, 4).permute(1, 0, 2).reshape(16, CH * 4)
    yl = _fma(g.expand_as(d), rstd[..., None] * d, b.expand_as(d))
    y = yl.reshape(T, BM, 16, CH, 4).permute(0, 1, 3, 2, 4).reshape(T, BM, N).to(op16)
    keep = torch.ones_like(grow, dtype=torch.bool) if defect == "rows past M stored" else grow < M
    return grow[keep], v[keep], y[keep]


def verdict(rows, c32, y16, E, op16, whole=True):
    """what the GPU file would see of a restated run: "sentinel" (a store outside the outputs), "missing" (an output row never stored),
    "bits" (a stored row differs from the expected bits in C32 or Y16) or None"""
    M = E["M"]
    if bool((rows >= M).any()) or bool((rows < 0).any()):
        return "sentinel"
    if whole and sorted(rows.tolist()) != list(range(M)):
        return "missing"
    if not torch.equal(c32.view(torch.int32), E["x"].float()[rows].view(torch.int32)):
        return "bits"
    if not torch.equal(y16.view(torch.int16), E["y"].to(op16)[rows].view(torch.int16)):
        return "bits"
    return None
