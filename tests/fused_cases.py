"""Case tables, operand builders, float64 references, exactness conditions and simulated defects of the variant matrix of the Hiera
stage 1-2 fused kernels: attn_winproj_kernel (csrc/attn_winproj.hip) and mlp_fused_kernel / mlp_fused384_kernel (csrc/mlp_fused.hip).

Plain torch, no GPU needed: tests/test_fused_variants_gpu.py runs the cases on the card (device="cuda"), tests/test_fused_cases_cpu.py
proves on the CPU that the builders and references do what the GPU file relies on.

Two passes per case:
  exact   operands built so that a correct kernel's output is known to the bit in fp16 and in bf16 (no tolerance):
          * window attention: every query SELECTS its keys.  Token t of a window carries a 1 in input channel chan[t], the bits of the
            global window index sit in channels chan[ws^2 + j]; Wk maps token t to C_SEL e_t, Wq to C_SEL e_pi(t), Wv to the one-hot of
            the token (7 h places on in head h, so that no two heads share a v slab) plus its window's bits.  The selected score exceeds every other by C_SEL^2 96^-0.5 log2(e) ~ 603 in the log2 domain,
            so every other probability is exactly 0 in fp32 and out[t] = v[pi(t)] (pooled: the mean of four v rows, multiples of 1/4);
          * MLP: x = m + a s (s balanced +-1, a a power of two, m a small integer) has an exact mean and variance, the normalised row
            s g + b rounds to small integers, W1 / W2 are {-1, 0, 1}, every hidden pre-activation is an integer in [8, 255] where GELU is
            the identity far below half a 16-bit ulp, and out = x + h W2^T + b2 is an exact fp32 value.
  random  randn operands against a float64 reference of the operand-rounded inputs: attention inside attention_error_bound() widened by
          the one-ulp uncertainty of the rounded q | k | v (the kernel rounds an fp32 sum, the reference a float64 sum) AND inside the
          project's 0.02 + 0.01 |ref|; the MLP inside the project's own statement (tests/test_kernels_gpu.py::test_ln_mlp_residual_fused).
"""
import math
import os

import torch

import attention_cases as AC

LOG2E = 1.4426950408889634
HD = 96                         # head dim of every built form
C_SEL = 64.0                    # the selection constant: k_t = C_SEL e_t, q_t = C_SEL e_pi(t)
NWV = 8                         # waves = units per pass of attn_winproj_kernel
GRID = 256                      # both kernels cap their grid at 256 persistent workgroups
WAVES4 = os.environ.get("MSAM2_MLP_WAVES4", "")[:1] == "1"     # read once per process by the library: the plain entry's 4-wave forms


def r16(t, op16):
    return t.to(op16).to(t.dtype)


def exact16(t):
    """every element survives a round trip through fp16 and through bf16"""
    d = t.double()
    return bool((d.to(torch.float16).double() == d).all()) and bool((d.to(torch.bfloat16).double() == d).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# kernel keys (helpers.kernel_key spelling) and the case tables
def WINPROJ(dim, pool):
    return f"attn_winproj_kernel<{dim},{8 if dim == 96 else 4},{'true' if pool else 'false'},{'false' if dim == 96 else 'true'},8>"


def MLP(dim, waves4=False):
    if dim == 384:
        return "mlp_fused384_kernel"
    hc, tb = (192, 2) if dim == 96 else (96, 1)
    return f"mlp_fused_kernel<{dim},{hc},{2 * tb},1,4,false,0>" if waves4 else f"mlp_fused_kernel<{dim},{hc},{tb},1,8,false,0>"


def PROJ(dim, side):
    hc, tb = (192, 2) if dim == 96 else (96, 1)
    return f"mlp_fused_kernel<{dim},{hc},{tb},1,8,true,{side}>"


def attn(dim, heads, pool, B, H, W):
    ws = 8 if dim == 96 else 4
    nw = (H // ws) * (W // ws)
    return dict(dim=dim, heads=heads, ws=ws, pool=pool, B=B, H=H, W=W, nw=nw, units=B * nw if ws == 8 else B * nw // 2, expect=WINPROJ(dim, pool))


# (B, H, W): a unit is one 8 x 8 window or two 4 x 4 windows, 8 units per pass, 256 workgroups.
#   dim 96: one unit (seven clamped waves); three windows in a row; 18 units (ragged third pass); 2112 units (the grid wraps: a second pass
#   over resident weights).  dim 192: one unit; 6 windows in rows of 3 (the middle pair straddles two window rows); 9 units (ragged second
#   pass); 2176 units (the grid wraps; with 1 / 3 heads a pass consumes 3 / 9 slabs and the second pass starts in the other ring slot).
ATTN_CASES = ([attn(96, h, p, *s) for h in (1, 2) for p in (False, True) for s in ((1, 8, 8), (1, 8, 24), (3, 16, 24), (33, 64, 64))]
              + [attn(192, h, p, 1, 4, 8) for h in (1, 2, 3, 4, 8) for p in (False, True)]
              + [attn(192, h, p, *s) for h in (2, 3) for p in (False, True) for s in ((1, 8, 12), (3, 8, 12))]
              + [attn(192, h, p, 17, 64, 64) for h in (1, 2, 3) for p in (False, True)])
# what msam2_window_qkv_attention_supported refuses: (dim, heads, ws, pool, H, W)
ATTN_REFUSED = [(96, 1, 8, False, 20, 16), (192, 2, 4, False, 8, 10),      # windows that do not tile
                (192, 2, 4, False, 12, 12),                                 # 9 windows of 4 x 4: no pairs
                (192, 2, 4, False, 4, 4),                                   # one window
                (96, 1, 8, True, 9, 16),                                    # odd H with pool
                (96, 3, 8, False, 16, 16), (192, 9, 4, False, 8, 8), (192, 2, 8, False, 16, 16), (96, 1, 4, False, 8, 8)]

PASS = {96: 512, 192: 256}      # tokens of one pass of a workgroup, 8-wave and 4-wave forms alike (8 x TB x 32 = 4 x 2 TB x 32)


def token_counts(dim):
    if dim == 384:               # no persistence: one workgroup per 64 tokens
        return [1, 63, 65, 229]
    p = PASS[dim]
    return [1, 31, 33, p - 1, p + 1, 3 * p + 17, GRID * p + p // 2 + 5]     # the last one wraps the grid: a second pass, ragged


def mlp(form, dim, T, side=0):
    """form: "plain" (msam2_ln_mlp_residual_fwd), "dual" (_fwd_dual: + out16), "proj" (msam2_proj_ln_mlp_residual_fwd; side bit 0 out16,
    bit 1 xn16)"""
    expect = PROJ(dim, side) if form == "proj" else MLP(dim, WAVES4)
    return dict(form=form, dim=dim, T=T, side=side, expect=expect)


MLP_CASES = ([mlp(f, dim, T) for dim in (96, 192) for f in ("plain", "dual", "proj") for T in token_counts(dim)]
             + [mlp("proj", dim, T, side) for dim in (96, 192) for side in (1, 2, 3) for T in (31, 3 * PASS[dim] + 17, token_counts(dim)[-1])]
             + [mlp(f, 384, T) for f in ("plain", "dual") for T in token_counts(384)])


def attn_id(c):
    return f"attn-d{c['dim']}-h{c['heads']}{'-pool' if c['pool'] else ''}-{c['B']}x{c['H']}x{c['W']}"


def mlp_id(c):
    return f"{c['form']}-d{c['dim']}-T{c['T']}" + (f"-side{c['side']}" if c["form"] == "proj" else "")


def instantiations():
    """every kernel instantiation the tables reach in this process or, for the 4-wave forms, in the child process of the GPU file"""
    return sorted({c["expect"] for c in ATTN_CASES} | {c["expect"] for c in MLP_CASES} | {MLP(96, True), MLP(192, True), MLP(96), MLP(192)})


# ---------------------------------------------------------------------------------------------------------------------------------
# window <-> token-image forms
def to_windows(img, ws):
    """[B, H, W, ...] -> [B * nw, ws * ws, ...], windows row-major inside an image, tokens row-major inside a window"""
    B, H, W = img.shape[:3]
    rest = img.shape[3:]
    k = len(rest)
    t = img.reshape(B, H // ws, ws, W // ws, ws, *rest).permute(0, 1, 3, 2, 4, *range(5, 5 + k))
    return t.reshape(B * (H // ws) * (W // ws), ws * ws, *rest)


def from_windows(win, B, H, W, ws):
    """the inverse: [B * nw, ws * ws, C] -> [B * H * W, C]"""
    C = win.shape[-1]
    t = win.reshape(B, H // ws, W // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5)
    return t.reshape(B * H * W, C)


def out_geometry(c):
    """(Hq, Wq, wq): the output token image and its window size"""
    return (c["H"] // 2, c["W"] // 2, c["ws"] // 2) if c["pool"] else (c["H"], c["W"], c["ws"])


def head_perm(c, head):
    """pi of a head: a seeded permutation of the window's tokens that is no involution (q / k exchanged selects pi^-1 != pi)"""
    n = c["ws"] ** 2
    g = torch.Generator().manual_seed(4000 + 31 * c["dim"] + head)
    while True:
        p = torch.randperm(n, generator=g)
        if bool((p[p] != torch.arange(n)).any()) and bool((p != torch.arange(n)).all()):
            return p


def attn_exact(c, device="cpu"):
    """(xn [T, dim], w [3 * heads * 96, dim], bias [3 * heads * 96], expected [Tq, heads * 96]) in float64, all exact in fp16 and bf16"""
    dim, heads, ws, B, H, W = c["dim"], c["heads"], c["ws"], c["B"], c["H"], c["W"]
    n, Bw = ws * ws, B * c["nw"]
    nb = max(1, (Bw - 1).bit_length())
    assert n + nb <= HD and n + nb <= dim and nb <= 13, "token one-hot + window bits fit the head and the input row"
    chan = torch.randperm(dim, generator=torch.Generator().manual_seed(77 + dim)).to(device)      # every k-step of the projection carries signal
    ar = lambda k: torch.arange(k, device=device)
    g = ar(Bw)
    bits = ((g[:, None] >> ar(nb)) & 1).double()                         # [Bw, nb]
    xw = torch.zeros(Bw, n, dim, dtype=torch.float64, device=device)
    xw[:, ar(n), chan[:n]] = 1.0
    xw[:, :, chan[n:n + nb]] = bits[:, None, :]
    xn = from_windows(xw, B, H, W, ws)
    w = torch.zeros(3, heads, HD, dim, dtype=torch.float64, device=device)
    gb = torch.Generator().manual_seed(99 + dim + heads)
    bias = torch.zeros(3, heads, HD, dtype=torch.float64)
    bias[0] = ((torch.arange(heads) % 3) - 1.0)[:, None]                   # q: one constant per head (shifts all of a query's scores alike)
    bias[1] = torch.randint(-3, 4, (heads, HD), generator=gb).double()     # k: any small integers (likewise)
    bias[2] = torch.randint(-3, 4, (heads, HD), generator=gb).double()
    bias = bias.to(device)
    Hq, Wq, wq = out_geometry(c)
    outs = []
    for h in range(heads):
        pi = head_perm(c, h).to(device)
        w[1, h, ar(n), chan[:n]] = C_SEL
        w[0, h, pi, chan[:n]] = C_SEL
        rot = (ar(n) + 7 * h) % n                 # head h's one-hot sits 7 h places on: no two heads share a v slab
        w[2, h, rot, chan[:n]] = 1.0
        w[2, h, n + ar(nb), chan[n:n + nb]] = 1.0
        v = torch.zeros(Bw, n, HD, dtype=torch.float64, device=device)     # v row of token j of window g: e_rot(j) + bits(g) + bias
        v[:, ar(n), rot] = 1.0
        v[:, :, n:n + nb] = bits[:, None, :]
        v = v + bias[2, h]
        sel = v[:, pi]                                                     # [Bw, n, 96]: query t takes v[pi(t)]
        if c["pool"]:                                                      # four keys with equal scores: the mean of four v rows
            s4 = sel.reshape(Bw, ws // 2, 2, ws // 2, 2, HD)
            pis = pi.reshape(ws // 2, 2, ws // 2, 2).permute(0, 2, 1, 3).reshape(-1, 4)
            assert all(len(set(q.tolist())) == 4 for q in pis), "the four selected keys of a pooled query are distinct"
            sel = s4.sum(dim=(2, 4)).reshape(Bw, wq * wq, HD) / 4.0
        outs.append(sel)
    expected = from_windows(torch.cat(outs, dim=-1), B, Hq, Wq, wq)
    return xn, w.reshape(3 * heads * HD, dim), bias.reshape(-1), expected


def attn_random(c, op16, device="cpu"):
    """randn operands rounded to the operand type (float64 holders): xn, w, bias (fp32 values)"""
    g = torch.Generator(device=device).manual_seed(500 + c["dim"] + 7 * c["heads"] + c["H"] * c["W"] + c["B"])
    T = c["B"] * c["H"] * c["W"]
    xn = torch.randn(T, c["dim"], generator=g, device=device)
    w = torch.randn(3 * c["heads"] * HD, c["dim"], generator=g, device=device) * c["dim"] ** -0.5
    b = torch.randn(3 * c["heads"] * HD, generator=g, device=device) * 0.5
    return xn.to(op16).double(), w.to(op16).double(), b.double()


def attn_reference(c, xn, w, bias, op16):
    """float64 reference on the operand-rounded inputs (q | k | v rounded where the kernel rounds them) and its element-wise bound:
    attention_error_bound() with the score error widened by c smax (4 u16 + 4 u16^2) -- every q and k element within one 16-bit ulp,
    2 u16 relative, of the reference's -- and 2 u16 A more for v"""
    heads, ws, B, H, W = c["heads"], c["ws"], c["B"], c["H"], c["W"]
    fp16 = op16 == torch.float16
    qkv = r16(xn @ w.T + bias, op16)
    win = to_windows(qkv.reshape(B, H, W, 3, heads, HD), ws)               # [Bw, n, 3, heads, 96]
    Bw, n = win.shape[:2]
    q, k, v = (win[:, :, i].permute(0, 2, 1, 3) for i in range(3))         # [Bw, heads, n, 96]
    Hq, Wq, wq = out_geometry(c)
    if c["pool"]:
        q = q.reshape(Bw, heads, wq, 2, wq, 2, HD).amax(dim=(3, 5)).reshape(Bw, heads, wq * wq, HD)
    cc = LOG2E / math.sqrt(HD)
    ref, A, smax, _ = AC.reference(q, k, v, cc)
    h = AC.u16(fp16)
    ds = AC.score_error(smax, HD, cc, fp16, False) + cc * smax * (4 * h + 4 * h * h)
    e = torch.expm1(2 * math.log(2.0) * ds) * A + h * A + (n + 8) * AC.U * A + 2 * h * A
    bound = e + h * (ref.abs() + e) + 2.0 ** -25
    back = lambda t: from_windows(t.permute(0, 2, 1, 3).reshape(Bw, wq * wq, heads * HD), B, Hq, Wq, wq)
    return back(ref), back(bound)


KEY_SWAP = torch.tensor([j + 4 if (j & 12) == 4 else j - 4 if (j & 12) == 8 else j for j in range(64)])    # keys 4..7 <-> 8..11 of every 16

ATTN_DEFECTS = ["keys 4..7 and 8..11 of a block exchanged", "the two windows of a 4 x 4 pair exchanged", "block-diagonal mask of the pair dropped",
                "nwx taken for windows per column", "pooled query from the quad's first token", "q and k slabs exchanged",
                "head h reads head h ^ 1's v slab", "second pass reads every slab from the other ring slot", "a clamped wave's rows stored"]


def attn_restate(c, xn, w, bias, op16, units=None, defect=None, fma=True, order=0):
    """attn_winproj_kernel restated in fp32 on the CPU, unit by unit as the kernel walks them (lane -> token map, rounding points, exp2
    with the folded scale, 16-bit P, normalisation in the store).  Returns (rows, values): the output rows the kernel stores -- as indices
    into the [Tq, heads * 96] output, possibly past its end for a defect -- and their 16-bit values.  order: another contraction order
    of every sum; fma: the exponent's multiply-add fused (the kernel) or in two roundings."""
    dim, heads, ws, pool, B, H, W, nw = c["dim"], c["heads"], c["ws"], c["pool"], c["B"], c["H"], c["W"], c["nw"]
    f32 = torch.float32
    xn, w3, b3 = xn.to(f32), w.to(f32).reshape(3, heads, HD, dim), bias.to(f32).reshape(3, heads, HD)
    NB = 2 if ws == 8 else 1
    L = NB * 32
    nwx = (H // ws) if defect == "nwx taken for windows per column" else (W // ws)
    n_units, T = c["units"], B * H * W
    n_pass = (n_units + NWV - 1) // NWV
    U_raw = torch.arange(n_pass * NWV) if units is None else torch.as_tensor(units)
    live = U_raw < n_units
    if defect != "a clamped wave's rows stored":
        U_raw = U_raw[live]
        live = live[live]
    U = torch.where(live, U_raw, torch.full_like(U_raw, n_units - 1))

    def lane_map(Uu, swap_pair=False):
        r = torch.arange(32)[None, None, :]
        tb = torch.arange(NB)[None, :, None]
        py = px = torch.zeros(1, 1, 1, dtype=torch.long)
        if ws == 8:
            win = Uu[:, None, None] + 0 * r
            if pool:
                pq = tb * 8 + (r >> 2)
                py, px = pq >> 2, pq & 3
                ty, tx = 2 * py + ((r >> 1) & 1), 2 * px + (r & 1)
            else:
                t = tb * 32 + r
                ty, tx = t >> 3, t & 7
        else:
            win = 2 * Uu[:, None, None] + ((1 - (r >> 4)) if swap_pair else (r >> 4))
            if pool:
                qd = (r >> 2) & 3
                py, px = qd >> 1, qd & 1
                ty, tx = 2 * py + ((r >> 1) & 1), 2 * px + (r & 1)
            else:
                t = r & 15
                ty, tx = t >> 2, t & 3
        b = win // nw
        wi = win - b * nw
        wy = wi // nwx
        wx = wi - wy * nwx
        tok = (b * H + wy * ws + ty) * W + wx * ws + tx
        otok = ((b * (H // 2) + wy * (ws // 2) + py) * (W // 2) + wx * (ws // 2) + px) if pool else tok
        return tok.reshape(len(Uu), L), otok.reshape(len(Uu), L)

    tok, _ = lane_map(U, swap_pair=defect == "the two windows of a 4 x 4 pair exchanged")
    _, otok = lane_map(U_raw if defect == "a clamped wave's rows stored" else U)
    X = xn[tok % T]                                                        # [n, L, dim]
    kp = torch.randperm(dim, generator=torch.Generator().manual_seed(5)) if order else torch.arange(dim)
    jp = torch.randperm(L, generator=torch.Generator().manual_seed(6)) if order else torch.arange(L)
    sc = torch.tensor((1.0 / math.sqrt(HD)), dtype=f32) * torch.tensor(1.4426950408889634, dtype=f32)    # scale * log2(e) as the host folds it
    second = (U_raw // NWV) >= GRID                                        # units of a workgroup's second pass
    lane = torch.arange(L)
    outs = []
    for h in range(heads):
        def slab(i, hh=h):                                                 # ring step 3 hh + (0 k, 1 q, 2 v) -> (weight rows, bias)
            return w3[(1, 0, 2)[i], hh]
        wk, wq_, wv = slab(0), slab(1), slab(2)
        bk, bq, bv = b3[1, h], b3[0, h], b3[2, h]
        if defect == "q and k slabs exchanged":
            wk, wq_ = wq_, wk
        if defect == "head h reads head h ^ 1's v slab" and (h ^ 1) < heads:
            wv = w3[2, h ^ 1]
        proj = lambda Wm: X[:, :, kp] @ Wm[:, kp].T

        def qkv_of(wk, wq_, wv):
            k = r16(proj(wk) + bk, op16)
            q = proj(wq_)
            if pool:
                q4 = q.reshape(-1, L // 4, 4, HD)
                q = (q4[:, :, :1] if defect == "pooled query from the quad's first token" else q4.amax(2, keepdim=True)).expand_as(q4).reshape(-1, L, HD)
            return r16(q + bq, op16), k, r16(proj(wv) + bv, op16)
        q, k, v = qkv_of(wk, wq_, wv)
        if defect == "second pass reads every slab from the other ring slot" and dim == 192 and bool(second.any()):
            prev_v = w3[2, h - 1] if h > 0 else w3[2, heads - 1]           # the slab of one step earlier
            q2, k2, v2 = qkv_of(prev_v, slab(0), slab(1))
            m = second[:, None, None]
            q, k, v = torch.where(m, q2, q), torch.where(m, k2, k), torch.where(m, v2, v)
        S = q @ k.transpose(1, 2)                                          # [n, query, key]; all-integer in the exact pass
        if ws == 4 and defect != "block-diagonal mask of the pair dropped":
            S = S.masked_fill((lane[:, None] >> 4) != (lane[None, :] >> 4), -float("inf"))
        mx = S.amax(-1, keepdim=True) * sc
        arg = (S.double() * sc.double() - mx.double()).to(f32) if fma else (S * sc - mx)
        pe = torch.exp2(arg)
        inv = 1.0 / pe[:, :, jp].sum(-1, keepdim=True)
        vv = v[:, KEY_SWAP[:L]] if defect == "keys 4..7 and 8..11 of a block exchanged" else v
        o = (r16(pe, op16)[:, :, jp] @ vv[:, jp]) * inv
        outs.append(o.to(op16))
    vals = torch.cat(outs, dim=-1)                                         # [n, L, heads * 96]
    keep = torch.ones(L, dtype=torch.bool) if not pool else (lane & 3) == 0
    return otok[:, keep].reshape(-1), vals[:, keep].reshape(-1, heads * HD)


def attn_verdict(rows, vals, expected16):
    """what the GPU file would see of a restated run: "sentinel" (a store outside the output), "bits" (a stored row differs from the
    expected bits), "missing" (an output row never stored) or None"""
    Tq = expected16.shape[0]
    if bool((rows >= Tq).any()) or bool((rows < 0).any()):
        return "sentinel"
    if not torch.equal(vals.view(torch.int16), expected16[rows].view(torch.int16)):
        return "bits"
    return None


# ---------------------------------------------------------------------------------------------------------------------------------
# MLP
def w1_order(dim):
    """the in-block permutation of msam2_mlp_fused_permute_w1 / _w2 (dim 96 / 192): permuted[..., i] = w[..., src[i]]"""
    i = torch.arange(dim)
    q = i & 31
    s, h, j = q >> 4, (q >> 3) & 1, q & 7
    return (i & ~31) + 16 * s + 8 * (j >> 2) + 4 * h + (j & 3)


def _sparse_signs(rows, cols, nnz, g, device):
    """[rows, cols] with exactly nnz entries of +-1 per row"""
    idx = torch.rand(rows, cols, generator=g, device=device).argsort(1)[:, :nnz]
    sg = torch.randint(0, 2, (rows, nnz), generator=g, device=device).double() * 2 - 1
    return torch.zeros(rows, cols, dtype=torch.float64, device=device).scatter_(1, idx, sg)


_MLP_W = {}


def mlp_exact_weights(dim, device="cpu"):
    key = (dim, str(device))
    if key not in _MLP_W:
        g = torch.Generator(device=device).manual_seed(300 + dim)
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g, device=device).double()
        P = {"ln_w": (2 * ri(0, 1, dim) - 1) * ri(1, 2, dim), "ln_b": (2 * ri(0, 1, dim) - 1) * ri(4, 5, dim),
             "w1": _sparse_signs(4 * dim, dim, 12, g, device), "w2": _sparse_signs(dim, 4 * dim, 24, g, device), "b2": ri(-8, 8, dim),
             "wp": _sparse_signs(dim, dim, 8, g, device), "bp": ri(-3, 3, dim)}
        # |xn| <= 7 and 12 non-zeros per W1 row: |W1 xn| <= 84, every pre-activation an integer in [8, 179]
        # (the offset 0..3 also steps with the 32-block, so that no shift of b1 by whole blocks or chunks goes unseen)
        j = torch.arange(4 * dim, device=device)
        P["b1"] = 8.0 + 84.0 + ((j + j // 32) % 4).double()
        # the next norm1 of the PROJ form's xn16: |z| <= sqrt(dim - 1) for a normalised row, so with |g| <= 1 and |b| >= 16 the result has
        # magnitude >= 2 -- never near zero, where the 16-bit spacing falls below the fp32 error of a LayerNorm and "within one 16-bit
        # ulp of another fp32 evaluation" cannot hold (next_norm_reference); as ln_b keeps the first norm's rows away from 0
        P["nln_w"] = (2 * ri(0, 1, dim) - 1) * 0.5 * ri(1, 2, dim)
        P["nln_b"] = (2 * ri(0, 1, dim) - 1) * (12.0 + 4 * ri(1, 2, dim))
        assert float(P["nln_b"].abs().min()) - float(P["nln_w"].abs().max()) * math.sqrt(dim - 1) >= 2 or dim == 384
        _MLP_W[key] = P
    return _MLP_W[key]


def mlp_exact(dim, T, device="cpu"):
    """exact-pass operands and expected output of T tokens (float64 holders; exact in fp32, the weights and o in fp16 / bf16):
    x = m + a s is the MLP's input row -- the plain forms take it as x, the PROJ form as res + o Wp^T + bp with res = x - (o Wp^T + bp)"""
    P = dict(mlp_exact_weights(dim, device))
    g = torch.Generator(device=device).manual_seed(700 + dim + T)
    s = (torch.rand(T, dim, generator=g, device=device).argsort(1) < dim // 2).double() * 2 - 1           # balanced: half +1, half -1
    a = 2.0 ** torch.randint(-2, 3, (T, 1), generator=g, device=device).double()
    m = torch.randint(-3, 4, (T, 1), generator=g, device=device).double()
    x = m + a * s
    xn = s * P["ln_w"] + P["ln_b"]                                          # what the normalised row rounds to (rstd a = 1 - O(1e-5))
    hid = xn @ P["w1"].T + P["b1"]
    assert float(xn.abs().min()) >= 2 and float(xn.abs().max()) <= 7 and float(hid.min()) >= 8 and float(hid.max()) <= 255
    out = x + hid @ P["w2"].T + P["b2"]
    assert float(out.abs().max()) < 65504
    o = torch.randint(-2, 3, (T, dim), generator=g, device=device).double()
    P.update(x=x, hid=hid, out=out, o=o, res=x - (o @ P["wp"].T + P["bp"]))
    return P


_MLP_RW = {}


def mlp_random_weights(dim, op16, device="cpu"):
    key = (dim, op16, str(device))
    if key not in _MLP_RW:
        g = torch.Generator(device=device).manual_seed(900 + dim)
        rn = lambda *s: torch.randn(*s, generator=g, device=device)
        _MLP_RW[key] = {"wp": r16(rn(dim, dim) / dim ** 0.5, op16).double(), "bp": (0.1 * rn(dim)).double(),
                        "ln_w": (1 + 0.1 * rn(dim)).double(), "ln_b": (0.1 * rn(dim)).double(),
                        "w1": r16(rn(4 * dim, dim) / dim ** 0.5, op16).double(), "b1": (0.1 * rn(4 * dim)).double(),
                        "w2": r16(rn(dim, 4 * dim) / (4 * dim) ** 0.5, op16).double(), "b2": (0.1 * rn(dim)).double(),
                        "nln_w": (1 + 0.1 * rn(dim)).double(), "nln_b": (0.1 * rn(dim)).double()}
    return _MLP_RW[key]


def mlp_random(dim, T, op16, device="cpu"):
    """random-pass operands (float64 holders of fp32 / 16-bit values): rows of scale 1.5 around 0.3; row 1 has mean = 1000 std and the last
    row is constant (var = 0: the normalised row is beta), as ln_data of the pointwise matrix.  x is the MLP's input row; the PROJ form
    gets res = fp32(x - (o Wp^T + bp))."""
    P = dict(mlp_random_weights(dim, op16, device))
    g = torch.Generator(device=device).manual_seed(1100 + dim + T)
    x = torch.randn(T, dim, generator=g, device=device) * 1.5 + 0.3
    if T > 2:
        x[1] = 1000.0 + torch.randn(dim, generator=g, device=device)
    if T > 1:
        x[T - 1] = 2.0
    o = r16(0.5 * x.clamp(-8, 8) + torch.randn(T, dim, generator=g, device=device), op16).double()
    x = x.double()
    res = (x - (o @ P["wp"].T + P["bp"])).float().double()
    P.update(x=x, o=o, res=res, x1=res + o @ P["wp"].T + P["bp"])
    return P


def mlp_reference(P, proj, eps=1e-6):
    """float64: x1 + fc2(GELU(fc1(LayerNorm(x1)))) with x1 = x (plain) or res + o Wp^T + bp (PROJ)"""
    x1 = P["x1"] if proj else P["x"]
    mu = x1.mean(1, keepdim=True)
    var = ((x1 - mu) ** 2).mean(1, keepdim=True)
    xn = (x1 - mu) / torch.sqrt(var + eps) * P["ln_w"] + P["ln_b"]
    hp = xn @ P["w1"].T + P["b1"]
    return x1 + (0.5 * hp * (1 + torch.erf(hp / math.sqrt(2.0)))) @ P["w2"].T + P["b2"]


def next_norm_reference(rows32, g, b, eps, op16):
    """float64 LayerNorm of fp32 rows and the element-wise bound of a correct fp32 evaluation rounded to the operand type.  With n = dim,
    u = 2^-24, A = mean |x| of the row, r = (var + eps)^-1/2:
      * the computed mean is off by delta <= (n + 1) u A (any summation order, the multiplication by 1 / n);
      * sum (x - mean')^2 = sum (x - mean)^2 + n delta^2, and its n additions: r is off by the factor rho = (delta^2 r^2 + (n + 3) u) / 2 + 2 u;
      * (x - mean') r' g + b: |g| r (delta + |x - mean| (rho + 4 u)) + 2 u (|ref| + |b|);
      * the 16-bit rounding of the result: u16 (|ref| + the above) + half the fp16 subnormal spacing.
    Two correct evaluations can therefore be MORE than one 16-bit ulp apart: where the result cancels to near zero (the 16-bit spacing
    falls below the fp32 error) and on a row whose mean is many standard deviations (delta r is not small)."""
    x, g, b = rows32.double(), g.double(), b.double()
    n = x.shape[1]
    m = x.mean(1, keepdim=True)
    d = x - m
    r = 1.0 / torch.sqrt((d * d).mean(1, keepdim=True) + eps)
    ref = d * r * g + b
    delta = (n + 1) * AC.U * x.abs().mean(1, keepdim=True)
    rho = 0.5 * (delta ** 2 * r ** 2 + (n + 3) * AC.U) + 2 * AC.U
    e = g.abs() * r * (delta + d.abs() * (rho + 4 * AC.U)) + 2 * AC.U * (ref.abs() + b.abs())
    h = AC.u16(op16 == torch.float16)
    return ref, e + h * (ref.abs() + e) + 2.0 ** -25


MLP_DEFECTS = ["W2's hidden permutation omitted", "W1's input permutation omitted (PROJ)", "the two lane halves' channels exchanged",
               "chunk c computed with chunk c - 1's weights", "b1 offset by one 32-block", "bp added twice",
               "residual taken from the clamped row on a ragged pass", "out16 rounded from the pre-residual value"]


def _seqsum(v):
    return v.cumsum(1)[:, -1:]


def mlp_restate(P, dim, op16, proj, order=0, gelu_pert=0.0, defect=None, eps=1e-6):
    """the fused MLP restated in fp32 on the CPU with the kernel's rounding points (normalised row and hidden activation in the operand
    type).  order 1: the statistics summed per lane half and added across, contractions in the permuted operand order; gelu_pert: the
    activation moved by this many times (1e-5 relative + 5e-5 absolute).  Returns (out fp32, out16)."""
    f32 = torch.float32
    F = {k: v.to(f32) for k, v in P.items()}
    T = F["x"].shape[0]
    src = w1_order(dim)
    if proj:
        x1 = (F["res"] + F["bp"]) + F["o"] @ F["wp"].T
        if defect == "bp added twice":
            x1 = x1 + F["bp"]
    else:
        x1 = F["x"]
    halves = [torch.arange(dim)[((torch.arange(dim) >> 3) & 1) == h] for h in (0, 1)] if order else [torch.arange(dim)]
    tot = lambda v: sum(_seqsum(v[:, i]) for i in halves)
    mean = tot(x1) * torch.tensor(1.0 / dim, dtype=f32)
    d = x1 - mean
    rstd = 1.0 / torch.sqrt(tot(d * d) * torch.tensor(1.0 / dim, dtype=f32) + torch.tensor(eps, dtype=f32))
    xn = r16(d * rstd * F["ln_w"] + F["ln_b"], op16)
    if defect == "the two lane halves' channels exchanged":
        xn = xn[:, torch.arange(dim) ^ (4 if proj else 8)]
    if defect == "W1's input permutation omitted (PROJ)" and proj:
        xn = xn[:, src]
    w1, w2, b1 = F["w1"], F["w2"], F["b1"]
    if defect == "chunk c computed with chunk c - 1's weights":
        hc = {96: 192, 192: 96, 384: 32}[dim]
        w1, w2 = w1.roll(hc, 0), w2.roll(hc, 1)
    if defect == "b1 offset by one 32-block":
        b1 = b1.roll(32)
    kp = src if order else torch.arange(dim)
    hp = b1 + xn[:, kp] @ w1[:, kp].T
    act = 0.5 * hp * (1 + torch.erf(hp * torch.tensor(math.sqrt(0.5), dtype=f32)))
    act = act + gelu_pert * (1e-5 * act.abs() + 5e-5)
    hid = r16(act, op16)
    if defect == "W2's hidden permutation omitted":
        hid = hid[:, w1_order(4 * dim)]
    hperm = w1_order(4 * dim) if order else torch.arange(4 * dim)
    y = hid[:, hperm] @ w2[:, hperm].T
    resid = x1
    if defect == "residual taken from the clamped row on a ragged pass":
        p = {96: 512, 192: 256, 384: 64}[dim]
        last = torch.arange(T) >= (T - 1) // p * p
        resid = torch.where((last & (T % p != 0))[:, None], x1[T - 1:T].expand_as(x1), x1)
    out = (y + F["b2"]) + resid
    pre = out - resid if defect == "out16 rounded from the pre-residual value" else out
    return out, pre.to(op16)
