"""Case tables, operand builders, exactness conditions, float64 references and simulated defects of the variant matrix of
patch_embed_kernel<NT,NTOK> and im2col_patch_kernel (csrc/conv.hip), conv3x3s2_mfma_kernel<CIN,COUT,WR,WC,SKINNY> (csrc/conv_mfma.hip) and
token_mlp3_kernel (csrc/conv.hip).

Plain torch, no GPU needed: tests/test_conv_variants_gpu.py runs the cases on the card (device="cuda"), tests/test_conv_cases_cpu.py proves
on the CPU that the builders and references do what the GPU file relies on and that every simulated defect fails its case.

Exact passes (values known to the bit in fp16 and in bf16, no kernel of the library in the expected value):
  patch embed  image integers (interior +-3, the three outermost rows and columns of every image +-4..7), dense weights in {+-1, +-2, +-3}
               drawn per (n, c, ky, kx), integer bias that steps with the 32-column tile, an integer position table whose rows all differ:
               every partial sum is an integer far below 2^24, the fp32 result is the float64 one in any order;
  conv         isolated impulses +-3 on a pitch-3 lattice (no 3 x 3 window holds two), dense +-1 weights whose columns are balanced and
               orthogonal to a balanced +-1 vector z, bias = c + 4 z: a patch with an impulse has pre = c +- 4 +- 3 (mean c, variance 25),
               one without has variance 16; ln_w in {+-20, +-40}, ln_b in 80..83 make every LayerNorm output an integer in [24, 139] up to
               2e-8 relative, where GELU is the identity: Y16 is that integer;
  token heads  hs integers in [-3, 3], 16 entries of +-1 per weight row, integer biases: integers through the three layers.
The restate functions walk the indices as the kernels do and take a `defect=` switch: every defect of PE_DEFECTS, CONV_DEFECTS and
TH_DEFECTS must change the exact pass's bits ("bits") or store where the output's sentinels are ("sentinel").
"""
import torch
import torch.nn.functional as Fn

from fused_cases import exact16, r16  # noqa: F401

F32 = torch.float32
F64 = torch.float64
GUARD = 64                                # NaN elements on either side of a flattened operand of a restatement


def cdiv(a, b):
    return (a + b - 1) // b


def _ri(g, device):
    return lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g, device=device).double()


def _guarded(t):
    """t flattened between GUARD NaNs: what a kernel reads at a flat index outside the tensor"""
    nan = torch.full((GUARD,), float("nan"), dtype=F64, device=t.device)
    return torch.cat([nan, t.double().flatten(), nan])


def _at(flat, idx):
    """flat[GUARD + idx], an index outside the guards reading NaN as well"""
    return flat[(idx + GUARD).clamp(0, flat.numel() - 1)]


def xcd_tile_order(idx, n):
    """common.h: workgroup idx of a launch of n -> tile index"""
    q, rem = n // 8, n % 8
    xcd = idx % 8
    return torch.where(xcd < rem, xcd * (q + 1), rem * (q + 1) + (xcd - rem) * q) + idx // 8


def frag_row(e, h):
    """common.h s_frag_key: accumulator register e of lane half h holds row (e & 3) + 8 (e >> 2) + 4 h of the 32 x 32 block"""
    return (e & 3) + 8 * (e >> 2) + 4 * h


# =================================================================================================================================
# 1. patch embedding
PE_GRID = 1024                            # msam2_patch_embed7x7s4: grid = min(n_seg, 1024)
IM2COL = "im2col_patch_kernel"


def pe_nt(E):
    return cdiv(E, 32)


def pe_ntok(S):
    So = S // 4
    return 128 if So % 128 == 0 else (64 if So % 64 == 0 else 32)


def PE(NT, NTOK):
    return f"patch_embed_kernel<{NT},{NTOK}>"


def pe_case(B, S, E, path):
    So, nt = S // 4, pe_ntok(S)
    n_seg = B * So * (So // nt)
    return dict(B=B, S=S, E=E, path=path, expect=PE(pe_nt(E), nt), n_seg=n_seg, per_row=So // nt, trips=cdiv(n_seg, PE_GRID),
                random=path == "small")


# E: NT = 1 (8: a partly used tile), 2 (33: one live column in the second tile), 3, 4 (97, 112: partly used fourth tile);
# S: NTOK = 32, 64, 128 with one segment per token row; B = 2: a batch seam
PE_SMALL = [pe_case(2, S, E, "small") for E in (8, 32, 33, 64, 96, 97, 112, 128) for S in (128, 256, 512)]
# three segments per token row: the middle one has a neighbour on both sides (smallest S per NTOK)
PE_INTERIOR = [pe_case(1, 384, 64, "interior"), pe_case(1, 768, 8, "interior"), pe_case(1, 1536, 128, "interior")]
# 1056, 1088, 1152 segments: a second trip of the grid-stride loop for some workgroups only; 2080: a third trip
PE_WRAP = [pe_case(33, 128, 96, "wrap"), pe_case(17, 256, 33, "wrap"), pe_case(9, 512, 128, "wrap"), pe_case(65, 128, 8, "wrap")]
# the product's own step: 2048 segments, exactly two trips for every workgroup
PE_PRODUCT = [pe_case(4, 1024, 96, "product"), pe_case(4, 1024, 112, "product")]
PE_CASES = PE_SMALL + PE_INTERIOR + PE_WRAP + PE_PRODUCT
# the fallback / weight-gradient input: So % 32 != 0, and one total above 16384 * 256 eight-column groups (the grid-stride loop wraps)
IM2COL_CASES = [dict(B=2, S=4), dict(B=2, S=36), dict(B=3, S=100), dict(B=1, S=1840)]
IM2COL_GRID = 16384 * 256


def pe_id(c):
    return f"{c['path']}-b{c['B']}-s{c['S']}-e{c['E']}"


def pe_instantiations():
    return sorted({c["expect"] for c in PE_CASES} | {IM2COL})


def pe_wperm(w):
    """[E, 3, 7, 7] -> [ceil32(E), 176]: k' = (c 7 + ky) 8 + 1 + kx, zero at k' % 8 == 0, in row 21 and in the padding rows
    (PatchEmbed._weight_perm's layout, restated)"""
    E = w.shape[0]
    wp = torch.zeros(cdiv(E, 32) * 32, 22, 8, dtype=w.dtype, device=w.device)
    wp[:E, :21, 1:] = w.reshape(E, 21, 7)
    return wp.reshape(-1, 176)


def conv_tokens(img, w, k, stride, pad):
    """float64 convolution as unfold + matmul, one image at a time: [B, C, H, W], [E, C, k, k] -> [B * Ho * Wo, E] (token-major)"""
    w2 = w.double().reshape(w.shape[0], -1)
    return torch.cat([(w2 @ Fn.unfold(img[b:b + 1].double(), k, padding=pad, stride=stride)[0]).t() for b in range(img.shape[0])])


def pe_exact(c, device="cpu"):
    B, S, E = c["B"], c["S"], c["E"]
    So = S // 4
    g = torch.Generator(device=device).manual_seed(77 + 1009 * S + 31 * E + B)
    ri = _ri(g, device)
    edge = torch.arange(S, device=device)
    edge = (edge < 3) | (edge >= S - 3)
    band = edge[:, None] | edge[None, :]
    img = torch.where(band, ri(4, 7, B, 3, S, S) * (ri(0, 1, B, 3, S, S) * 2 - 1), ri(-3, 3, B, 3, S, S))
    v = ri(0, 5, E, 3, 7, 7)
    w = torch.where(v < 3, v - 3, v - 2)                                 # {-3, -2, -1, 1, 2, 3}: dense
    j = torch.arange(E, device=device)
    bias = ((j + j // 32) % 5).double() - 2
    t = torch.arange(So * So, device=device)
    pos = ri(-8, 8, So * So, E)
    pos[:, 0], pos[:, 1], pos[:, 2] = (t % 64).double() - 32, (t // 64 % 64).double() - 32, (t // 4096).double() - 18
    # ---- the conditions the exact pass rests on
    assert bool((w != 0).all()) and torch.unique(w.reshape(E, -1), dim=0).shape[0] == E, "two channels share a weight pattern"
    assert torch.unique(w.reshape(E, 147).t(), dim=0).shape[0] == 147, "two taps share a weight pattern"
    assert bool(((pos[:, 0] + 32) + 64 * (pos[:, 1] + 32) + 4096 * (pos[:, 2] + 18) == t).all()), "two position rows are equal"
    assert exact16(w) and float(img.abs().max()) == 7 and float(img[:, :, 3:-3, 3:-3].abs().max()) <= 3
    assert float(img[:, :, :3].abs().min()) >= 4 and float(img[:, :, :, -3:].abs().min()) >= 4, "the border band has its own range"
    assert 147 * 7 * 3 + float(bias.abs().max()) + float(pos.abs().max()) < 2 ** 24, "every partial sum is an integer below 2^24"
    flat = img.reshape(B, -1)
    assert B == 1 or bool((flat[1:] != flat[:-1]).any(1).all()), "neighbouring images differ"
    pre = conv_tokens(img, w, 7, 4, 3) + bias
    assert float(pre.abs().max()) < 2 ** 24 and bool((pre == pre.round()).all())
    return dict(B=B, S=S, E=E, img=img, w=w, wp=pe_wperm(w), bias=bias, pos=pos, pre=pre, ref=pre + pos.repeat(B, 1))


def pe_random(c, op16, device="cpu"):
    """randn operands as tests/test_kernels_gpu.py::test_patch_embed_one_kernel builds them; float64 references of the operand-rounded
    inputs: pre = conv + bias, S = sum |a w| (error_bound's S), ref = pre + pos"""
    B, S, E = c["B"], c["S"], c["E"]
    g = torch.Generator().manual_seed(S + E)
    img = torch.randn(B, 3, S, S, generator=g)
    img[:, :, :5, :] *= 3.0
    img[:, :, :, -5:] -= 2.0
    w = torch.randn(E, 3, 7, 7, generator=g) * 0.1
    bias = torch.randn(E, generator=g)
    pos = torch.randn((S // 4) ** 2, E, generator=g)
    img, w, bias, pos = (x.to(device).double() for x in (img, w, bias, pos))
    img16, w16 = r16(img.float(), op16).double(), r16(w, op16)
    pre = conv_tokens(img16, w16, 7, 4, 3) + bias
    return dict(B=B, S=S, E=E, img=img, w=w16, wp=pe_wperm(w16), bias=bias, pos=pos, pre=pre, Sabs=conv_tokens(img16.abs(), w16.abs(), 7, 4, 3),
                ref=pre + pos.repeat(B, 1))


def swap_images(X, i, j):
    """the operands with images i and j exchanged in the batch"""
    perm = list(range(X["B"]))
    perm[i], perm[j] = j, i
    return dict(X, img=X["img"][perm])


# (the right and bottom padding never occur: the last staged column of a token row is pixel 4 (So - nt) - 4 + 4 nt + 3 = S - 1 and the last
# window row is 4 (So - 1) + 3 = S - 1, so `x < S` and `y < S` are dead tests and dropping them is no defect -- PE_DEAD_CHECKS; the live
# horizontal test is x >= 0)
PE_DEAD_CHECKS = ("x >= S not zeroed", "y >= S not zeroed")
PE_DEFECTS = ("the zero tap placed behind instead of in front", "a window starting at column 4 t + 4", "x < 0 not zeroed", "y < 0 not zeroed",
              "the position row taken with the batch offset", "a wave with 32 wave >= NTOK storing",
              "the second trip computed from the first trip's registers", "a channel n >= E stored", "the bias one 32-tile off",
              "the + 4 h dropped")


def pe_restate(X, op16, with_pos=True, defect=None, segs=None):
    """patch_embed_kernel's walk: segment -> staged (c, ky) rows whose column j is pixel 4 tx0 - 4 + j -> fragment k' = 8 R + e read at
    column 4 t + e -> token -> accumulator row (e & 3) + 8 (e >> 2) + 4 h -> store with bias and the position row of the token within its
    image.  Returns (out fp32 flat, written mask, number of stores outside the output, tokens of the walked segments)."""
    assert defect is None or defect in PE_DEFECTS + PE_DEAD_CHECKS
    B, S, E = X["B"], X["S"], X["E"]
    dev = X["img"].device
    So, nt, NT = S // 4, pe_ntok(S), pe_nt(E)
    spr = So // nt
    n_seg = B * So * spr
    grid = min(n_seg, PE_GRID)
    imgf = _guarded(r16(X["img"].float(), op16))
    posf = _guarded(X["pos"].float())
    wp = r16(X["wp"], op16).double()
    if defect == "the zero tap placed behind instead of in front":
        wp = torch.zeros(NT * 32, 22, 8, dtype=F64, device=dev)
        wp[:E, :21, :7] = r16(X["w"], op16).double().reshape(E, 21, 7)
        wp = wp.reshape(-1, 176)
    n_out = B * So * So * E
    out = torch.zeros(n_out, dtype=F32, device=dev)
    written = torch.zeros(n_out, dtype=torch.bool, device=dev)
    outside, mine = 0, []
    ar = lambda n: torch.arange(n, device=dev)
    rows = ar(21)
    cc, ky = rows // 7, rows % 7
    jj = ar(4 * nt + 4)
    waves = 4 if defect == "a wave with 32 wave >= NTOK storing" else nt // 32
    bias = torch.cat([X["bias"].double(), torch.zeros(NT * 32 - E, dtype=F64, device=dev)])
    for seg in (range(n_seg) if segs is None else segs):
        src = seg - grid if (defect == "the second trip computed from the first trip's registers" and seg >= grid) else seg
        sx, ty, b = src % spr, (src // spr) % So, src // (spr * So)
        y, x = (4 * ty - 3 + ky)[:, None], (4 * sx * nt - 4 + jj)[None, :]
        inb = torch.ones(21, 4 * nt + 4, dtype=torch.bool, device=dev)
        if defect != "x >= S not zeroed":
            inb = inb & (x < S)
        if defect != "y >= S not zeroed":
            inb = inb & (y < S)
        if defect != "x < 0 not zeroed":
            inb = inb & (x >= 0)
        if defect != "y < 0 not zeroed":
            inb = inb & (y >= 0)
        staged = torch.where(inb, _at(imgf, ((b * 3 + cc[:, None]) * S + y) * S + x), torch.zeros((), dtype=F64, device=dev))
        simg = torch.full((22, 4 * 128 + 16), float("nan"), dtype=F64, device=dev)      # LDS behind the staged columns: not this segment's
        simg[:21, :4 * nt + 4] = staged
        simg[21] = 0.0                                                                   # row 21 does not exist: zero fragment
        t = ar(32 * waves)
        col = 4 * t[:, None, None] + ar(8)[None, None, :] + (4 if defect == "a window starting at column 4 t + 4" else 0)
        A = simg[ar(22)[None, :, None], col].reshape(32 * waves, 176)
        acc = (A @ wp.t()).float()                                                       # [tokens of the segment, NT * 32]
        # ---- store, per (wave, tile j, lane half h, register e, lane r)
        sx, ty, b = seg % spr, (seg // spr) % So, seg // (spr * So)
        wv, j, h, e, r = torch.meshgrid(ar(waves), ar(NT), ar(2), ar(16), ar(32), indexing="ij")
        srow = frag_row(e, h)                                                            # the row the MFMA left in this register
        drow = frag_row(e, 0 if defect == "the + 4 h dropped" else h)
        n = 32 * j + r
        tok0 = (b * So + ty) * So + sx * nt + 32 * wv
        ptok0 = tok0 if defect == "the position row taken with the batch offset" else ty * So + sx * nt + 32 * wv
        nb = ((j + 1) % NT) * 32 + r if defect == "the bias one 32-tile off" else n
        val = acc[32 * wv + srow, n] + bias[nb].float()
        if with_pos:
            val = val + torch.where(n < E, _at(posf, (ptok0 + drow) * E + n), torch.zeros((), dtype=F64, device=dev)).float()
        live = torch.ones_like(n, dtype=torch.bool) if defect == "a channel n >= E stored" else n < E
        addr = ((tok0 + drow) * E + n)[live]
        val = val[live]
        ok = (addr >= 0) & (addr < n_out)
        outside += int((~ok).sum())
        out[addr[ok]] = val[ok]
        written[addr[ok]] = True
        first = (b * So + ty) * So + sx * nt
        mine.append(torch.arange(first, first + nt, device=dev))
    return out, written, outside, torch.cat(mine)


def pe_verdict(res, X, with_pos=True):
    """None when the walk gave the expected bits on its tokens and stored nowhere else; else "sentinel" (a store outside the output) or
    "bits" """
    out, written, outside, toks = res
    if outside:
        return "sentinel"
    want = (X["ref"] if with_pos else X["pre"]).float()
    E = X["E"]
    own = torch.zeros(want.shape[0], dtype=torch.bool, device=out.device)
    own[toks] = True
    w2, o2 = written.view(-1, E), out.view(-1, E)
    if bool(w2[~own].any()) or not bool(w2[own].all()):
        return "bits"
    return None if torch.equal(o2[own].view(torch.int32), want[own].view(torch.int32)) else "bits"


def im2col_restate(img, op16):
    """im2col_patch_kernel's map on the operand-rounded image: out[(b, yo, xo), col] = img[b, c, 4 yo - 3 + ky, 4 xo - 3 + kx] with
    col = c 49 + ky 7 + kx < 147, zero outside the image and in columns 147..159"""
    B, _, S, _ = img.shape
    dev = img.device
    So = S // 4
    i16 = img.float().to(op16)
    col = torch.arange(160, device=dev)
    c, k = (col // 49).clamp(max=2), col % 49
    ky, kx = k // 7, k % 7
    o = torch.arange(So, device=dev)
    y = (4 * o - 3)[:, None, None] + ky[None, None, :]                    # [yo, 1, col]
    x = (4 * o - 3)[None, :, None] + kx[None, None, :]                    # [1, xo, col]
    inb = (col < 147)[None, None, :] & (y >= 0) & (y < S) & (x >= 0) & (x < S)
    idx = (c[None, None, :] * S + y.clamp(0, S - 1)) * S + x.clamp(0, S - 1)
    out = torch.stack([i16[b].flatten()[idx] for b in range(B)])
    return torch.where(inb[None], out, torch.zeros((), dtype=op16, device=dev)).reshape(B * So * So, 160)


# =================================================================================================================================
# 2. implicit-GEMM convolution of the mask down-sampler
CONV_TILING = {4: (4, 1), 16: (4, 1), 64: (2, 4)}                        # CIN -> (WR, WC)
CONV_EPS = 1e-6
# (B, H, W): one pixel, every border tap dead; M = 30, 32, 33 around the M <= 32 dispatch edge; M = 1089: 9 workgroups at BM = 128, 18 at
# BM = 64 (xcd_tile_order with quotient and remainder), a ragged last tile, W / 2 odd
CONV_SHAPES = [(1, 2, 2), (2, 6, 10), (2, 8, 8), (1, 6, 22), (1, 66, 66)]
# exact cases per (CIN, shape): the small shapes are swept (lattice offset, channels, signs and c change with v) until every k of the
# instantiation has met an impulse -- a SKINNY launch has at most 32 patches, so at most 32 of its 9 CIN columns see one
CONV_SWEEP = {4: 3, 16: 12, 64: 42}


def conv_skinny(cin, M):
    return cin >= 16 and M <= 32                                          # ceil8(9 cin) % 16 == 0 at CIN = 16, 64 only


def CONV(cin, M):
    wr, wc = CONV_TILING[cin]
    return f"conv3x3s2_mfma_kernel<{cin},{4 * cin},{wr},{wc},{'true' if conv_skinny(cin, M) else 'false'}>"


def conv_M(B, H, W):
    return B * (H // 2) * (W // 2)


def conv_taps(y, x, H, W):
    """the (patch row, patch column, tap) triples that see input pixel (y, x)"""
    out = []
    for oy, ky in (((y // 2, 1),) if y % 2 == 0 else (((y - 1) // 2, 2), ((y + 1) // 2, 0))):
        for ox, kx in (((x // 2, 1),) if x % 2 == 0 else (((x - 1) // 2, 2), ((x + 1) // 2, 0))):
            if oy < H // 2 and ox < W // 2:
                out.append((oy, ox, ky * 3 + kx))
    return out


def _conv_plan():
    """the exact cases of every instantiation with their impulses (b, y, x, channel, sign): a lattice of pitch 3 whose offset changes with
    the case and the image; the channel of an impulse is the next one its least-covered tap has not met"""
    cases, ptr = [], {}
    for cin in (4, 16, 64):
        for si, (B, H, W) in enumerate(CONV_SHAPES):
            M = conv_M(B, H, W)
            key = CONV(cin, M)
            p = ptr.setdefault(key, [0] * 9)
            for v in range(1 if M > 64 else CONV_SWEEP[cin]):
                imp, i = [], 0
                for b in range(B):
                    a0, b0 = (v + si + b) % 3, ((v + si) // 3 + 2 * b) % 3
                    for y in range(a0, H, 3):
                        for x in range(b0, W, 3):
                            taps = [t for _, _, t in conv_taps(y, x, H, W)]
                            t0 = min(taps, key=lambda t: p[t])
                            imp.append((b, y, x, p[t0] % cin, 3 if (i + v) % 2 == 0 else -3))
                            p[t0] += 1
                            i += 1
                cases.append(dict(cin=cin, B=B, H=H, W=W, M=M, v=v, expect=key, impulses=imp, c=float((v + si) % 5 - 2)))
    return cases


CONV_EXACT = _conv_plan()
CONV_RANDOM = [dict(cin=cin, B=B, H=H, W=W, M=conv_M(B, H, W), expect=CONV(cin, conv_M(B, H, W))) for cin in (4, 16, 64) for B, H, W in CONV_SHAPES]


def conv_id(c):
    return f"c{c['cin']}-{c['B']}x{c['H']}x{c['W']}" + (f"-v{c['v']}" if "v" in c else "")


def conv_instantiations():
    return sorted({c["expect"] for c in CONV_EXACT})


def conv_z(cout, device="cpu"):
    """the fixed balanced +-1 vector"""
    n = torch.arange(cout, device=device)
    return 1.0 - 2.0 * ((n ^ (n >> 2) ^ (n >> 4)) & 1).double()


def conv_weights(cin, device="cpu"):
    """dense +-1 [COUT, 9 CIN], columns (ky, kx, c): every column balanced and orthogonal to z (so balanced on either sign of z), all distinct"""
    cout, K = 4 * cin, 9 * cin
    g = torch.Generator(device=device).manual_seed(4242 + cin)
    z = conv_z(cout, device)
    Wk = torch.empty(cout, K, dtype=F64, device=device)
    for _ in range(64):                                                  # (COUT = 16 has 4900 such columns: redraw until the 36 differ)
        for sign in (1.0, -1.0):
            half = (z == sign).nonzero().flatten()
            pick = torch.rand(K, cout // 2, generator=g, device=device).argsort(1) < cout // 4
            Wk[half] = (pick.double() * 2 - 1).t()
        if torch.unique(Wk.t(), dim=0).shape[0] == K:
            break
    assert bool((Wk.abs() == 1).all()) and bool((Wk.sum(0) == 0).all()) and bool(((Wk * z[:, None]).sum(0) == 0).all())
    assert torch.unique(Wk.t(), dim=0).shape[0] == K, "two columns of W are equal"
    assert float(z.sum()) == 0
    return Wk, z


def layernorm64(x, w, b, eps):
    d = x - x.mean(-1, keepdim=True)
    return d / torch.sqrt((d * d).mean(-1, keepdim=True) + eps) * w + b


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / 2.0 ** 0.5))


def conv_exact(c, device="cpu"):
    cin, B, H, W, M = c["cin"], c["B"], c["H"], c["W"], c["M"]
    cout, K = 4 * cin, 9 * cin
    KP = cdiv(K, 8) * 8
    g = torch.Generator(device=device).manual_seed(999 + 131 * cin + 17 * H + W + 7 * c["v"])
    ri = _ri(g, device)
    X = torch.zeros(B, H, W, cin, dtype=F64, device=device)
    imp = torch.tensor(c["impulses"], dtype=torch.long, device=device).reshape(-1, 5)      # (a one-pixel case whose lattice offset misses it has none)
    X[imp[:, 0], imp[:, 1], imp[:, 2], imp[:, 3]] = imp[:, 4].double()
    Wk, z = conv_weights(cin, device)
    Wp = torch.full((cout, KP + 8), float("nan"), dtype=F64, device=device)               # ldw = KP + 8, NaN beyond KP
    Wp[:, :KP] = 0.0                                                                     # columns 9 CIN .. KP are zero: the contract
    Wp[:, :K] = Wk
    bias = c["c"] + 4 * z
    ln_w = 20.0 * (ri(0, 1, cout) + 1) * (ri(0, 1, cout) * 2 - 1)                         # +-20, +-40
    ln_b = 80.0 + ri(0, 3, cout)
    # ---- expected values: float64, independent of the plan's bookkeeping
    cols = Fn.unfold(X.permute(0, 3, 1, 2), 3, padding=1, stride=2)                       # [B, cin * 9 (c, ky, kx), Ho * Wo]
    cols = cols.reshape(B, cin, 9, -1).permute(0, 3, 2, 1).reshape(M, K)                  # [M, (ky, kx, c)]
    assert int((cols != 0).sum(1).max()) <= 1, "a 3 x 3 window holds two impulses"
    pre = cols @ Wk.t() + bias
    hit = (cols != 0).any(1)
    var = ((pre - pre.mean(1, keepdim=True)) ** 2).sum(1) / cout
    assert bool((pre.mean(1) == c["c"]).all()) and bool((var[hit] == 25).all()) and bool((var[~hit] == 16).all())
    ln = layernorm64(pre, ln_w, ln_b, CONV_EPS)
    u = ln.round()
    assert float((ln - u).abs().max()) < 2e-6 and 10 <= float(u.min()) and float(u.max()) <= 153
    # GELU is the identity there: its own distance from u plus the 5e-5 csrc/common.h states for the polynomial form, and the LayerNorm's
    # 2e-8 relative, stay far below half an ulp of either 16-bit type at u (bf16 at [128, 256): 1 / 2)
    assert float((gelu64(u) - u).abs().max()) + 5e-5 + 2e-6 < 2.0 ** -5, "half an fp16 ulp at 128..256 is 2^-4, half a bf16 ulp at 16..32 is 2^-4"
    assert exact16(u) and exact16(X) and exact16(Wk)
    return dict(c, X=X, Wp=Wp, KP=KP, bias=bias, ln_w=ln_w, ln_b=ln_b, y=u, pre=pre, ks_hit=set((cols != 0).any(0).nonzero().flatten().tolist()),
                patches_hit=hit)


def conv_coverage(key):
    """(k's met by an impulse, facts about the impulses' places) over the exact cases of one instantiation"""
    ks, facts = set(), set()
    for c in CONV_EXACT:
        if c["expect"] != key:
            continue
        H, W, Ho, Wo = c["H"], c["W"], c["H"] // 2, c["W"] // 2
        last = set()
        for b, y, x, ch, s in c["impulses"]:
            seen = conv_taps(y, x, H, W)
            facts |= {f"sees{len(seen)}", "top" if y == 0 else "", "bottom" if y == H - 1 else "", "left" if x == 0 else "", "right" if x == W - 1 else ""}
            for oy, ox, t in seen:
                ks.add(t * c["cin"] + ch)
                if (oy, ox) == (Ho - 1, Wo - 1):
                    last.add(b)
                if (oy, ox) == (0, 0) and b - 1 in last:
                    facts.add("seam")                                                    # the last patch of image b - 1 and the first of image b
    return ks, facts - {""}


CONV_DEFECTS = ("ky and kx exchanged", "a window origin of 2 o instead of 2 o - 1", "a clamped border tap not zeroed", "b derived with Wo in place of Ho",
                "the two taps of a lane half exchanged at CIN = 4", "k >= 9 CIN not zeroed", "rows past M stored",
                "two column quarters exchanged at WC = 4")


def conv_restate(E, op16, defect=None):
    """conv3x3s2_mfma_kernel's walk: workgroup -> tile (xcd_tile_order) -> clamped pixel row -> load_a's tap / channel map for CIN = 4
    (two taps x four channels per lane half) and CIN >= 16, clamped loads zeroed outside, load_w's clamp and zero past KP -> bias ->
    LayerNorm in fp32 -> GELU -> the rows below M.  Returns (global rows stored, Y16 of those rows)."""
    assert defect is None or defect in CONV_DEFECTS
    cin, B, H, W, M, KP = E["cin"], E["B"], E["H"], E["W"], E["M"], E["KP"]
    dev = E["X"].device
    cout = 4 * cin
    WR, WC = CONV_TILING[cin]
    BM = 32 * WR
    nwg = cdiv(M, BM)
    KSTEPS = KP // 16 if conv_skinny(cin, M) else cdiv(KP, 32) * 2
    Ho, Wo = H // 2, W // 2
    Xf = _guarded(r16(E["X"], op16))
    wg = torch.arange(nwg, device=dev)
    grow = (xcd_tile_order(wg, nwg) * BM)[:, None] + torch.arange(BM, device=dev)[None, :]
    grow = grow.flatten()
    m = grow.clamp(max=M - 1)
    t1 = m // Wo
    ox = m - t1 * Wo
    D = Wo if defect == "b derived with Wo in place of Ho" else Ho
    b = t1 // D
    oy = t1 - b * D
    o = 0 if defect == "a window origin of 2 o instead of 2 o - 1" else 1
    y0, x0 = 2 * oy - o, 2 * ox - o
    k = torch.arange(KSTEPS * 16, device=dev)
    ks, h, e8 = k // 16, (k % 16) // 8, k % 8
    if cin >= 16:
        tap = (16 * ks) // cin
        ch = (16 * ks) % cin + 8 * h + e8
        tc = torch.where(tap < 9, tap, torch.zeros_like(tap))
    else:
        q = e8 // 4
        tap = 4 * ks + 2 * h + (1 - q if defect == "the two taps of a lane half exchanged at CIN = 4" else q)
        ch = e8 % 4
        tc = tap.clamp(max=8)
    ty, tx = tc // 3, tc % 3
    if defect == "ky and kx exchanged":
        ty, tx = tx, ty
    y, x = y0[:, None] + ty[None, :], x0[:, None] + tx[None, :]
    inside = (y >= 0) & (y < H) & (x >= 0) & (x < W)
    live = (tap < 9)[None, :].expand_as(inside)
    inb = live if defect == "a clamped border tap not zeroed" else (inside if defect == "k >= 9 CIN not zeroed" else inside & live)
    A = torch.where(inb, _at(Xf, ((b[:, None] * H + y.clamp(0, H - 1)) * W + x.clamp(0, W - 1)) * cin + ch[None, :]), torch.zeros((), dtype=F64, device=dev))
    k0 = 16 * ks + 8 * h
    Wm = r16(E["Wp"], op16)[:, k0.clamp(max=KP - 8) + e8]
    if defect != "k >= 9 CIN not zeroed":
        Wm = torch.where((k0 < KP)[None, :], Wm, torch.zeros((), dtype=F64, device=dev))
    if conv_skinny(cin, M):                                               # gemm_skinny_kernel's association: ((p0 + p1) + p2) + p3, then the bias
        per = cdiv(KSTEPS, 4) * 16
        acc = torch.zeros(A.shape[0], cout, dtype=F32, device=dev)
        for q in range(4):
            acc = acc + (A[:, q * per:(q + 1) * per] @ Wm[:, q * per:(q + 1) * per].t()).float()
        pre = acc + E["bias"].float()
    else:
        pre = (A @ Wm.t() + E["bias"]).float()
    if defect == "two column quarters exchanged at WC = 4" and WC == 4:
        pre = pre.view(-1, 4, cout // 4)[:, [1, 0, 3, 2]].reshape(-1, cout)
    mean = pre.sum(1, keepdim=True) / cout
    d = pre - mean
    rstd = 1.0 / torch.sqrt((d * d).sum(1, keepdim=True) / cout + torch.tensor(CONV_EPS, dtype=F32, device=dev))
    u = E["ln_w"].float() * (rstd * d) + E["ln_b"].float()
    y16 = gelu64(u.double()).float().to(op16)
    keep = torch.ones_like(grow, dtype=torch.bool) if defect == "rows past M stored" else grow < M
    return grow[keep], y16[keep]


def conv_verdict(rows, y16, E, op16):
    if bool((rows >= E["M"]).any()):
        return "sentinel"
    if sorted(rows.tolist()) != list(range(E["M"])):
        return "bits"
    want = E["y"].to(op16)[rows]
    return None if torch.equal(y16.view(torch.int16), want.view(torch.int16)) else "bits"


# =================================================================================================================================
# 3. the mask decoder's token heads
TH_G, TH_T, TH_C = 6, 9, 256
TH_OUT_DIM = (1, 4, 8, 9, 32, 256)       # the edges of the 8-row load groups and of a wave's 16 rows
TH_TOK = (5, 2, 7, 2, 0, 3)              # out of order, one repeat
TH_SIGMOID = (0, 1, 0, 1, 0, 0)
TH_B = (1, 3)
TH_HS_TS, TH_HS_PAD = TH_C + 8, 24       # hs token stride and extra batch stride: a strided view
TOKEN_MLP3 = "token_mlp3_kernel"


def th_instantiations():
    return [TOKEN_MLP3]


def th_packed_layout(B):
    """adjacent regions, head g's rows out_ld[g] = out_dim[g] + 3 apart, two sentinel elements behind every region -> (off, ld, total)"""
    off, ld, at = [], [], 0
    for od in TH_OUT_DIM:
        off.append(at)
        ld.append(od + 3)
        at += B * (od + 3) + 2
    return off, ld, at


def _th_weights(g, device, nnz=16):
    ri = _ri(g, device)
    place = torch.rand(TH_G, TH_C, TH_C, generator=g, device=device).argsort(2) < nnz
    return place.double() * (ri(0, 1, TH_G, TH_C, TH_C) * 2 - 1)


def th_reference(hs, Ws, bs):
    """float64 heads: [B, G, 256] outputs (sigmoid applied where flagged), plus the per-layer pre-activations"""
    x = hs[:, list(TH_TOK)]                                                              # [B, G, C]
    pres = []
    for layer in range(3):
        pre = torch.einsum("bgk,gok->bgo", x, Ws[layer]) + bs[layer]
        pres.append(pre)
        x = pre.clamp_min(0)
    sg = torch.tensor(TH_SIGMOID, device=hs.device, dtype=torch.bool)[None, :, None]
    return torch.where(sg, torch.sigmoid(pres[2]), pres[2]), pres


def th_exact(B, device="cpu"):
    g = torch.Generator(device=device).manual_seed(600 + B)
    ri = _ri(g, device)
    hs = ri(-3, 3, B, TH_T, TH_C)
    Ws = [_th_weights(g, device) for _ in range(3)]
    bs = [ri(-4, 4, TH_G, TH_C) + torch.arange(TH_G, device=device).double()[:, None] for _ in range(3)]
    for gi, od in enumerate(TH_OUT_DIM):
        Ws[2][gi, od:] = 0.0                                                             # the contract: w3 rows >= out_dim are zero
    for w in Ws[:2]:
        assert torch.unique(w.reshape(-1, TH_C), dim=0).shape[0] == TH_G * TH_C, "two rows or heads share a weight pattern"
    live3 = torch.cat([Ws[2][gi, :od] for gi, od in enumerate(TH_OUT_DIM)])
    assert torch.unique(live3, dim=0).shape[0] == sum(TH_OUT_DIM)
    assert all(bool((w.abs().sum(2)[w.abs().sum(2) > 0] == 16).all()) for w in Ws)
    assert all(bool((bs[i][a] != bs[i][b]).any()) for i in range(3) for a in range(TH_G) for b in range(a))
    ref, pres = th_reference(hs, Ws, bs)
    x = hs[:, list(TH_TOK)]
    for layer in range(3):
        S = torch.einsum("bgk,gok->bgo", x.abs(), Ws[layer].abs()) + bs[layer].abs()
        assert float(S.max()) < 2 ** 24 and bool((pres[layer] == pres[layer].round()).all()), "integers below 2^24 through every partial sum"
        if layer < 2:
            assert bool((pres[layer] > 0).any(2).all()) and bool((pres[layer] < 0).any(2).all()), "both signs before each ReLU"
        x = pres[layer].clamp_min(0)
    assert exact16(Ws[0]) and exact16(Ws[1]) and exact16(Ws[2])
    return dict(B=B, hs=hs, Ws=Ws, bs=bs, ref=ref, pres=pres)


def th_random(B, op16, device="cpu"):
    """randn operands as tests/test_kernels_gpu.py::test_token_mlp3 builds them (weights rounded to the operand type)"""
    g = torch.Generator().manual_seed(51 + B)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(device).double()
    hs = rnd(B, TH_T, TH_C).float().double()
    Ws = [r16(rnd(TH_G, TH_C, TH_C, scale=0.08), op16) for _ in range(3)]
    bs = [rnd(TH_G, TH_C).float().double() for _ in range(3)]
    for gi, od in enumerate(TH_OUT_DIM):
        Ws[2][gi, od:] = 0.0
    ref, pres = th_reference(hs, Ws, bs)
    return dict(B=B, hs=hs, Ws=Ws, bs=bs, ref=ref, pres=pres)


def th_bound(X, error_bound):
    """error_bound composed over the three layers: layer i's bound times sum |w| of layer i + 1 (ReLU's Lipschitz constant is 1) plus
    layer i + 1's own.  n_terms = 256: one rounding of each fp32 x 16-bit product and at most 255 additions on the way of a term (the
    inner-product bound gamma_256).  The sigmoid heads: the carried error times the sigmoid's 1/4."""
    x = X["hs"][:, list(TH_TOK)]
    carried = torch.zeros_like(x)
    for layer in range(3):
        W, pre = X["Ws"][layer], X["pres"][layer]
        S = torch.einsum("bgk,gok->bgo", x.abs(), W.abs())
        push = torch.einsum("bgk,gok->bgo", carried, W.abs())
        if layer < 2:
            x = pre.clamp_min(0)
            carried = error_bound(S, TH_C, pre, x, act=2) + push
    sg = torch.tensor(TH_SIGMOID, device=x.device, dtype=torch.bool)[None, :, None]
    plain = error_bound(S, TH_C, pre, X["ref"], act=0) + push
    sig = error_bound(S, TH_C, pre, X["ref"], act=3) + 0.25 * push
    return torch.where(sg, sig, plain)


TH_DEFECTS = ("another head's token", "layer-3 rows >= out_dim written", "a packed row stride of out_dim instead of out_ld",
              "the activation buffer parity exchanged")


def th_restate(X, packed, defect=None):
    """token_mlp3_kernel's walk: workgroup (g, b) -> act[0] = hs[b, tok[g]] -> per layer, wave w owns rows 16 w .. 16 w + 15 in two groups
    of eight, a group is loaded when its first row is below the layer's row count, a layer-3 row is stored when it is below out_dim ->
    plain [B, G, 256] or packed out[off[g] + b ld[g] + o].  Returns (out fp32 flat, written mask, may-write mask)."""
    assert defect is None or defect in TH_DEFECTS
    B, dev = X["B"], X["hs"].device
    off, ld, total = th_packed_layout(B)
    n = total if packed else B * TH_G * TH_C
    out = torch.zeros(n, dtype=F32, device=dev)
    written = torch.zeros(n, dtype=torch.bool, device=dev)
    allowed = torch.zeros(n, dtype=torch.bool, device=dev)
    o_all = torch.arange(TH_C, device=dev)
    sig = lambda s: 1.0 / (1.0 + torch.exp(-s))
    for gi in range(TH_G):
        od = TH_OUT_DIM[gi]
        for b in range(B):
            base = off[gi] + b * ld[gi] if packed else (b * TH_G + gi) * TH_C
            allowed[base:base + od] = True
            tok = TH_TOK[(gi + 1) % TH_G] if defect == "another head's token" else TH_TOK[gi]
            act = [X["hs"][b, tok].float(), torch.full((TH_C,), float("nan"), dtype=F32, device=dev)]
            for layer in range(3):
                src = layer & 1
                if defect == "the activation buffer parity exchanged" and layer == 2:
                    src ^= 1
                rows = od if layer == 2 else TH_C
                loaded = (o_all // 8 * 8) < rows                                         # `if (o0 >= rows) break` per group of eight
                s = (X["Ws"][layer][gi] @ act[src].double() + X["bs"][layer][gi]).float()
                if layer < 2:
                    nxt = act[(layer + 1) & 1].clone()
                    nxt[loaded] = s[loaded].clamp_min(0)
                    act[(layer + 1) & 1] = nxt
                else:
                    store = loaded if defect == "layer-3 rows >= out_dim written" else loaded & (o_all < od)
                    val = sig(s) if TH_SIGMOID[gi] else s
                    if packed and defect == "a packed row stride of out_dim instead of out_ld":
                        base = off[gi] + b * od
                    addr = base + o_all[store]
                    ok = addr < n
                    out[addr[ok]] = val[store][ok]
                    written[addr[ok]] = True
    return out, written, allowed


def th_expected(X, packed):
    """(flat float64 expectation, may-write mask) of the plain or packed output"""
    B, dev = X["B"], X["hs"].device
    off, ld, total = th_packed_layout(B)
    n = total if packed else B * TH_G * TH_C
    want = torch.zeros(n, dtype=F64, device=dev)
    allowed = torch.zeros(n, dtype=torch.bool, device=dev)
    for gi, od in enumerate(TH_OUT_DIM):
        for b in range(B):
            base = off[gi] + b * ld[gi] if packed else (b * TH_G + gi) * TH_C
            want[base:base + od] = X["ref"][b, gi, :od]
            allowed[base:base + od] = True
    return want, allowed


def th_verdict(res, X, packed, tol=1e-6):
    """"sentinel": a store where the output must keep its sentinel; "bits": a head without sigmoid differs in its bits, or a sigmoid head
    lies further than `tol` from the float64 sigmoid of the exact integer, or a value was not written"""
    out, written, _ = res
    want, allowed = th_expected(X, packed)
    if bool((written & ~allowed).any()):
        return "sentinel"
    if not bool(written[allowed].all()):
        return "bits"
    d = (out.double() - want).abs()[allowed]
    exact = torch.ones_like(want, dtype=torch.bool)
    off, ld, _ = th_packed_layout(X["B"])
    for gi, od in enumerate(TH_OUT_DIM):
        if TH_SIGMOID[gi]:
            for b in range(X["B"]):
                base = off[gi] + b * ld[gi] if packed else (b * TH_G + gi) * TH_C
                exact[base:base + od] = False
    lim = torch.where(exact, torch.zeros_like(want), torch.full_like(want, tol))[allowed]
    return None if bool((d <= lim).all()) else "bits"
