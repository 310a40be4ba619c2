"""Case tables, operand builders, float64 references, error bounds and simulated defects of the attention kernel-variant matrix.

Plain torch, no GPU needed: tests/test_attention_variants_gpu.py runs the cases on the card (device="cuda"), tests/test_attention_cases_cpu.py
proves on the CPU that the integer passes of every case can see the defects they are there for.

Every problem is held in one form, q [B, H, Lq, D], k [B, H, Lk, D], v [B, H, Lk, Dv] in float64 ("instances": batch x head; for the window
entry a batch element is one window, padded tokens included, whose K / V rows are the qkv bias).  The GPU file lays these out as the
entry point wants them (strided views, packed qkv, token images) and reads the result back into the same form.

The three passes (module docstring of tests/test_attention_variants_gpu.py has the why):
  selection  every query picks exactly one key: key j carries the +-1 code of its index in the first nb = bit_length(Lk - 1) channels, query
             i carries s times the code of its target t(i), s = ceil(GAP / (2 c)), c = log2(e) / sqrt(D).  score(i, t) - score(i, j) >= GAP
             bits for every other j, so the output is V[t(i)] to within Lk 2^-GAP; all operands are small integers (exact in fp16 / bf16).
  tie        the same with K[b] = K[a] for a list of pairs: queries that target a return (V[a] + V[b]) / 2.
  random     randn operands, bound attention_error_bound().
"""
import math
import os

import torch

LOG2E = 1.4426950408889634
GAP = 40                       # bits between the target's score and every other key's in the integer passes
U = 2.0 ** -24                 # fp32 unit round-off


def u16(fp16: bool) -> float:
    return 2.0 ** -11 if fp16 else 2.0 ** -8


# switches the library reads once per process: the GPU file runs their cases in child processes that have them set
G96_V1 = "MSAM2_G96_V1" in os.environ
G96_X2 = "MSAM2_G96_X2" in os.environ
KV64_V1 = "MSAM2_KV64_V1" in os.environ


# ---------------------------------------------------------------------------------------------------------------------------------
# kernel names (regular expressions on helpers.kernel_key)
def FWD(D, NW, win=False):
    return rf"attn_fwd_kernel<{D},{NW},{'true' if win else 'false'}>"


def MERGE(D):
    return rf"attn_merge_kernel<{D}>"


GLDS128, GLDS256, GLDS96 = r"attn_glds_kernel<128,128,4,2,false>", r"attn_glds_kernel<256,256,4,2,false>", r"attn_glds_kernel<96,128,4,3,false>"
G96X2_8, G96X2_4 = r"attn_g96x2_kernel<1,8>", r"attn_g96x2_kernel<2,4>"
KV64, KV64X2 = r"attn_kv64_kernel<4,3>", r"attn_kv64x2_kernel<4>"
WIN, TINY1, TINY2 = r"attn_win_kernel<96>", r"attn_tinywin_kernel<96,1>", r"attn_tinywin_kernel<96,2>"
G96 = GLDS96 if G96_V1 else (G96X2_4 if G96_X2 else G96X2_8)      # D = 96, >= 256 queries, every split owning a 64-key stage
KVX2 = KV64 if KV64_V1 else KV64X2                                  # kv64 with >= 256 queries
V1 = {"MSAM2_ATTN_V1": "1"}
LONG = 38 * 4096 + 64            # the steady-state memory bank of the largest configuration: 38 memories of 4096 tokens + pointer tokens


def effective_splits(Lk, splits):
    """attn_effective_splits of csrc/attention.hip: every split owns at least one 32-key tile"""
    tiles = (Lk + 31) // 32
    s = min(splits, tiles)
    while s > 1 and (s - 1) * ((tiles + s - 1) // s) >= tiles:
        s -= 1
    return s


def split_bounds(Lk, splits, unit):
    """first key of every split (and Lk at the end) when the keys are dealt out in units of `unit` keys: 32-key tiles everywhere but in
    attn_g96x2_kernel, which deals out 64-key stages"""
    n = (Lk + unit - 1) // unit
    per = (n + splits - 1) // splits
    return [min(s * per * unit, Lk) for s in range(splits + 1)]


def last_split_start(Lk, splits, unit):
    """first key of the last split that owns a key (a device-side key count can leave trailing splits empty)"""
    return max(b for b in split_bounds(Lk, splits, unit)[:-1] if b < Lk)


def live_splits(Lk, splits, unit=32):
    return len({b for b in split_bounds(Lk, splits, unit)[:-1] if b < Lk})


def plain(entry, B, H, Lq, Lk, D, splits, expect, env=None, **kw):
    """a case of msam2_attention_fwd ("fwd"; lse=True: _fwd_lse) or msam2_attention_kv64_* ("kv64"; D = 256 q / k rows, 64-wide v rows).
    layout: "plain" (each operand its own NaN-padded buffer, row pitch D + 8), "packed" (q / k / v strided views of one [B, L, 3, H, D]
    buffer; Lq == Lk), "pitch" (H = 1; k / v rows inside wider rows at element 64: pitch 320 / 128 for kv64, the memory-bank layouts);
    defer: split pass + attention_merge must equal the fused call bit for bit; partial = (n0, n1, ..): kv64 _partial over these sub-ranges
    of the splits + attention_merge likewise; dyn = key count on the device (Lk is the capacity; rows past the count hold NaN)."""
    c = dict(entry=entry, B=B, H=H, Lq=Lq, Lk=Lk, D=D, Dv=64 if entry == "kv64" else D, splits=splits, expect=list(expect), env=env or {},
             layout="plain", lse=False, defer=False, partial=None, dyn=None, mref=any(e in (G96X2_8, G96X2_4) for e in expect), p16=True)
    c.update(kw)
    c["eff"] = effective_splits(Lk, max(splits, 2) if c["lse"] else splits)
    c["keys"] = c["dyn"] or Lk
    return c


def case_id(c):
    if c["entry"] == "window":
        s = f"window-{c['B']}x{c['Hh']}x{c['Ww']}-h{c['heads']}-ws{c['ws']}{'-pool' if c['pool'] else ''}-D{c['D']}"
    elif c["entry"] == "small":
        s = f"small-{c['B']}x{c['H']}x{c['Lq']}x{c['Lk']}x{c['D']}"
    else:
        s = f"{c['entry']}-{c['B']}x{c['H']}x{c['Lq']}x{c['Lk']}x{c['D']}-s{c['splits']}"
        s += "".join(f"-{t}" for t in ("lse", "defer") if c[t]) + (f"-{c['layout']}" if c["layout"] != "plain" else "")
        s += (f"-dyn{c['dyn']}" if c["dyn"] else "") + (f"-partial{'+'.join(map(str, c['partial']))}" if c["partial"] else "")
    return s + "".join("-" + k.replace("MSAM2_", "") for k in c["env"])


# Dispatch rules (attention_fwd_impl, launch_attn_glds, dispatch_nw, g96x2_applies, launch_attn_kv64 in csrc/attention.hip): D = 64 always
# on the register-staged kernel with 1 / 2 / 4 waves for Lq <= 32 / <= 64 / more; D = 96 / 128 / 256 with more than 64 queries on the LDS-DMA
# kernels unless MSAM2_ATTN_V1=1 or the log-sum-exp rows are wanted from a single key tile; D = 96 with >= 256 queries on attn_g96x2_kernel
# when every split owns a 64-key stage.  The merge kernel unrolls up to 8 splits and walks more serially.
CASES = [
    # ---- attn_fwd_kernel<64, NW>: 1 query / 1 key; the 32 / 33 and 64 / 65 query edges; packed qkv with batch and heads
    plain("fwd", 1, 2, 1, 1, 64, 1, [FWD(64, 1)]),
    plain("fwd", 1, 1, 31, 31, 64, 1, [FWD(64, 1)]),
    plain("fwd", 2, 2, 32, 33, 64, 1, [FWD(64, 1)]),
    plain("fwd", 1, 2, 33, 32, 64, 1, [FWD(64, 2)]),
    plain("fwd", 1, 1, 64, 63, 64, 2, [FWD(64, 2), MERGE(64)]),
    plain("fwd", 1, 2, 65, 65, 64, 1, [FWD(64, 4)]),
    plain("fwd", 1, 1, 129, 100, 64, 3, [FWD(64, 4), MERGE(64)]),
    plain("fwd", 2, 4, 40, 40, 64, 1, [FWD(64, 2)], layout="packed"),
    plain("fwd", 1, 1, 100, 100, 64, 7, [FWD(64, 4), MERGE(64)]),                       # 4 tiles: the request of 7 runs as 4
    # ---- attn_fwd_kernel<96 / 128 / 256, NW> below 65 queries, with MSAM2_ATTN_V1=1 above, and for lse from a single key tile
    plain("fwd", 1, 1, 32, 64, 96, 1, [FWD(96, 1)]),
    plain("fwd", 1, 1, 64, 65, 96, 1, [FWD(96, 2)]),
    plain("fwd", 1, 2, 100, 31, 96, 1, [FWD(96, 4)], lse=True),                         # one key tile: the kernel writes lse itself
    plain("fwd", 1, 1, 127, 200, 96, 1, [FWD(96, 4)], env=V1),
    plain("fwd", 1, 1, 300, 330, 96, 2, [FWD(96, 4), MERGE(96)], env=V1),
    plain("fwd", 1, 1, 17, 96, 128, 1, [FWD(128, 1)]),
    plain("fwd", 1, 1, 64, 40, 128, 1, [FWD(128, 2)]),
    plain("fwd", 1, 1, 128, 129, 128, 1, [FWD(128, 4)], env=V1),
    plain("fwd", 1, 1, 8, 520, 256, 1, [FWD(256, 1)]),
    plain("fwd", 1, 1, 64, 4104, 256, 8, [FWD(256, 2), MERGE(256)]),                    # 8 splits: the last of the unrolled merge
    plain("fwd", 1, 1, 64, 2100, 256, 9, [FWD(256, 2), MERGE(256)]),                    # 9 splits: the serial merge
    plain("fwd", 1, 1, 40, 4091, 256, 64, [FWD(256, 2), MERGE(256)]),                   # 128 tiles in 64 splits of 2
    plain("fwd", 1, 1, 257, 300, 256, 1, [FWD(256, 4)], env=V1),
    # ---- attn_glds_kernel<128, 128, 4, 2>
    plain("fwd", 1, 1, 65, 64, 128, 1, [GLDS128]),
    plain("fwd", 2, 2, 127, 127, 128, 1, [GLDS128], layout="packed"),
    plain("fwd", 1, 1, 129, 1000, 128, 3, [GLDS128, MERGE(128)]),
    plain("fwd", 1, 1, 128, 200, 128, 1, [GLDS128, MERGE(128)], lse=True),
    # ---- attn_glds_kernel<256, 256, 4, 2>
    plain("fwd", 1, 1, 65, 33, 256, 1, [GLDS256]),
    plain("fwd", 1, 1, 130, 63, 256, 1, [GLDS256]),
    plain("fwd", 2, 1, 255, 520, 256, 1, [GLDS256]),
    plain("fwd", 1, 1, 256, 2100, 256, 7, [GLDS256, MERGE(256)]),
    plain("fwd", 1, 1, 300, 700, 256, 2, [GLDS256, MERGE(256)], defer=True),
    plain("fwd", 1, 1, 256, LONG, 256, 24, [GLDS256, MERGE(256)]),
    # ---- attn_glds_kernel<96, 128, 4, 3>: 65 .. 255 queries; >= 256 queries when a split owns a 32-key tile but no 64-key stage
    plain("fwd", 1, 1, 65, 31, 96, 1, [GLDS96]),
    plain("fwd", 2, 4, 70, 100, 96, 1, [GLDS96]),
    plain("fwd", 1, 2, 255, 1000, 96, 3, [GLDS96, MERGE(96)]),
    plain("fwd", 1, 1, 256, 96, 96, 3, [GLDS96, MERGE(96)]),                            # 3 tiles in 3 splits, but only 2 stages
    # ---- attn_g96x2_kernel (<1, 8> by default, <2, 4> under MSAM2_G96_X2, attn_glds_kernel<96, 128, 4, 3> under MSAM2_G96_V1)
    plain("fwd", 1, 1, 256, 64, 96, 1, [G96]),
    plain("fwd", 1, 1, 256, 31, 96, 1, [G96]),
    plain("fwd", 1, 2, 512, 96, 96, 1, [G96]),
    plain("fwd", 2, 1, 300, 200, 96, 1, [G96]),
    plain("fwd", 1, 1, 257, 65, 96, 1, [G96]),
    plain("fwd", 1, 1, 260, 1000, 96, 1, [G96]),
    plain("fwd", 1, 2, 384, 1100, 96, 3, [G96, MERGE(96)]),
    plain("fwd", 1, 1, 1024, 4100, 96, 7, [G96, MERGE(96)]),
    plain("fwd", 2, 2, 256, 256, 96, 1, [G96], layout="packed"),
    plain("fwd", 1, 1, 256, 300, 96, 1, [G96, MERGE(96)], lse=True),
    # ---- attn_kv64_kernel<4, 3> (fewer than 256 queries, or MSAM2_KV64_V1) and attn_kv64x2_kernel<4>
    plain("kv64", 1, 1, 1, 1, 256, 1, [KV64]),
    plain("kv64", 1, 1, 32, 32, 256, 1, [KV64]),
    plain("kv64", 2, 1, 200, 520, 256, 1, [KV64], layout="pitch"),
    plain("kv64", 1, 1, 130, 2100, 256, 4, [KV64, MERGE(64)]),
    plain("kv64", 2, 1, 64, 4104, 256, 8, [KV64, MERGE(64)]),
    plain("kv64", 1, 1, 255, 65, 256, 1, [KV64]),
    plain("kv64", 1, 2, 100, 63, 256, 2, [KV64, MERGE(64)]),
    plain("kv64", 2, 1, 300, 520, 256, 1, [KVX2]),
    plain("kv64", 1, 1, 256, 64, 256, 1, [KVX2]),
    plain("kv64", 1, 1, 512, 31, 256, 1, [KVX2]),
    plain("kv64", 1, 1, 257, 33, 256, 1, [KVX2]),
    plain("kv64", 1, 1, 260, 4100, 256, 7, [KVX2, MERGE(64)]),
    plain("kv64", 1, 1, 384, 96, 256, 3, [KVX2, MERGE(64)]),
    plain("kv64", 1, 1, 256, 2100, 256, 9, [KVX2, MERGE(64)]),
    plain("kv64", 2, 1, 320, 700, 256, 5, [KVX2, MERGE(64)], layout="pitch", defer=True),
    plain("kv64", 1, 1, 256, LONG, 256, 24, [KVX2, MERGE(64)]),
    # _partial over every split in two or three sub-ranges + attention_merge == the fused call
    plain("kv64", 1, 1, 130, 2100, 256, 4, [KV64, MERGE(64)], partial=(1, 3)),
    plain("kv64", 1, 1, 300, 1000, 256, 5, [KVX2, MERGE(64)], partial=(2, 1, 2)),
    # _dyn_fwd / _dyn_partial: capacity 1000 keys in 4 splits of 8 tiles; counts 1, a tile (and split) boundary +- 1, 40 (two tiles: the
    # last two splits stay empty), the capacity itself.  (The tie pass of 257 and 40 is what showed attn_kv64_kernel giving the partial
    # last tile to every empty trailing split once more.)
    *[plain("kv64", 1, 1, 100, 1000, 256, 4, [KV64, MERGE(64)], dyn=n) for n in (1, 255, 256, 257, 40, 1000)],
    *[plain("kv64", 1, 1, 256, 1000, 256, 4, [KVX2, MERGE(64)], dyn=n) for n in (1, 255, 256, 257, 40, 1000)],
    plain("kv64", 1, 1, 100, 1000, 256, 4, [KV64, MERGE(64)], dyn=257, partial=(1, 3)),
    plain("kv64", 1, 1, 256, 1000, 256, 4, [KVX2, MERGE(64)], dyn=40, partial=(2, 2)),
]


def window(B, Hh, Ww, heads, ws, pool, expect, D=96, env=None):
    """msam2_window_attention_fwd on a [B, Hh, Ww] token image, ws x ws windows (q-pooled: queries from the [B, Hh/2, Wh/2] image with
    windows of ws / 2), zero-padded at the bottom / right to whole windows: the padded tokens' K / V rows are the qkv bias"""
    wq = ws // 2 if pool else ws
    return dict(entry="window", B=B, Hh=Hh, Ww=Ww, heads=heads, H=heads, ws=ws, pool=pool, D=D, Dv=D, Lq=wq * wq, Lk=ws * ws, keys=ws * ws,
                splits=1, eff=1, expect=list(expect), env=env or {}, mref=False, p16=True, lse=False)


WV1, NOTINY, TINY64 = {"MSAM2_WIN_V1": "1"}, {"MSAM2_NO_TINYWIN": "1"}, {"MSAM2_TINYWIN_64": "1"}
# attn_win_applies: 32 < Lq <= 256, Lk >= 32, 2 Lq >= Lk, K + V images <= 80 KiB (ws = 16: 96 KiB, so the tiled kernel);
# attn_tinywin_applies: 16 keys, windows tile both images exactly, an even number of windows per image (64 keys and <= 32 queries under
# MSAM2_TINYWIN_64=1); everything else, and head dims 64 / 128, on the tiled kernel attn_fwd_kernel<D, NW, true>
WINDOW_CASES = [
    window(2, 16, 16, 1, 8, False, [WIN]),
    window(1, 18, 16, 2, 8, False, [WIN]),                         # padding at the bottom
    window(1, 16, 20, 2, 8, False, [WIN]),                         # on the right
    window(1, 20, 20, 1, 14, False, [WIN]),                        # both
    window(1, 28, 28, 8, 14, False, [WIN]),
    window(1, 8, 8, 8, 7, False, [WIN]),                           # both
    window(1, 14, 14, 2, 7, False, [WIN]),
    window(2, 16, 16, 1, 8, False, [FWD(96, 2, True)], env=WV1),
    window(1, 20, 20, 1, 14, False, [FWD(96, 4, True)], env=WV1),
    window(1, 8, 8, 8, 7, False, [FWD(96, 2, True)], env=WV1),
    window(1, 16, 16, 2, 4, False, [TINY1]),
    window(1, 8, 8, 4, 4, True, [TINY1]),
    window(2, 8, 8, 1, 4, False, [TINY1]),
    window(1, 8, 8, 8, 4, False, [TINY1]),
    window(1, 12, 12, 2, 4, False, [FWD(96, 1, True)]),            # 9 windows: the two-windows-per-wave kernel declines
    window(1, 10, 8, 2, 4, False, [FWD(96, 1, True)]),             # padding: it declines
    window(1, 16, 16, 2, 4, False, [FWD(96, 1, True)], env=NOTINY),
    window(1, 16, 16, 2, 8, True, [FWD(96, 1, True)]),
    window(1, 16, 16, 2, 8, True, [TINY2], env=TINY64),
    window(1, 32, 32, 1, 16, False, [FWD(96, 4, True)]),
    window(1, 20, 36, 2, 16, False, [FWD(96, 4, True)]),           # both
    window(1, 32, 32, 2, 16, True, [FWD(96, 2, True)]),
    window(1, 16, 16, 8, 14, True, [FWD(96, 2, True)]),            # both, q-pooled: 49 queries, 196 keys
    window(1, 16, 16, 2, 8, False, [FWD(64, 2, True)], D=64),
    window(1, 10, 12, 1, 4, False, [FWD(64, 1, True)], D=64),
    window(1, 20, 20, 2, 14, False, [FWD(128, 4, True)], D=128),
    window(1, 16, 16, 1, 8, True, [FWD(128, 1, True)], D=128),
]


def small(B, Lq, Lk, heads, D, expect, env=None):
    """msam2_attention_small_fwd: q [B, Lq, heads * D], k / v [B, Lk, heads * D]; fp32 arithmetic except attn_fewq16_kernel, which feeds
    16-bit probabilities to the matrix pipe"""
    return dict(entry="small", B=B, H=heads, Lq=Lq, Lk=Lk, keys=Lk, D=D, Dv=D, splits=1, eff=1, expect=list(expect), env=env or {}, mref=False,
                p16="fewq16" in expect[0], lse=False)


def FEWKEYS(D):
    return rf"attn_fewkeys_kernel<{D}>"


def FEWQ(D):
    return rf"attn_fewq_kernel<{D}>"


def SMALL(D):
    return rf"attn_small_kernel<{D}>"


FEWQ16 = r"attn_fewq16_kernel"
# fewkeys: Lk <= 32 and Lq >= 64; fewq16: D = 16, Lq <= 32, 1024 <= Lk <= 4096 (MSAM2_NO_FEWQ16=1 turns it off); fewq: Lk >= 1024 and
# B H Lq <= 4096; attn_small_kernel for the rest
SMALL_CASES = [
    small(2, 64, 32, 8, 16, [FEWKEYS(16)]),
    small(1, 64, 32, 8, 32, [FEWKEYS(32)]),
    small(2, 256, 8, 8, 16, [FEWKEYS(16)]),
    small(1, 100, 1, 4, 32, [FEWKEYS(32)]),
    small(1, 63, 32, 8, 16, [SMALL(16)]),
    small(1, 64, 33, 8, 16, [SMALL(16)]),
    small(1, 32, 1024, 8, 16, [FEWQ16]),
    small(2, 8, 4096, 8, 16, [FEWQ16]),
    small(1, 1, 1500, 8, 16, [FEWQ16]),
    small(1, 33, 1024, 8, 16, [FEWQ(16)]),
    small(1, 32, 1023, 8, 16, [SMALL(16)]),
    small(1, 32, 4097, 8, 16, [FEWQ(16)]),
    small(1, 32, 1024, 8, 16, [FEWQ(16)], env={"MSAM2_NO_FEWQ16": "1"}),
    small(2, 8, 1500, 8, 32, [FEWQ(32)]),
    small(1, 512, 1024, 8, 32, [FEWQ(32)]),                        # B H Lq = 4096
    small(1, 241, 1024, 17, 32, [SMALL(32)]),                      # 4097
    small(3, 7, 7, 8, 32, [SMALL(32)]),
    small(2, 8, 256, 8, 16, [SMALL(16)]),
]
ALL_CASES = CASES + WINDOW_CASES + SMALL_CASES


# ---------------------------------------------------------------------------------------------------------------------------------
# operands
def v_pattern(j, d, tie):
    """small integers of (key j, channel d): even channels ((1 + d // m) 29 j + 3 d) mod m, odd channels the same with 17 and the prime
    below m, centred; m = 61 / 59 (|V| <= 30; tie pass 31 / 29, |V| <= 15).  Two rows are equal only 61 * 59 (31 * 29) keys apart, two
    channels never over >= 64 keys (the factor 1 + d // m separates channels m apart)."""
    m1, m2 = (31, 29) if tie else (61, 59)
    j, d = j[..., :, None], d[None, :]
    a = ((1 + d // m1) * 29 * j + 3 * d) % m1 - m1 // 2
    b = ((1 + d // m2) * 17 * j + 5 * d) % m2 - m2 // 2
    return torch.where(d % 2 == 0, a, b).double()


def code(idx, nb):
    return (((idx[..., None] >> torch.arange(nb, device=idx.device)) & 1) * 2 - 1).double()


def sel_scale(D):
    return math.ceil(GAP / (2 * LOG2E / math.sqrt(D)))


def special_targets(Lk, eff):
    """the keys a kernel is most likely to get wrong, most telling first: the last key, the first key of the last split (32-key tiles and
    64-key stages), key 0, the keys on either side of every split boundary, first / last key of the first and last tile and stage"""
    b32, b64 = split_bounds(Lk, eff, 32), split_bounds(Lk, eff, 64)
    out = [Lk - 1, last_split_start(Lk, eff, 32), last_split_start(Lk, eff, 64), 0]
    for b in b32[1:-1] + b64[1:-1]:
        out += [b - 1, b]
    out += [31, 32, 63, 64, (Lk - 1) // 32 * 32, (Lk - 1) // 32 * 32 - 1, (Lk - 1) // 64 * 64, (Lk - 1) // 64 * 64 - 1, Lk - 2, 16, 33]
    seen, res = set(), []
    for t in out:
        if 0 <= t < Lk and t not in seen:
            seen.add(t)
            res.append(t)
    return res


def tie_pairs(Lk, eff):
    """(a, b): K[b] becomes K[a].  (a, Lk - 1) with a in another split / tile whenever there is one; a pair inside one tile; in different
    tiles of one split; first split / first tile of the last split (tiles and stages)"""
    if Lk < 2:
        return []
    b32 = split_bounds(Lk, eff, 32)
    cand = [(1 if Lk >= 3 else 0, Lk - 1), (4, 9), (6, 38)]
    if live_splits(Lk, eff) > 1:
        cand += [(11, last_split_start(Lk, eff, 32) + 3), (13, last_split_start(Lk, eff, 64) + 3)]
    pairs, used = [], set()
    for a, b in cand:
        if a < b < Lk and a not in used and b not in used:
            if (a, b) == (6, 38) and b32[1] <= 38:
                continue
            pairs.append((a, b))
            used |= {a, b}
    return pairs


def window_geometry(c, device):
    """(windows, pad_k [W, Lk] bool, pad_q [W, Lq] bool) of a window case: which tokens of every window lie outside the image"""
    def pads(h, w, ws):
        ph, pw = (ws - h % ws) % ws, (ws - w % ws) % ws
        img = torch.nn.functional.pad(torch.ones(c["B"], h, w, device=device), (0, pw, 0, ph))
        win = img.reshape(c["B"], (h + ph) // ws, ws, (w + pw) // ws, ws).permute(0, 1, 3, 2, 4).reshape(-1, ws * ws)
        return win == 0
    pk = pads(c["Hh"], c["Ww"], c["ws"])
    pq = pads(c["Hh"] // 2, c["Ww"] // 2, c["ws"] // 2) if c["pool"] else pk
    assert pk.shape[0] == pq.shape[0]
    return pk.shape[0], pk, pq


class Problem:
    """q / k / v in instance form (float64, already exact in the 16-bit operand types for the integer passes), the log2-domain scale c,
    what the output must be (`expected`, integer passes), which query rows exist (`q_valid` [Bz, Lq]), and for windows the pad masks"""
    pass


def build(c, kind, device="cpu", op16=None):
    """kind: "sel", "tie" or "rand".  op16: round the random operands to this dtype (the integer ones are exact in both)."""
    P = Problem()
    D, Dv, Lq, Lk, H = c["D"], c["Dv"], c["Lq"], c["keys"], c["H"]
    win = c["entry"] == "window"
    if win:
        Bz, pad_k, pad_q = window_geometry(c, device)
    else:
        Bz, pad_k, pad_q = c["B"], None, None
    P.c, P.pad_k, P.Bz = LOG2E / math.sqrt(D), pad_k, Bz
    P.q_valid = ~pad_q if win else torch.ones(Bz, Lq, dtype=torch.bool, device=device)
    n = (torch.arange(Bz, device=device)[:, None] * H + torch.arange(H, device=device)[None, :])          # instance number [Bz, H]
    if kind == "rand":
        g = torch.Generator(device=device).manual_seed(1000 + 7 * Lq + 3 * Lk + D + Bz)
        q = torch.randn(Bz, H, Lq, D, generator=g, device=device) * 2.0          # scores ~ N(0, 2^2): neither flat nor one-hot rows
        k = torch.randn(Bz, H, Lk, D, generator=g, device=device)
        v = torch.randn(Bz, H, Lk, Dv, generator=g, device=device)
        if Lk >= 40 and Lq >= 8:                                                  # one key far above the rest in a late tile
            k[0, 0, Lk - 3] = q[0, 0, 5] * 0.75
        kb, vb = torch.randn(H, D, generator=g, device=device), torch.randn(H, Dv, generator=g, device=device)
        q, k, v, kb, vb = (t.to(op16).double() if op16 is not None else t.double() for t in (q, k, v, kb, vb))
        P.expected = None
    else:
        tie = kind == "tie"
        nb = max(1, (Lk - 1).bit_length())
        assert nb + (1 if win else 0) <= D and sel_scale(D) <= 256
        s = float(sel_scale(D))
        spec = special_targets(Lk, c["eff"])
        i = torch.arange(Lq, device=device)
        nn = n[:, :, None]
        walk = (37 * i[None, None, :] + 5 + 11 * nn) % Lk
        spec_t = torch.tensor(spec, device=device)[(i[None, None, :] + nn) % len(spec)]
        t = torch.where(i[None, None, :] < len(spec), spec_t, walk)                # [Bz, H, Lq]
        jk = torch.arange(Lk, device=device)
        rep = jk.repeat(Bz, 1)                                                     # key -> the key whose K row it carries
        pairs = tie_pairs(Lk, c["eff"]) if tie else []
        for a, b in pairs:
            rep[:, b] = a
        if win:
            t = torch.where(torch.gather(pad_k[:, None, :].expand(Bz, H, Lk), 2, t), torch.zeros_like(t), t)
            if tie:                                                                # a pair whose a is padding here is no pair; padded
                rep = torch.where(torch.gather(pad_k, 1, rep), jk.repeat(Bz, 1), rep)     # tokens carry key 0's code (through the bias)
                rep = torch.where(pad_k, torch.zeros_like(rep), rep)
        if tie:
            t = torch.gather(rep[:, None, :].expand(Bz, H, Lk), 2, t)
            if pairs:
                a_t = torch.tensor([a for a, _ in pairs], device=device)[(i[None, None, :] + nn) % len(pairs)]
                a_t = torch.where(torch.gather(pad_k[:, None, :].expand(Bz, H, Lk), 2, a_t), torch.zeros_like(a_t), a_t) if win else a_t
                t = torch.where((i[None, None, :] < 2 * len(pairs)) | (i[None, None, :] % 5 == 0), a_t, t)
        kc = code(rep, nb)                                                         # [Bz, Lk, nb]
        k = torch.zeros(Bz, H, Lk, D, dtype=torch.float64, device=device)
        k[..., :nb] = kc[:, None]
        q = torch.zeros(Bz, H, Lq, D, dtype=torch.float64, device=device)
        q[..., :nb] = s * code(t, nb)
        dd = torch.arange(Dv, device=device)
        v = v_pattern(jk[None, None, :] + 13 * n[:, :, None], dd, tie)            # [Bz, H, Lk, Dv]
        kb = torch.zeros(H, D, dtype=torch.float64, device=device)
        vb = v_pattern(977 + 5 * torch.arange(H, device=device), dd, tie)
        if win:                                                                    # channel nb: +1 on real keys, -1 on the bias
            k[..., nb], q[..., nb], kb[:, nb] = 1.0, s, -1.0
            if tie:
                kb[:, :nb], kb[:, nb] = code(torch.zeros(1, dtype=torch.long, device=device), nb), 1.0
        P.t, P.rep, P.pairs, P.vmax = t, rep, pairs, (15.0 if tie else 30.0)
    if win:
        k = torch.where(pad_k[:, None, :, None], kb[None, :, None, :], k)
        v = torch.where(pad_k[:, None, :, None], vb[None, :, None, :], v)
        q = q * P.q_valid[:, None, :, None]
        P.kbias, P.vbias = kb, vb
    P.q, P.k, P.v = q, k, v
    if kind != "rand":
        # closed form: the mean of V over the keys that carry the target's K row
        sums = torch.zeros_like(v).scatter_add_(2, P.rep[:, None, :, None].expand_as(v), v)
        cnt = torch.zeros(Bz, Lk, dtype=torch.float64, device=device).scatter_add_(1, P.rep, torch.ones(Bz, Lk, dtype=torch.float64, device=device))
        mean = sums / cnt.clamp_min(1)[:, None, :, None]
        P.expected = torch.gather(mean, 2, P.t[..., None].expand(Bz, H, Lq, Dv))
        asum = torch.zeros_like(v).scatter_add_(2, P.rep[:, None, :, None].expand_as(v), v.abs()) / cnt.clamp_min(1)[:, None, :, None]
        P.A = torch.gather(asum, 2, P.t[..., None].expand(Bz, H, Lq, Dv))          # sum_j p_j |v_jd|: the mean of |V| over those keys
        check_pattern(v, c, P.pad_k)
    return P


def check_pattern(v, c, pad_k):
    """the properties the integer passes lean on: keys a confusable distance apart (< 64, a multiple of 16 up to 1024, 4096, a split
    length) never have equal V rows; no two channels are equal over all keys (from 64 keys on)"""
    Lk = v.shape[2]
    assert v.abs().max().item() <= 31
    per = {split_bounds(Lk, c["eff"], u)[1] for u in (32, 64)} if c["eff"] > 1 else set()
    deltas = sorted(set(range(1, 64)) | set(range(16, 1025, 16)) | {4096} | per)
    assert all(d % (61 * 59) and d % (31 * 29) for d in deltas)                   # the pattern's analytic period
    if pad_k is not None:
        return
    w = v[0, 0, :8192]
    for d in deltas:
        if d < w.shape[0]:
            assert not (w[:-d] == w[d:]).all(1).any(), f"V rows {d} keys apart are equal"
    if Lk >= 64:
        assert torch.unique(w, dim=1).shape[1] == w.shape[1], "two V channels are equal over all keys"


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 reference and bounds
def reference(q, k, v, c, rows=1 << 25):
    """float64 softmax attention over query chunks of at most `rows` score elements.  Returns the output, A = sum_j p_j |v_jd|,
    smax = max_j sum_d |q_id k_jd| and lse = log2 sum_j 2^(c q.k)."""
    Bz, H, Lq, _ = q.shape
    Lk = k.shape[2]
    step = max(1, rows // max(1, Bz * H * Lk))
    kt, ka, va = k.transpose(2, 3), k.abs().transpose(2, 3), v.abs()
    out, A, smax, lse = [], [], [], []
    for i in range(0, Lq, step):
        qc = q[:, :, i:i + step]
        s = (qc @ kt) * c
        m = s.max(-1, keepdim=True).values
        p = torch.exp2(s - m)
        l = p.sum(-1, keepdim=True)
        out.append(p @ v / l)
        A.append(p @ va / l)
        lse.append((m + torch.log2(l))[..., 0])
        smax.append((qc.abs() @ ka).max(-1, keepdim=True).values)
    return torch.cat(out, 2), torch.cat(A, 2), torch.cat(smax, 2), torch.cat(lse, 2)


def integer_bound(expected, A, Lk, split, fp16, vmax):
    """Bound of the selection and tie passes.  Every probability is 0, 1 or 1 / 2 to within 2^-(GAP-1) whatever the fp32 score error, so a
    correct kernel is off by: P rounded to 16 bits before P V (relative to p: the kernels' reference need not be the row maximum),
    u16 A with A = sum_j p_j |v_jd|; with split-KV the 16-bit partial outputs, u16 A once more; the output rounding, u16 |expected|; the
    other keys' mass, vmax Lk 2^-(GAP-1); a few fp32 roundings (exp2, the row sum, the normalisation), 8 u vmax.
    A and not |expected| in the first two terms: the two keys of a tie can sit in different tiles or splits, where their probabilities
    (powers of two of different references) and their partial outputs are rounded independently, so with V rows of opposite sign the
    errors do not shrink with their mean (seen on attn_g96x2_kernel with two splits: one fp16 ulp of 15 on an expected 1.0).  In the
    selection pass A = |expected|: (2 or 3) u16 |expected|."""
    h = u16(fp16)
    return (2 if split else 1) * h * A + h * expected.abs() + vmax * Lk * 2.0 ** -(GAP - 1) + 8 * U * vmax


def score_error(smax, D, c, fp16, mref):
    """ds: error of a score in the log2 domain.  fp32 accumulation of D exact products and the scaling, (D + 2) u c sum_d |q k|; the kernels
    that pre-multiply Q by c and round it to 16 bits (attn_g96x2_kernel with MSAM2_G96_MREF) add u16 c sum_d |q k|."""
    return ((D + 2) * U + (u16(fp16) if mref else 0.0)) * c * smax


def attention_error_bound(ref, A, smax, Lk, D, c, *, fp16, mref=False, split=False, p16=True):
    """Largest |kernel - float64 reference| of a correct kernel, element by element (float64 tensors: ref [.., Lq, Dv], A = sum_j p_j |v_jd|
    likewise, smax = max_j sum_d |q k| [.., Lq, 1]).  u = 2^-24, u16 = 2^-11 (fp16) / 2^-8 (bf16).
      * scores: ds = score_error(); every probability is then off by a factor within 2^(+-ds), numerator and denominator of the
        normalised output together by 2^(2 ds): (2^(2 ds) - 1) A;
      * P rounded to 16 bits before P V while the row sum takes the unrounded values (so it does not cancel), relative to p because the
        running reference may lag the maximum by MSAM2_RESCALE_SLACK bits: u16 A (p16; the fp32 attention_small kernels have none);
      * fp32 accumulation of P V and of the row sum over the keys, Lk u A; exp2, the lazy rescales of O and the final division, 8 u A;
      * split-KV: partial outputs stored normalised in 16 bits, u16 A, and the merge weights, 4 u A;
      * the 16-bit output: u16 (|ref| + the above) + half the fp16 subnormal spacing."""
    h = u16(fp16)
    ds = score_error(smax, D, c, fp16, mref)
    e = torch.expm1(2 * math.log(2.0) * ds) * A + (h * A if p16 else 0.0) + (Lk + 8) * U * A
    if split:
        e = e + (h + 4 * U) * A
    return e + h * (ref.abs() + e) + 2.0 ** -25


def lse_bound(lse, smax, D, c, fp16, mref):
    """|lse - log2 sum_j 2^(c q.k)| <= max_j ds + a few u |lse|"""
    return score_error(smax, D, c, fp16, mref)[..., 0] + 4 * U * lse.abs() + 4 * U


# ---------------------------------------------------------------------------------------------------------------------------------
# simulated defects (CPU companion): each returns the output a kernel with that defect would give, or None where it does not apply
def _attn(q, k, v, c, w=None):
    s = (q @ k.transpose(2, 3)) * c
    p = torch.exp2(s - s.max(-1, keepdim=True).values)
    if w is not None:
        p = p * w
    return p @ v / p.sum(-1, keepdim=True)


def _perm(L, x):
    j = torch.arange(L)
    jj = j ^ x
    return torch.where(jj < L, jj, j)


def defects(c, P):
    """{name: output} of every simulated defect that applies to case c, computed on problem P"""
    q, k, v, cc = P.q, P.k, P.v, P.c
    Bz, H, Lq, D = q.shape
    Lk, Dv, eff = k.shape[2], v.shape[3], c["eff"]
    out = {}
    good = _attn(q, k, v, cc)
    if Lk >= 2:
        out["V rows of neighbouring keys swapped"] = _attn(q, k, v[:, :, _perm(Lk, 1)], cc)
        out["key Lk-1 dropped"] = _attn(q, k[:, :, :-1], v[:, :, :-1], cc)
        w = torch.ones(Lk, dtype=torch.float64)
        w[-1] = 2
        out["last key counted twice"] = _attn(q, k, v, cc, w)
    for x in (16, 32):
        if Lk > x:
            out[f"keys j and j^{x} swapped in K"] = _attn(q, k[:, :, _perm(Lk, x)], v, cc)
    for unit in (32, 64):
        b = split_bounds(Lk, eff, unit)
        if live_splits(Lk, eff, unit) > 1 and not (unit == 64 and (b == split_bounds(Lk, eff, 32) or not c["mref"])):
            b0 = last_split_start(Lk, eff, unit)
            for name, val in (("skipped", 0.0), ("counted twice", 2.0)):
                w = torch.ones(Lk, dtype=torch.float64)
                w[b0:b0 + 32] = val
                out[f"first tile of the last split ({unit}-key units) {name}"] = _attn(q, k, v, cc, w)
            for name, idx in (("last key of the first split", b[1] - 1), ("first key of the last split", b0)):
                w = torch.ones(Lk, dtype=torch.float64)
                w[idx] = 0.0
                out[f"{name} ({unit}-key units) dropped"] = _attn(q, k, v, cc, w)
            parts = [_attn(q, k[:, :, b[s]:b[s + 1]], v[:, :, b[s]:b[s + 1]], cc) for s in range(eff) if b[s] < b[s + 1]]
            out[f"splits merged with equal weights ({unit}-key units)"] = sum(parts) / len(parts)
    if Lk > 32:
        # online softmax over 32-key tiles whose O is not rescaled when the running maximum moves (the row sum is)
        T = (Lk + 31) // 32
        s = torch.full((Bz, H, Lq, T * 32), -float("inf"), dtype=torch.float64)
        s[..., :Lk] = (q @ k.transpose(2, 3)) * cc
        run = s.view(Bz, H, Lq, T, 32).max(-1).values.cummax(-1).values                      # running maximum after every tile
        p_then = torch.exp2(s.view(Bz, H, Lq, T, 32) - run[..., None]).reshape(Bz, H, Lq, T * 32)[..., :Lk]
        p_true = torch.exp2(s[..., :Lk] - run[..., -1:])
        out["O not rescaled when the running maximum moves"] = p_then @ v / p_true.sum(-1, keepdim=True)
    for x in (4, 32):
        if Dv > x:
            out[f"output channels d and d^{x} swapped"] = good[..., _perm(Dv, x)]
    if Lq > 16 and Lk >= 2:                      # (with one key every row of the output is that key's V row)
        out["query rows i and i^16 swapped"] = good[:, :, _perm(Lq, 16)]
    if c["entry"] == "window":
        if P.pad_k.any():
            z = ~P.pad_k[:, None, :, None]
            out["padded window tokens with zero K / V"] = _attn(q, k * z, v * z, cc)
        if any("tinywin_kernel<96,1>" in e for e in c["expect"]):
            pair = torch.arange(Bz) ^ 1
            out["two windows of a wave not masked from each other"] = _attn(q, torch.cat((k, k[pair]), 2), torch.cat((v, v[pair]), 2), cc)
    return out
