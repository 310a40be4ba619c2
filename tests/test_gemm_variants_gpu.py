"""GEMM kernel-variant matrix (GPU): every forward kernel that msam2_gemm / msam2_gemm_rope can pick (gemm_launch, csrc/gemm.hip) reached
on purpose -- through its shape and the MSAM2_* switches that gemm_launch reads per call -- and checked at its edges.

Each case of CASES / ROPE_CASES names the kernel(s) it must reach; torch.profiler asserts that exactly those GEMM kernels ran, so that a
change of the dispatch heuristics cannot move the coverage to another kernel silently.  Per case and epilogue:
  * A and W are views inside larger NaN-filled buffers (lda, ldw > K; rows past M / N): a kernel that uses any padding element returns NaN;
  * the output is a view inside a sentinel-filled buffer (rows and columns on every side, ldc > N; an odd ldc for the generic 16-bit
    store): the sentinels must be bit-identical afterwards;
  * exact pass: small-integer operands with row, column and k-chunk structure (a swapped row, column or k-chunk, or a lost k-tile, changes
    the result), every output < 256 (exact in fp16 and bf16): bit for bit against float64 wherever the epilogue's arithmetic is exact on
    integers (linear, bias, column scale, residuals, ReLU), within error_bound() for GELU / sigmoid / RoPE;
  * random pass: float64 reference from the operand-rounded inputs, every element within error_bound();
  * reproducibility: the random pass launched once more while an independent GEMM runs on a second stream (other wave scheduling) must give
    the same bits -- split-K on its integer data, the one where the atomics' order cannot matter.
The float64 references run on the GPU (torch), so at-size W-stationary shapes cost milliseconds.  The opt-in 256-row W-stationary kernel
runs the default W-stationary cases in a child process (MSAM2_GEMM_WSTAT256 is read once per process).
"""
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import sam2_oracle as O  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import Canvas, kernels_launched, nan_padded  # noqa: E402

DEV = "cuda"
SWITCHES = ("MSAM2_GEMM_V1", "MSAM2_GEMM_VARIANT", "MSAM2_GEMM_WSTAT", "MSAM2_NT_BYTES", "MSAM2_NT_BYTES_F32", "MSAM2_NO_SPLITK")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import medical_sam2_amd.ops as ops_mod
    return ops_mod


@pytest.fixture(scope="module")
def background(ops):
    """an independent GEMM (8192 x 2048 x 1024, all CUs busy for tens of microseconds) to launch on a second stream"""
    g = torch.Generator(device=DEV).manual_seed(99)
    a = torch.randn(8192, 1024, generator=g, device=DEV).to(ops.OP16)
    w = (torch.randn(2048, 1024, generator=g, device=DEV) * 0.05).to(ops.OP16)
    c = torch.empty(8192, 2048, dtype=ops.OP16, device=DEV)
    s2 = torch.cuda.Stream()
    s2.wait_stream(torch.cuda.current_stream())

    def launch():
        with torch.cuda.stream(s2):
            ops.gemm(a, w, out=c)
    return launch


@pytest.fixture
def clean_env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


# ---------------------------------------------------------------------------------------------------------------------------------
def error_bound(S, n_terms, pre, ref, *, act=0, colscale=None, out16=False, fp16=True):
    """Largest |kernel - float64 reference| a correct kernel can show, element by element (float64 tensors, broadcast together).

    S        sum_k |a_ik w_jk| of the operand-rounded inputs (their products are exact in fp32);
    n_terms  fp32 additions along one output (K; split-K adds one per split);
    pre      a w^T + bias in float64 (the pre-activation), ref the float64 result.
    Terms: fp32 accumulation in any order, n_terms * 2^-24 * S (the gamma_n bound, unit round-off 2^-24); one fp32 rounding of the bias add,
    2^-24 |pre|; both carried through the activation with its Lipschitz constant (ReLU 1, GELU 1.13, sigmoid 1/4) and scaled by |colscale|;
    GELU: + the 5e-5 absolute error csrc/common.h states for its polynomial erf form; sigmoid: + 1e-6 (__expf and the reciprocal are a
    few fp32 ulps of a value <= 1); the column scale and the residual add: two more fp32 roundings, 2^-23 |ref|; a 16-bit output: + half an
    ulp of the output type relative to the value, 2^-11 (fp16) or 2^-8 (bf16), and half the fp16 subnormal spacing."""
    u = 2.0 ** -24
    e = n_terms * u * S + u * pre.abs()
    e = e * {0: 1.0, 1: 1.13, 2: 1.0, 3: 0.25}[act] + {0: 0.0, 1: 5e-5, 2: 0.0, 3: 1e-6}[act]
    if colscale is not None:
        e = e * colscale.abs()
    e = e + 2 * u * ref.abs()
    if out16:
        e = e + (2.0 ** -11 if fp16 else 2.0 ** -8) * (ref.abs() + e) + 2.0 ** -25
    return e


def gemm_kernels_launched(fn):
    """the set of GEMM kernels of libmsam2_hip.so that fn launched (torch.profiler, kernel activity)"""
    return kernels_launched(fn, "gemm_")


def assert_reached(launched, expect, what):
    assert launched, f"{what}: the profiler saw no GEMM kernel"
    for pat in expect:
        assert any(re.fullmatch(pat, k) for k in launched), f"{what}: expected {pat}, launched {sorted(launched)}"
    stray = [k for k in launched if not any(re.fullmatch(pat, k) for pat in expect)]
    assert not stray, f"{what}: other GEMM kernels ran: {stray} (expected only {expect})"


# ---------------------------------------------------------------------------------------------------------------------------------
def int_operands(M, N, K, seed):
    """small integers with structure: column 0 carries the row index mod 3 / 4, every row has a +1 in its own k-chunk (8 m + 3 mod K), the
    last column (inside the last, possibly partial k-tile) varies per 32-row / 32-column block, plus a few random entries per row"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    a = torch.zeros(M, K, device=DEV)
    w = torch.zeros(N, K, device=DEV)
    nz = min(4, K)
    a.scatter_add_(1, torch.randint(0, K, (M, nz), generator=g, device=DEV), torch.randint(-1, 2, (M, nz), generator=g, device=DEV).float())
    w.scatter_add_(1, torch.randint(0, K, (N, nz), generator=g, device=DEV), torch.randint(-1, 2, (N, nz), generator=g, device=DEV).float())
    im, iN = torch.arange(M, device=DEV), torch.arange(N, device=DEV)
    a[:, 0] += (im % 3).float()
    w[:, 0] += (iN % 4).float() - 1
    a[im, (8 * im + 3) % K] += 1
    w[iN, (8 * iN + 5) % K] += 1
    a[:, K - 1] += ((im // 32) % 5).float() - 2
    w[:, K - 1] += 1 + ((iN // 32) % 2).float()
    return a, w


# epilogues: out 16-bit / fp32, bias, colscale, residual (fp32 with ldr > N, 16-bit, or fp32 indexed m % res_mod), act, store_nt forced on
# (MSAM2_NT_BYTES(_F32)=0), output layout (aligned: direct / LDS-specialised epilogues; odd: generic epilogue, odd ldc for 16-bit)
EPI = {
    "lin_f32": dict(out=32),
    "lin_16": dict(out=16),
    "bias_f32": dict(out=32, bias=True),
    "bias_cs_f32": dict(out=32, bias=True, cs=True),
    "bias_cs_16": dict(out=16, bias=True, cs=True),
    "res_f32": dict(out=32, bias=True, res=32),
    "res_16": dict(out=16, bias=True, res=32),
    "res16_f32": dict(out=32, res=16),
    "resmod_f32": dict(out=32, bias=True, cs=True, res=32, res_mod=True),
    "gelu_16": dict(out=16, bias=True, act=1),
    "gelu_f32": dict(out=32, bias=True, act=1),
    "relu_16": dict(out=16, bias=True, act=2),
    "sigmoid_f32": dict(out=32, bias=True, act=3),
    "nt_lin_f32": dict(out=32, bias=True, nt=True),
    "nt_lin_16": dict(out=16, nt=True),
    "nt_gelu_16": dict(out=16, bias=True, act=1, nt=True),
    "nt_relu_16": dict(out=16, bias=True, act=2, nt=True),
    "odd_16": dict(out=16, bias=True, aligned=False),
    "odd_f32": dict(out=32, aligned=False),
}
FULL = list(EPI)
WSTAT = ["lin_16", "relu_16", "gelu_16", "nt_lin_16", "nt_relu_16"]
SPLITK = ["lin_f32", "bias_f32", "nt_lin_f32", "odd_f32"]

R32x128, R128x32, R128x64, R128x128 = (r"gemm_kernel<32,128,1,4>", r"gemm_kernel<128,32,4,1>", r"gemm_kernel<128,64,2,2>",
                                       r"gemm_kernel<128,128,2,2>")
SKINNY, GLDS, GLDS32 = r"gemm_skinny_kernel<false>", r"gemm_glds_kernel", r"gemm_glds32_kernel<2,4>"
WIDE = {6: r"gemm_wide_kernel<256,128,3,2>", 8: r"gemm_wide_kernel<128,128,3,3>", 9: r"gemm_wide_kernel<256,128,2,2>",
        10: r"gemm_wide_kernel<128,128,2,4>", 11: r"gemm_wide_kernel<128,128,4,2>"}
V1 = {"MSAM2_GEMM_V1": "1"}


def var(v):
    return {"MSAM2_GEMM_VARIANT": str(v)}


# MSAM2_GEMM_WSTAT256=1 (read once per process; test_gemm_wstat256_kernel_in_a_child_process) sends the default W-stationary cases to the
# 256-row kernel instead; the A-prefetch form (MSAM2_GEMM_WSTAT=2) stays on the 128-row kernel
WS256 = os.environ.get("MSAM2_GEMM_WSTAT256", "").startswith("1")


def wstat(nk, act="[012]", nt="(true|false)", apf=False):
    if WS256 and not apf:
        return rf"gemm_wstat256_kernel<{nk},{act},{nt}>"
    return rf"gemm_wstat_kernel<{nk},{act},{nt},{'true' if apf else 'false'}>"


# (id label, expected kernel patterns, env, M, N, K, epilogues).  Dispatch rules: gemm_launch in csrc/gemm.hip.  The DMA and W-stationary
# kernels need M >= 256 and N >= 96 (dma_ok), so their M / N edges are tile multiples +- 1 above those floors.
CASES = [
    # register-staged 32x128: M <= 32 with K % 16 != 0
    ("gemm_kernel<32,128,1,4>", [R32x128], {}, 1, 3, 8, FULL),
    ("gemm_kernel<32,128,1,4>", [R32x128], {}, 31, 129, 24, FULL),
    ("gemm_kernel<32,128,1,4>", [R32x128], {}, 32, 127, 40, FULL),
    ("gemm_kernel<32,128,1,4>", [R32x128], {}, 17, 260, 8, FULL),
    # register-staged 128x32: N <= 32 (K = 8 / 16 with N = 4 / 16: the mask-prompt convs of sam_heads.py)
    ("gemm_kernel<128,32,4,1>", [R128x32], {}, 33, 1, 16, FULL),
    ("gemm_kernel<128,32,4,1>", [R128x32], {}, 127, 3, 8, FULL),
    ("gemm_kernel<128,32,4,1>", [R128x32], {}, 129, 31, 24, FULL),
    ("gemm_kernel<128,32,4,1>", [R128x32], {}, 256, 32, 40, FULL),
    ("gemm_kernel<128,32,4,1>", [R128x32], {}, 300, 28, 16, FULL),
    ("gemm_kernel<128,32,4,1>", [R128x32], {}, 16384, 4, 8, ["bias_f32"]),
    ("gemm_kernel<128,32,4,1>", [R128x32], {}, 4096, 16, 16, ["bias_f32"]),
    # register-staged 128x64: N <= 64, or N % 64 == 0 with N < 512 and no DMA kernel
    ("gemm_kernel<128,64,2,2>", [R128x64], {}, 33, 33, 8, FULL),
    ("gemm_kernel<128,64,2,2>", [R128x64], {}, 127, 63, 24, FULL),
    ("gemm_kernel<128,64,2,2>", [R128x64], {}, 129, 64, 16, FULL),
    ("gemm_kernel<128,64,2,2>", [R128x64], {}, 256, 60, 40, FULL),
    ("gemm_kernel<128,64,2,2>", [R128x64], {}, 200, 192, 96, FULL),
    # register-staged 128x128: the rest without a DMA kernel; MSAM2_GEMM_V1=1 at a DMA-sized shape
    ("gemm_kernel<128,128,2,2>", [R128x128], {}, 33, 127, 8, FULL),
    ("gemm_kernel<128,128,2,2>", [R128x128], {}, 127, 129, 24, FULL),
    ("gemm_kernel<128,128,2,2>", [R128x128], {}, 129, 132, 16, FULL),
    ("gemm_kernel<128,128,2,2>", [R128x128], V1, 1000, 388, 104, FULL),
    ("gemm_kernel<128,128,2,2>", [R128x128], V1, 256, 256, 384, FULL),
    # skinny: M <= 32, K % 16 == 0
    ("gemm_skinny_kernel", [SKINNY], {}, 1, 1, 16, FULL),
    ("gemm_skinny_kernel", [SKINNY], {}, 31, 33, 48, FULL),
    ("gemm_skinny_kernel", [SKINNY], {}, 32, 36, 2048, FULL),
    ("gemm_skinny_kernel", [SKINNY], {}, 17, 3, 256, FULL),
    # LDS-DMA 128x128x64 (variant 2; default for K % 64 == 0, K >= 384 outside the few-tiles-long-K rule)
    ("gemm_glds_kernel", [GLDS], var(2), 257, 97, 64, FULL),
    ("gemm_glds_kernel", [GLDS], var(2), 383, 132, 64, FULL),
    ("gemm_glds_kernel", [GLDS], var(2), 512, 256, 192, FULL),
    ("gemm_glds_kernel", [GLDS], {}, 1000, 384, 384, FULL),
    # LDS-DMA 128x128x32 4-stage (variant 5; default for the other K % 32 == 0 shapes)
    ("gemm_glds32_kernel", [GLDS32], {}, 257, 129, 32, FULL),
    ("gemm_glds32_kernel", [GLDS32], {}, 383, 132, 96, FULL),
    ("gemm_glds32_kernel", [GLDS32], {}, 512, 97, 160, FULL),
    ("gemm_glds32_kernel", [GLDS32], var(5), 300, 256, 64, FULL),
    # wide-tile DMA (variants 6, 8, 9, 10, 11; 8 is the default for <= 256 tiles with K >= 1024)
    ("gemm_wide_kernel-v8", [WIDE[8]], {}, 257, 132, 1024, FULL),
    ("gemm_wide_kernel-v8", [WIDE[8]], var(8), 256, 128, 32, FULL),
    ("gemm_wide_kernel-v6", [WIDE[6]], var(6), 383, 129, 32, FULL),
    ("gemm_wide_kernel-v9", [WIDE[9]], var(9), 512, 132, 96, FULL),
    ("gemm_wide_kernel-v10", [WIDE[10]], var(10), 257, 256, 64, FULL),
    ("gemm_wide_kernel-v11", [WIDE[11]], var(11), 300, 97, 160, FULL),
    # W-stationary: 16-bit out, act 0 / 1 / 2, K 256 / 384, N % 128 == 0 (n_panels <= 32), M % 128 == 0, M >= 8192.  groups =
    # min(256 / n_panels, M / 128): one panel at M = 8192 -> one 128-row unit per workgroup; 32 panels at M = 9216 -> 9 units (odd)
    ("gemm_wstat_kernel", [wstat(4)], {}, 8192, 128, 256, WSTAT),
    ("gemm_wstat_kernel", [wstat(4)], {}, 9216, 4096, 256, WSTAT),
    ("gemm_wstat_kernel", [wstat(6)], {}, 9216, 4096, 384, WSTAT),
    ("gemm_wstat_kernel-fc1", [wstat(6, act="1", nt="true")], {}, 16384, 1536, 384, ["gelu_16"]),   # Hiera fc1: > 30 MB, stored nt
    ("gemm_wstat_kernel-apf", [wstat(4, apf=True)], {"MSAM2_GEMM_WSTAT": "2"}, 8192, 128, 256, WSTAT),
    ("gemm_wstat_kernel-apf", [wstat(6, apf=True)], {"MSAM2_GEMM_WSTAT": "2"}, 9216, 1536, 384, WSTAT),
    # split-K: fp32 out, act 0, no colscale / residual, <= 32 output tiles, K >= 4096; splits that do not divide the k-tiles
    # (K = 4136: 130 k-tiles, the last one partial, in 15 splits of 9; K = 8200: 257 k-tiles in 29 splits of 9)
    ("split_k", [r"gemm_zero_kernel", R128x128], {}, 33, 129, 4136, SPLITK),
    ("split_k", [r"gemm_zero_kernel", R128x128], {}, 256, 252, 8200, SPLITK),
]


def case_id(c):
    return f"{c[0]}-{c[3]}x{c[4]}x{c[5]}" + ("-V1" if c[2].get("MSAM2_GEMM_V1") else "")


def epilogue_inputs(spec, M, N, seed, integer):
    """bias / column scale (fp32 vectors followed by NaN) and the residual source rows ([M, N], or [min(M, 7), N] read as m % res_mod)"""
    g = torch.Generator(device=DEV).manual_seed(seed)

    def vec(lo, hi, rand):
        buf = torch.full((N + 8,), float("nan"), device=DEV)
        buf[:N] = torch.randint(lo, hi, (N,), generator=g, device=DEV).float() if integer else rand()
        return buf[:N]
    bias = vec(-4, 5, lambda: torch.randn(N, generator=g, device=DEV)) if spec.get("bias") else None
    cs = vec(1, 3, lambda: 0.5 + torch.rand(N, generator=g, device=DEV)) if spec.get("cs") else None
    res, res_mod = None, 0
    if spec.get("res"):
        rows = min(M, 7) if spec.get("res_mod") else M
        res_mod = rows if spec.get("res_mod") else 0
        res = torch.randint(-8, 9, (rows, N), generator=g, device=DEV).float() if integer else torch.randn(rows, N, generator=g, device=DEV)
    return bias, cs, res, res_mod


def run_case(ops, monkeypatch, background, label, expect, env, M, N, K, epis, seed):
    fp16 = ops.OP16 == torch.float16
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    lda, ldw = K + 8 * (1 + K % 3), K + 16
    passes = []
    for integer in (True, False):
        if integer:
            a, w = int_operands(M, N, K, seed)
        else:
            g = torch.Generator(device=DEV).manual_seed(seed + 1)
            a, w = torch.randn(M, K, generator=g, device=DEV), torch.randn(N, K, generator=g, device=DEV) * 0.25
        A, W = nan_padded(M, K, lda, ops.OP16, a), nan_padded(N, K, ldw, ops.OP16, w)
        passes.append((integer, A, W))

    jobs = []   # (name, spec, integer, A, W, bias, cs, residual view, res_mod, canvas)
    for ei, name in enumerate(epis):
        spec = EPI[name]
        for integer, A, W in passes:
            bias, cs, res, res_mod = epilogue_inputs(spec, M, N, seed * 31 + ei, integer)
            resv = None
            if res is not None:                            # ldr = N + 12, NaN in the padding and in two rows below
                dt = torch.float32 if spec["res"] == 32 else ops.OP16
                rb = torch.full((res.shape[0] + 2, N + 12), float("nan"), dtype=dt, device=DEV)
                rb[:res.shape[0], :N] = res.to(dt)
                resv = rb[:res.shape[0], :N]
            cv = Canvas(M, N, torch.float32 if spec["out"] == 32 else ops.OP16, spec.get("aligned", True))
            jobs.append((name, spec, integer, A, W, bias, cs, resv, res_mod, cv))

    def launch(job, out):
        name, spec, integer, A, W, bias, cs, resv, res_mod, cv = job
        if spec.get("nt"):
            monkeypatch.setenv("MSAM2_NT_BYTES", "0")
            monkeypatch.setenv("MSAM2_NT_BYTES_F32", "0")
        ops.gemm(A, W, bias, act=spec.get("act", 0), colscale=cs, residual=resv, res_mod=res_mod, out=out)
        if spec.get("nt"):
            monkeypatch.delenv("MSAM2_NT_BYTES")
            monkeypatch.delenv("MSAM2_NT_BYTES_F32")

    launched = gemm_kernels_launched(lambda: [launch(j, j[-1].view) for j in jobs])
    assert_reached(launched, expect, label)

    lin_cache = {}
    for job in jobs:
        name, spec, integer, A, W, bias, cs, resv, res_mod, cv = job
        what = f"{label} {M}x{N}x{K} {name} ({'integer' if integer else 'random'} pass)"
        assert cv.sentinels_intact(), f"{what}: wrote outside the output view"
        if integer not in lin_cache:
            a64, w64 = A.double(), W.double()
            lin_cache[integer] = (a64 @ w64.t(), a64.abs() @ w64.abs().t())
        lin, S = lin_cache[integer]
        pre = lin + (bias.double() if bias is not None else 0.0)
        act = spec.get("act", 0)
        y = O.gelu(pre) if act == 1 else pre.clamp_min(0) if act == 2 else torch.sigmoid(pre) if act == 3 else pre
        if cs is not None:
            y = y * cs.double()
        if resv is not None:
            r = resv.double()
            y = y + (r[torch.arange(M, device=DEV) % res_mod] if res_mod else r)
        out16 = spec["out"] == 16
        got = cv.view.double()
        if integer and out16:
            assert y.abs().max().item() < 256, f"{what}: test data leaves the exact 16-bit range"
        split = any("zero" in p for p in expect)
        if integer and act in (0, 2):
            bad = got != y
            assert not bad.any(), f"{what}: {int(bad.sum())} outputs differ from the exact result, max |d| {(got - y).abs().nan_to_num(1e30).max().item():.4g}"
        else:
            bound = error_bound(S, K + (K // 32 + 1 if split else 0), pre, y, act=act, colscale=cs.double() if cs is not None else None,
                                out16=out16, fp16=fp16)
            err = (got - y).abs()
            bad = ~(err <= bound)
            assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} outside the bound, worst |d| - bound "
                                   f"{(err - bound).nan_to_num(1e30).max().item():.4g}")

    # reproducibility: once more beside an independent GEMM on a second stream (split-K: its integer pass)
    split = any("zero" in p for p in expect)
    for job in jobs:
        name, spec, integer, *_, cv = job
        if integer != split:
            continue
        first = cv.bits()
        again = Canvas(M, N, cv.buf.dtype, spec.get("aligned", True))
        background()
        launch(job, again.view)
        torch.cuda.synchronize()
        assert torch.equal(again.bits(), first), f"{label} {M}x{N}x{K} {name}: different bits when launched beside another GEMM"


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_gemm_variant(ops, clean_env, background, case):
    label, expect, env, M, N, K, epis = case
    run_case(ops, clean_env, background, label, expect, env, M, N, K, epis, seed=M * 7 + N * 3 + K)


def test_gemm_wstat256_kernel_in_a_child_process():
    """gemm_wstat256_kernel is opt-in (MSAM2_GEMM_WSTAT256=1, read once per process): the default W-stationary cases above through it,
    with the same padding, canaries and reproducibility checks, in a child process"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider", "-k",
                        "test_gemm_variant and gemm_wstat_kernel and not apf"], env=dict(os.environ, MSAM2_GEMM_WSTAT256="1"),
                       capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0 and "4 passed" in r.stdout, (r.stdout + r.stderr)[-2000:]


# ---------------------------------------------------------------------------------------------------------------------------------
# msam2_gemm_rope: (id label, expected kernel, env, batches B, rows per batch L, rows past n_rope n_excl, N, rope_cols, head_dim, K).
# The first is the memory attention's fused key projection of four layers (memory.py: K = mem_dim 64, N = 4 x 256, one head of 256,
# 16 object-pointer tokens per batch left unrotated), on the kernel that default dispatch picks for it.
ROPE_CASES = [
    ("gemm_glds32_kernel-rope", [GLDS32], {}, 2, 528, 16, 1024, 1024, 256, 64),
    ("gemm_kernel<128,128,2,2>-rope", [R128x128], V1, 2, 528, 16, 1024, 1024, 256, 64),
    ("gemm_kernel<128,64,2,2>-rope", [R128x64], {}, 2, 260, 4, 192, 128, 64, 64),
    ("gemm_kernel<128,32,4,1>-rope", [R128x32], {}, 2, 260, 4, 32, 32, 32, 24),
    ("gemm_glds_kernel-rope", [GLDS], var(2), 1, 384, 0, 256, 128, 128, 64),
    ("gemm_wide_kernel-v8-rope", [WIDE[8]], {}, 2, 256, 3, 256, 256, 256, 1024),
]


@pytest.mark.parametrize("case", ROPE_CASES, ids=[f"{c[0]}-{c[3] * c[4]}x{c[6]}x{c[9]}" for c in ROPE_CASES])
def test_gemm_rope_variant(ops, clean_env, background, case):
    label, expect, env, B, L, n_excl, N, cols, D, K = case
    for k, v in env.items():
        clean_env.setenv(k, v)
    fp16 = ops.OP16 == torch.float16
    M, n_rope, side = B * L, L - n_excl, 16
    cos, sin = ops.rope_table(side, D, 10000.0, DEV)
    oc, osn = O.axial_rope_table(D, side, side, 10000.0)
    assert (cos.cpu() - oc).abs().max().item() < 1e-5 and (sin.cpu() - osn).abs().max().item() < 1e-5
    jobs = []
    for integer in (True, False):
        if integer:
            a, w = int_operands(M, N, K, M + N + K)
            bias = torch.randint(-4, 5, (N,), generator=torch.Generator(device=DEV).manual_seed(K), device=DEV).float()
        else:
            g = torch.Generator(device=DEV).manual_seed(M + N)
            a, w = torch.randn(M, K, generator=g, device=DEV), torch.randn(N, K, generator=g, device=DEV) * 0.25
            bias = torch.randn(N, generator=g, device=DEV)
        A, W = nan_padded(M, K, K + 8, ops.OP16, a), nan_padded(N, K, K + 24, ops.OP16, w)
        jobs.append((integer, A, W, bias, Canvas(M, N, ops.OP16, True)))

    def launch(job, out):
        integer, A, W, bias, _ = job
        ops.gemm_rope(A, W, bias, (cos, sin), rope_cols=cols, head_dim=D, rows_per_batch=L, n_rope=n_rope, out=out)

    launched = gemm_kernels_launched(lambda: [launch(j, j[-1].view) for j in jobs])
    assert_reached(launched, expect, label)
    c64, s64 = cos.double(), sin.double()
    pos = torch.arange(n_rope, device=DEV) % cos.shape[0]
    for job in jobs:
        integer, A, W, bias, cv = job
        what = f"{label} B={B} L={L} N={N} K={K} ({'integer' if integer else 'random'} pass)"
        assert cv.sentinels_intact(), f"{what}: wrote outside the output view"
        a64, w64 = A.double(), W.double()
        pre = (a64 @ w64.t() + bias.double()).view(B, L, N)
        S = (a64.abs() @ w64.abs().t()).view(B, L, N)
        e = error_bound(S, K, pre, pre)                                # before the rotation (fp32 accumulator + bias)
        ref, eb = pre.clone(), e.clone()
        for h0 in range(0, cols, D):
            blk = pre[:, :n_rope, h0:h0 + D]
            ref[:, :n_rope, h0:h0 + D] = O.rope_rotate(blk, c64[pos], s64[pos])
            # a rotated pair (x0, x1): |cos|, |sin| <= 1, each output takes both inputs' errors and three fp32 roundings of products / sums
            eblk = e[:, :n_rope, h0:h0 + D]
            pair = eblk[..., 0::2] + eblk[..., 1::2] + 2.0 ** -22 * (blk[..., 0::2].abs() + blk[..., 1::2].abs())
            eb[:, :n_rope, h0:h0 + D] = torch.stack((pair, pair), dim=-1).flatten(-2)
        bound = eb + (2.0 ** -11 if fp16 else 2.0 ** -8) * (ref.abs() + eb) + 2.0 ** -25
        err = (cv.view.double().view(B, L, N) - ref).abs()
        bad = ~(err <= bound)
        assert not bad.any(), f"{what}: {int(bad.sum())} outside the bound, worst |d| - bound {(err - bound).nan_to_num(1e30).max().item():.4g}"
    # reproducibility of the random pass beside an independent GEMM
    job = jobs[1]
    again = Canvas(M, N, ops.OP16, True)
    background()
    launch(job, again.view)
    torch.cuda.synchronize()
    assert torch.equal(again.bits(), job[-1].bits()), f"{label}: different bits when launched beside another GEMM"
