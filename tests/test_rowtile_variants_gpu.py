"""Variant matrix of the full-row GEMM + LayerNorm kernels (GPU): gemm_rowln_kernel<384,0>, <256,0>, <256,64>, <256,256>
(csrc/gemm_rowln.hip) and mlp_rowln_kernel<384,0> (csrc/mlp_rowln.hip) on the tile of csrc/rowtile.h, every instantiation reached on purpose
through its entry, in the style of tests/test_fused_variants_gpu.py:
  * each case names the instantiation it must reach; torch.profiler asserts that exactly that one ran (rowtile_cases.instantiations() is
    compared with a literal list in tests/test_rowtile_cases_cpu.py);
  * every 16-bit operand, R32 and the W matrices lie inside NaN padding with a leading dimension above the row length, every bias and
    LayerNorm vector and the split-KV workspace between guards (the workspace must come back unchanged), C32 and Y16 inside
    sentinel-filled canvases whose sentinels must be bit-identical afterwards;
  * pass 1, exact: operands built so that C32 and Y16 are known to the bit (rowtile_cases: target rows x = m + a s, integers through the
    GEMMs, power-of-two merges) -- compared with == on the bits against values computed from integers in float64, at every row count of
    the table including 1089 (18 workgroups) and 16901 (265: the grid wraps);
  * pass 2, random (the small row counts): float64 references on the GPU from the operand-rounded inputs.  C32 inside error_bound() of
    tests/test_gemm_variants_gpu.py (merged: widened by one 16-bit ulp of each A element times |W|), the MLP inside the family's
    btol(6e-3) + btol(4e-3) |ref|; Y16 inside fused_cases.next_norm_reference around the float64 LayerNorm of the kernel's own C32 rows.
    The worst ratio to every limit is printed ("RATIO ...");
  * token order: out(rows[perm]) == out(rows)[perm] bit for bit for every entry at a ragged M;
  * the null-Y path of msam2_mlp_residual_layernorm_fwd, which the Python wrapper cannot reach, through the C entry.
The 16-bit type is ops.OP16 throughout; the file runs once more in a child process on the bf16 library.
"""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowtile_cases as RC  # noqa: E402
from helpers import ROOT, Canvas, btol, kernels_launched, nan_guarded, nan_padded, op16_is_fp16, reached  # noqa: E402
from test_gemm_variants_gpu import error_bound  # noqa: E402

DEV = "cuda"
F32 = torch.float32
GUARD = 256                    # guard bytes on either side of a workspace


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
    """same_bits that names the first element that went wrong"""
    it = {2: torch.int16, 4: torch.int32}[got.dtype.itemsize]
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    ne = got.contiguous().view(it) != want.contiguous().view(it)
    if bool(ne.any()):
        i = int(ne.flatten().nonzero()[0])
        row, col = divmod(i, got.shape[1])
        rows = ne.any(1).nonzero().flatten()
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} elements in {len(rows)} rows differ in their bits; first at row {row}, "
                             f"column {col}: got {float(got[row, col])}, expected {float(want[row, col])}; rows {rows[:12].tolist()}")


def inside(got, ref, bound, what):
    """|got - ref| <= bound element by element (a NaN fails); prints the worst ratio"""
    d = (got.double() - ref).abs()
    bad = ~(d <= bound)
    print(f"RATIO {what}: {float((d / bound).max()):.4f} (max |err| {float(d.max()):.4g})")
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        row, col = divmod(i, got.shape[1])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; first at row {row}, column {col}: got "
                             f"{float(got[row, col])}, reference {float(ref[row, col])}, bound {float(bound.expand_as(d)[row, col]):.3e}")


class Launch:
    """one launch of a case's entry on the operands E (float64 holders on the device): inputs in NaN padding / between guards, outputs in
    canvases"""

    def __init__(self, ops, E):
        self.ops, self.E, self.kind = ops, E, E["kind"]
        M, N, K, op16 = E["M"], E["N"], E["K"], ops.OP16
        vec = lambda t: None if t is None else nan_guarded(t.to(F32))
        self.c, self.y = Canvas(M, N, F32), Canvas(M, N, op16)                                  # ldc, ldy > N
        self.R = nan_padded(M, N, N + 4, F32, E["R"])                                           # ldr > N
        self.ln_w, self.ln_b, self.b = vec(E["ln_w"]), vec(E["ln_b"]), vec(E["b"])
        self.buf = None
        if self.kind == "mlp":
            self.A = nan_padded(M, N, N + 8, op16, E["A"])                                      # lda > N
            self.W1 = nan_padded(K, N, N + 8, op16, E["W1"])                                    # ldw1 > N
            self.W2 = nan_padded(N, K, K + 16, op16, E["W2"])                                   # ldw2 > H
            self.b1 = vec(E["b1"])
        else:
            self.W = nan_padded(N, K, K + 8, op16, E["W"])                                      # ldw > K
            if self.kind == "plain":
                self.A = nan_padded(M, K, K + 8, op16, E["A"])                                  # lda > K
            else:
                body = RC.workspace_bytes(E, op16)
                assert body.numel() == ops.lib().msam2_attention_workspace_bytes(1, 1, M, K, E["splits"])
                self.buf = torch.full((2 * GUARD + body.numel(),), 0xA5, dtype=torch.uint8, device=DEV)
                self.ws = self.buf[GUARD:GUARD + body.numel()]
                self.ws.copy_(body)
                self.before = self.buf.clone()

    def call(self):
        o, E = self.ops, self.E
        kw = dict(out=self.c.view, out16=self.y.view)
        if self.kind == "plain":
            o.gemm_residual_layernorm(self.A, self.W, self.b, self.R, self.ln_w, self.ln_b, E["eps"], **kw)
        elif self.kind == "merged":
            o.gemm_merged_residual_layernorm(self.ws, E["splits"], E["K"], self.W, self.b, self.R, self.ln_w, self.ln_b, E["eps"], **kw)
        else:
            o.mlp_residual_layernorm(self.A, self.W1, self.b1, self.W2, self.b, self.R, self.ln_w, self.ln_b, E["eps"], **kw)
        return 0

    def call_c(self, L, with_y=True, with_ln=True):
        """the MLP's C entry itself (null Y16 / ln_w / ln_b are the wrapper's blind spot)"""
        E = self.E
        return L.msam2_mlp_residual_layernorm_fwd(p(self.A), self.A.stride(0), p(self.W1), self.W1.stride(0), p(self.b1), p(self.W2), self.W2.stride(0),
                                                  p(self.b), p(self.R), self.R.stride(0), p(self.c.view), self.c.view.stride(0),
                                                  p(self.ln_w) if with_ln else None, p(self.ln_b) if with_ln else None, E["eps"],
                                                  p(self.y.view) if with_y else None, self.y.view.stride(0), E["M"], E["N"], E["K"], stream())

    def check_outside(self):
        torch.cuda.synchronize()
        assert self.c.sentinels_intact() and self.y.sentinels_intact(), "wrote outside an output view (padding columns, or rows past M)"
        assert self.buf is None or torch.equal(self.buf, self.before), "the workspace or its guard bytes changed"

    def run(self, L, expect=None):
        prefix = "mlp_rowln_kernel" if self.kind == "mlp" else "gemm_rowln_kernel"
        if expect is not None:
            reached(L, expect, prefix, [self.call])
        else:
            self.call()
        self.check_outside()
        return self.c.view, self.y.view


def c32_bound(E):
    if E["kind"] == "mlp":
        return btol(6e-3) + btol(4e-3) * E["ref"].abs()
    return error_bound(E["S"], E["K"], E["pre"], E["ref"], fp16=op16_is_fp16()) + E.get("widen", 0.0)


@pytest.mark.parametrize("c", RC.CASES, ids=RC.case_id)
def test_variant(ops, L, c):
    cid = RC.case_id(c)
    # ---- pass 1: exact, and the kernel by name
    E = RC.exact(c, DEV)
    c32, y16 = Launch(ops, E).run(L, expect=c["expect"])
    bits_equal(c32, E["x"].to(F32), f"{cid} exact pass, C32")
    bits_equal(y16, E["y"].to(ops.OP16), f"{cid} exact pass, Y16")
    if c["large"]:
        return
    del E
    # ---- pass 2: random rows against float64
    E = RC.random(c, ops.OP16, DEV)
    c32, y16 = Launch(ops, E).run(L)
    inside(c32, E["ref"], c32_bound(E), f"{cid} C32 vs float64")
    yref, ybound = RC.next_norm_reference(c32, E["ln_w"], E["ln_b"], E["eps"], ops.OP16)
    inside(y16, yref, ybound, f"{cid} Y16 vs the float64 LayerNorm of its own C32 rows")


ORDER_CASES = [RC.case("plain", 384, 384, RC.PERM_M), RC.case("plain", 256, 2048, RC.PERM_M), RC.case("merged", 256, 64, RC.PERM_M, True, 5),
               RC.case("merged", 256, 256, RC.PERM_M, False, 7), RC.case("mlp", 384, 256, RC.PERM_M)]


@pytest.mark.parametrize("c", ORDER_CASES, ids=RC.case_id)
def test_token_order(ops, L, c):
    """a row's arithmetic does not depend on its tile, wave or lane: A, the workspace's rows and R32 permuted alike -> the same rows, permuted"""
    assert RC.case_id(c) in RC.BY_ID and c["M"] % RC.BM
    E = RC.random(c, ops.OP16, DEV)
    c32, y16 = Launch(ops, E).run(L)
    perm = torch.randperm(c["M"], generator=torch.Generator().manual_seed(9)).to(DEV)
    c2, y2 = Launch(ops, RC.permute_rows(E, perm)).run(L, expect=c["expect"])
    bits_equal(c2, c32[perm], f"{RC.case_id(c)} rows permuted, C32")
    bits_equal(y2, y16[perm], f"{RC.case_id(c)} rows permuted, Y16")


@pytest.mark.parametrize("M", [65, 200])
def test_mlp_null_y(ops, L, M):
    """Y16, ln_w and ln_b null: the kernel ends behind the fp32 rows (rowtile_fill_out hands it R32 for the two vectors it never uses)"""
    c = RC.case("mlp", 384, 256, M)
    for kind in ("exact", "random"):
        E = RC.exact(c, DEV) if kind == "exact" else RC.random(c, ops.OP16, DEV)
        with_y = Launch(ops, E)
        assert with_y.call_c(L) == 0, L.msam2_last_error().decode()
        with_y.check_outside()
        run = Launch(ops, E)
        reached(L, c["expect"], "mlp_rowln_kernel", [lambda: run.call_c(L, with_y=False, with_ln=False)])
        run.check_outside()
        assert bool((run.y.buf.view(torch.int16) == run.y.sent).all()), "no Y16 row was asked for"
        bits_equal(run.c.view, with_y.c.view, f"null Y, {kind} operands, M={M}: C32 against the call with Y")
        if kind == "exact":
            bits_equal(run.c.view, E["x"].to(F32), f"null Y, M={M}: C32 exact")
            bits_equal(with_y.y.view, E["y"].to(ops.OP16), f"C entry with Y, M={M}: Y16 exact")
        # Y without its parameters is refused with the entry's message; nothing is launched, nothing written
        bad = Launch(ops, E)

        def refused():
            assert bad.call_c(L, with_y=True, with_ln=False) != 0, "Y16 without ln_w, ln_b: accepted"
        assert kernels_launched(refused, "mlp_rowln_kernel") == set()
        assert L.msam2_last_error().decode() == "mlp_residual_layernorm: LayerNorm rows asked for without ln_w, ln_b"
        bad.check_outside()
        assert bool((bad.c.buf.view(torch.int32) == bad.c.sent).all()) and bool((bad.y.buf.view(torch.int16) == bad.y.sent).all())


def test_same_file_on_the_bf16_library(ops):
    """the operand type is a property of the loaded library: the tests of this file once more in a child process on libmsam2_hip_bf16.so"""
    if os.environ.get("MSAM2_LIB_PATH"):
        assert str(ops.OP16).endswith(os.environ.get("MSAM2_EXPECT_OP16", "")), ops.OP16
        return                                              # this IS a run on a chosen library
    lib = os.path.join(ROOT, "medical-sam2_amd", "libmsam2_hip_bf16.so")
    assert os.path.exists(lib), "libmsam2_hip_bf16.so is built by __graft_entry__.build()"
    env = dict(os.environ, MSAM2_LIB_PATH=lib, MSAM2_EXPECT_OP16="bfloat16", PYTHONUNBUFFERED="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-30:])
    print(tail)
    assert r.returncode == 0 and " passed" in tail and "failed" not in tail, tail
