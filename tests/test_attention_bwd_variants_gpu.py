"""Attention-backward kernel-variant matrix (GPU): the 77 kernel instantiations of csrc/attention_bwd.hip -- attn_bwd_kernel<D, NW, ROLE, DROP>
(48), attn_bwd_dma_kernel (24), attn_bwd_prep_kernel<D> (4), attn_bwd_reduce_kernel -- reached on purpose through the C entries
msam2_attention_bwd / msam2_attention_bwd_dropout and checked at their edges.  Tables, builders, the float64 reference, the derived bound
and the proof that the passes can fail are in tests/attention_bwd_cases.py and tests/test_attention_bwd_cases_cpu.py.

Per case:
  * torch.profiler asserts that exactly the case's attn_bwd* kernels ran (attention_bwd_cases.expected_kernels, a restatement of
    launch_fill / dq_key_splits), so a change of a dispatch rule cannot move the coverage silently;
  * o and lse are computed in float64 from the operand-rounded q, k, v (with the host-reproduced dropout mask), so the kernels are
    held to their own contract and the forward can neither cause nor hide a failure (test_backward_of_the_projects_own_forward feeds
    attention_forward_lse's results instead, once per head dim);
  * q, k, v, o are views inside NaN-filled buffers (row pitch D + 8, 5 rows past L, unpacked batch / head strides; "token" cases: [B, H,
    L, D] views of token-major [B, L, H D] buffers), dO an fp32 view of pitch D + 4 in a NaN-filled buffer, lse exactly [B, H, Lq] with
    NaN words behind it; dq, dk, dv are fp32 views of pitch D + 4 with extra rows in sentinel-filled buffers ("token" cases: the three
    column thirds of one [B, L, 3 H D] buffer) that must be bit-identical outside the views afterwards; the workspace is exactly
    msam2_attention_bwd_workspace_bytes long, pre-filled with NaN (a partial-dQ slot that the reduction reads but nobody wrote shows up)
    and sits between two 256-byte guards that must be intact; no output may hold a NaN;
  * the selection, tie and bounded passes of the case module: bit for bit where the arithmetic is exact, every element within
    attention_bwd_error_bound() otherwise;
  * the bounded pass launched once more beside an independent attention launch on a second stream gives the same bits ("no atomics
    anywhere"); in the dropout cases this second launch passes part of the seed on the device.
For D = 128 / 256 the default process reaches attn_bwd_dma_kernel; MSAM2_BWD_NO_DMA is read once per process, so the register-staged
attn_bwd_kernel<128 / 256, ..> run in one child process per head dim, with the same profiler assertion inside the child.

Left out on purpose: the fall-back from the DMA kernel to attn_bwd_kernel when max(Lq, Lk) * row pitch * 2 >= 2^31 bytes.  It needs a
2 GiB operand view and selects kernels that the switch already covers."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_bwd_cases as AB  # noqa: E402
from attention_cases import LOG2E, lse_bound  # noqa: E402
from helpers import SENT32, K, kernels_launched, op16_is_fp16, same_bits, within  # noqa: E402,F401

DEV = "cuda"
NAN = float("nan")
IDS = [AB.case_id(c) for c in AB.CASES]
NOT_REACHED = {}                      # kernel key -> why no case reaches it


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import medical_sam2_amd.ops as ops_mod
    return ops_mod


@pytest.fixture(scope="module")
def L(ops):
    from medical_sam2_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def background(ops):
    """an independent attention launch (2 x 4 heads, 1024 x 1024, D = 128: all CUs busy for tens of microseconds) for a second stream"""
    g = torch.Generator(device=DEV).manual_seed(99)
    q, k, v = (torch.randn(2, 4, 1024, 128, generator=g, device=DEV).to(ops.OP16) for _ in range(3))
    o = torch.empty(2, 1024, 4, 128, dtype=ops.OP16, device=DEV).permute(0, 2, 1, 3)
    s2 = torch.cuda.Stream()
    s2.wait_stream(torch.cuda.current_stream())

    def launch():
        with torch.cuda.stream(s2):
            ops.attention(q, k, v, out=o)
    return launch


def assert_reached(launched, expect, what):
    assert launched == set(expect), f"{what}: expected {sorted(expect)}, launched {sorted(launched)}"


# ---------------------------------------------------------------------------------------------------------------------------------
def lay16(t, dt, layout):
    """t [B, H, L, D] as a view of a NaN-filled 16-bit buffer with 5 more rows and 8 more elements per row"""
    B, H, Ln, D = t.shape
    if layout == "token":
        buf = torch.full((B, Ln + 5, H * D + 8), NAN, dtype=dt, device=DEV)
        buf[:, :Ln, :H * D] = t.permute(0, 2, 1, 3).reshape(B, Ln, H * D).to(dt)
        return buf[:, :Ln, :H * D].unflatten(2, (H, D)).permute(0, 2, 1, 3)
    buf = torch.full((B, H, Ln + 5, D + 8), NAN, dtype=dt, device=DEV)
    buf[:, :, :Ln, :D] = t.to(dt)
    return buf[:, :, :Ln, :D]


class Outputs:
    """dq, dk, dv as fp32 views inside SENT32-filled buffers"""

    def __init__(self, c):
        B, H, Lq, Lk, D = c["B"], c["H"], c["Lq"], c["Lk"], c["D"]
        if c["layout"] == "token":
            shape = (B, max(Lq, Lk) + 3, 3 * H * D + 4)
            views = lambda b: [b[:, :Ln, i * H * D:(i + 1) * H * D].unflatten(2, (H, D)).permute(0, 2, 1, 3) for i, Ln in enumerate((Lq, Lk, Lk))]
            self.bufs = [torch.empty(shape, device=DEV)]
            masks = [torch.zeros(shape, dtype=torch.bool, device=DEV)]
            self.dq, self.dk, self.dv = views(self.bufs[0])
            for m in views(masks[0]):
                m.fill_(True)
        else:
            self.bufs, masks, vs = [], [], []
            for Ln in (Lq, Lk, Lk):
                b = torch.empty(B, H, Ln + 6, D + 4, device=DEV)
                m = torch.zeros(b.shape, dtype=torch.bool, device=DEV)
                m[:, :, 3:3 + Ln, :D] = True
                self.bufs.append(b)
                masks.append(m)
                vs.append(b[:, :, 3:3 + Ln, :D])
            self.dq, self.dk, self.dv = vs
        for b in self.bufs:
            b.view(torch.int32).fill_(SENT32)
        self.outside = [~m for m in masks]

    def intact(self):
        return all(bool((b.view(torch.int32)[o] == SENT32).all()) for b, o in zip(self.bufs, self.outside))

    def untouched(self):
        return all(bool((b.view(torch.int32) == SENT32).all()) for b in self.bufs)

    def get(self):
        return dict(dq=self.dq, dk=self.dk, dv=self.dv)


class Workspace:
    G = 256

    def __init__(self, L, c):
        self.n = L.msam2_attention_bwd_workspace_bytes(c["B"], c["H"], c["Lq"], c["D"])
        assert self.n == AB.workspace_bytes(c["B"], c["H"], c["Lq"], c["D"])
        self.buf = torch.full((self.n + 2 * self.G,), 0xFF, dtype=torch.uint8, device=DEV)          # 0xFF..: NaN in fp32 and in both 16-bit types
        self.buf[:self.G] = 0xA5
        self.buf[self.G + self.n:] = 0xA5
        self.ptr = self.buf[self.G:].data_ptr()
        assert self.ptr % 16 == 0

    def intact(self):
        return bool((self.buf[:self.G] == 0xA5).all()) and bool((self.buf[self.G + self.n:] == 0xA5).all())


class Job:
    """one pass of one case: the operands laid out for the entry, outputs and workspace between their guards"""

    def __init__(self, L, ops, c, X, lse=None):
        self.L, self.ops, self.c, self.X = L, ops, c, X
        B, H, Lq = c["B"], c["H"], c["Lq"]
        dt = ops.OP16
        self.q, self.k, self.v, self.o = (lay16(t, dt, c["layout"]) for t in (X.q, X.k, X.v, X.o))
        gbuf = torch.full((B, H, Lq + 5, c["D"] + 4), NAN, device=DEV)
        gbuf[:, :, :Lq, :c["D"]] = X.g.float()
        self.g = gbuf[:, :, :Lq, :c["D"]]
        self.lse_buf = torch.full((B * H * Lq + 16,), NAN, device=DEV)
        self.lse_buf[:B * H * Lq] = (X.lse if lse is None else lse).float().flatten()
        self.seed_dev = torch.tensor([AB.SEED_DEV], dtype=torch.int64, device=DEV)
        self.out, self.ws = Outputs(c), Workspace(L, c)

    def launch(self, out=None, ws=None, split_seed=False, short=0):
        c, s3, out, ws = self.c, self.ops._strides3, out or self.out, ws or self.ws
        a = []
        for t in (self.q, self.k, self.v, self.o):
            a += [t.data_ptr(), s3(t)]
        a += [self.lse_buf.data_ptr(), self.g.data_ptr(), s3(self.g)]
        for t in (out.dq, out.dk, out.dv):
            a += [t.data_ptr(), s3(t)]
        a += [ws.ptr, ws.n - short, c["B"], c["H"], c["Lq"], c["Lk"], c["D"], self.X.scale]
        stream = torch.cuda.current_stream().cuda_stream
        if c["p"]:
            seed, dev = (AB.SEED - AB.SEED_DEV, self.seed_dev.data_ptr()) if split_seed else (AB.SEED, None)
            return self.L.msam2_attention_bwd_dropout(*a, c["p"], seed, AB.OFFSET, dev, stream)
        return self.L.msam2_attention_bwd(*a, stream)


def check(job, what, fp16, extra_de=None):
    X, kind = job.X, job.X.kind
    assert job.out.intact(), f"{what}: wrote outside an output view"
    assert job.ws.intact(), f"{what}: wrote outside the workspace"
    got = {n: t.double() for n, t in job.out.get().items()}
    ref, bound = AB.reference(X), AB.attention_bwd_error_bound(X, fp16, extra_de)
    for n in ("dq", "dk", "dv"):
        err = (got[n] - ref[n]).abs()
        print(f"{what} {n}: max err {float(err.nan_to_num(1e30).max()):.4g}, max err / bound {float((err / bound[n].clamp_min(1e-300)).nan_to_num(1e30).max()):.3g}")
    for n in ("dq", "dk", "dv"):
        assert bool(torch.isfinite(got[n]).all()), f"{what}: {int((~torch.isfinite(got[n])).sum())} non-finite elements in {n}"
        within(got[n], ref[n], bound[n], f"{what} {n}")
    if kind != "rand":
        slack = AB.int_slack(X, fp16)
        for n in ("dv",) if kind == "sel" else ("dq", "dk", "dv"):
            exp = getattr(X, "exp_" + n)
            if fp16:
                same_bits(got[n].float() + 0.0, exp.float() + 0.0, f"{what} {n} against its closed form")         # (+ 0.0: -0 is 0)
            else:
                within(got[n], exp, slack[n], f"{what} {n} against its closed form")


def run_case(L, ops, background, c):
    fp16, what = op16_is_fp16(), AB.case_id(c)
    jobs = {kind: Job(L, ops, c, AB.build(c, kind, device=DEV, op16=ops.OP16)) for kind in c["passes"]}

    def go():
        for j in jobs.values():
            rc = j.launch()
            assert rc == 0, L.msam2_last_error().decode()
    assert_reached(kernels_launched(go, "attn_bwd"), AB.expected_kernels(c, AB.NO_DMA), what)
    for kind, job in jobs.items():
        check(job, f"{what} {kind}", fp16)
    # reproducibility: the bounded pass once more beside an independent launch (dropout: part of the seed on the device)
    job = jobs["rand"]
    again, ws2 = Outputs(c), Workspace(L, c)
    background()
    assert job.launch(again, ws2, split_seed=True) == 0, L.msam2_last_error().decode()
    torch.cuda.synchronize()
    assert ws2.intact()
    for a, b in zip(again.bufs, job.out.bufs):
        same_bits(a, b, f"{what}: launched beside another kernel")


@pytest.mark.parametrize("case", AB.CASES, ids=IDS)
def test_attention_bwd_variant(L, ops, background, case):
    run_case(L, ops, background, case)


@pytest.mark.parametrize("D", AB.ALL_D)
def test_backward_of_the_projects_own_forward(L, ops, D):
    """o and lse from attention_forward_lse instead of float64: the same bound with the forward's lse_bound added to the score error"""
    from medical_sam2_amd import backward
    c = next(c for c in AB.CASES if c["name"] == "C1" and c["D"] == D)
    fp16 = op16_is_fp16()
    X = AB.build(c, "rand", device=DEV, op16=ops.OP16)
    q, k, v = (lay16(t, ops.OP16, "plain") for t in (X.q, X.k, X.v))
    o, lse = backward.attention_forward_lse(q, k, v, X.scale)
    smax = (X.q.abs() @ X.k.abs().transpose(2, 3)).max(-1, keepdim=True).values
    lb = lse_bound(X.lse_true, smax, D, X.scale * LOG2E, fp16, False)
    within(lse, X.lse_true, lb, f"forward lse D={D}")
    X.o, X.lse = o.double(), X.lse_true                     # the reference: the forward's o (delta), the true lse (P)
    job = Job(L, ops, c, X, lse=lse)
    assert job.launch() == 0, L.msam2_last_error().decode()
    check(job, f"own forward D={D}", fp16, extra_de=lb)


@pytest.mark.parametrize("D", AB.ALL_D)
def test_short_workspace_is_refused_without_a_launch(L, ops, D):
    for p in (0.0, 0.5):
        c = next(c for c in AB.CASES if c["name"] == ("C9C2" if p else "C2") and c["D"] == D and c["p"] == p)
        job = Job(L, ops, c, AB.build(c, "rand", device=DEV, op16=ops.OP16))
        rcs = []
        launched = kernels_launched(lambda: rcs.append(job.launch(short=1)), "attn_bwd")
        assert rcs == [-1] and b"workspace too small" in L.msam2_last_error(), (rcs, L.msam2_last_error())
        assert launched == set(), launched
        assert job.out.untouched() and job.ws.intact() and bool((job.ws.buf[job.ws.G:job.ws.G + job.ws.n] == 0xFF).all())
        assert job.launch() == 0


def test_every_instantiation_has_a_case():
    want = ([f"attn_bwd_kernel<{D},{NW},{R},{dr}>" for D in (64, 96, 128, 256) for NW in (2, 4) for R in (0, 1, 2) for dr in ("false", "true")] +
            [f"attn_bwd_dma_kernel<{D},{NW},{R},{dr}>" for D in (128, 256) for NW in (2, 4) for R in (0, 1, 2) for dr in ("false", "true")] +
            ["attn_bwd_prep_kernel<64>", "attn_bwd_prep_kernel<96>", "attn_bwd_prep_kernel<128>", "attn_bwd_prep_kernel<256>", "attn_bwd_reduce_kernel"])
    assert len(want) == 77
    have = {k for c in AB.CASES for k in AB.expected_kernels(c, False)} | {k for c in AB.CASES if c["D"] in CHILD_DS for k in AB.expected_kernels(c, True)}
    assert have | set(NOT_REACHED) == set(want) and not have & set(NOT_REACHED), sorted(set(want) ^ have)


CHILD_DS = (128, 256)


@pytest.mark.parametrize("D", CHILD_DS)
def test_register_staged_kernels_of_the_dma_head_dims_in_a_child_process(D):
    """attn_bwd_kernel<128 / 256, ..> (MSAM2_BWD_NO_DMA=1, read once per process) on the cases of the DMA kernels"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    count = sum(1 for c in AB.CASES if c["D"] == D)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider", "-k",
                        f"test_attention_bwd_variant and D{D}-"], env={**os.environ, "MSAM2_BWD_NO_DMA": "1"}, capture_output=True, text=True,
                       timeout=600, cwd=root)
    assert r.returncode == 0 and f"{count} passed" in r.stdout, (r.stdout + r.stderr)[-3000:]
