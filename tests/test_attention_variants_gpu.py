"""Attention kernel-variant matrix (GPU): every forward kernel behind msam2_attention_fwd / _fwd_lse, msam2_attention_kv64_fwd / _partial /
_dyn_fwd / _dyn_partial, msam2_window_attention_fwd and msam2_attention_small_fwd (csrc/attention.hip) reached on purpose -- through its
shape and the MSAM2_* switches -- and checked at its edges.  The tables, operand builders, bounds and the proof that the passes can fail
are in tests/attention_cases.py and tests/test_attention_cases_cpu.py.

Each case names the kernel(s) it must reach; torch.profiler asserts that exactly those attn_* kernels ran, so that a change of a dispatch
predicate cannot move the coverage to another kernel silently.  Per case:
  * q / k / v are views inside NaN-filled buffers (row pitch > D, rows past Lq / Lk, and for a device-side key count the rows past it): a
    kernel that uses any padding element returns NaN; the output is a view inside a sentinel-filled buffer that must be bit-identical
    outside the view afterwards (so must the fp32 words behind the log-sum-exp rows);
  * selection pass: integer operands that make every query pick exactly one key (score margin 40 bits), targets on every tile, stage and
    split edge: the output is that key's V row; a wrong key, channel, query row, tile or split moves an element by >= 1 against a bound
    below 0.37 (bf16) / 0.05 (fp16) -- attention_cases.integer_bound().  Bit for bit where the arithmetic is exact (the fp32
    attention_small kernels with fp16 operands);
  * tie pass: pairs of keys share a K row, their queries return the mean of the two V rows: a key counted twice, a split weighted wrongly
    by the merge, O not rescaled when the running maximum moves, a padded window token masked out or read as zeros;
  * random pass: randn operands with one key far above the rest in a late tile, every element within attention_error_bound() of the
    float64 softmax attention of the operand-rounded inputs (torch on the GPU, chunked over queries); log-sum-exp rows within lse_bound();
  * reproducibility: the random pass launched once more beside an independent launch on a second stream gives the same bits; so do the
    deferred merge, the kv64 partial launches + attention_merge, and a device-side key count equal to the capacity against the fused /
    host-count call.
MSAM2_G96_V1, MSAM2_G96_X2 and MSAM2_KV64_V1 are read once per process: their cases run in one child process each, one after the other,
where the same profiler check asserts the switched kernel."""
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_cases as AC  # noqa: E402
from helpers import SENT32, Canvas, kernels_launched, nan_padded  # noqa: E402

DEV = "cuda"
SWITCHES = ("MSAM2_ATTN_V1", "MSAM2_WIN_V1", "MSAM2_NO_TINYWIN", "MSAM2_TINYWIN_64", "MSAM2_NO_FEWQ16")
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import medical_sam2_amd.ops as ops_mod
    return ops_mod


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


@pytest.fixture
def clean_env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def assert_reached(launched, expect, what):
    assert launched, f"{what}: the profiler saw no attention kernel"
    for pat in expect:
        assert any(re.fullmatch(pat, k) for k in launched), f"{what}: expected {pat}, launched {sorted(launched)}"
    stray = [k for k in launched if not any(re.fullmatch(pat, k) for pat in expect)]
    assert not stray, f"{what}: other attention kernels ran: {stray} (expected only {expect})"


# ---------------------------------------------------------------------------------------------------------------------------------
# laying a problem out for its entry point
def padded4(t, dtype, layout, cap=None):
    """t [B, H, L, D] as a view of a NaN-filled buffer: its own buffer with 5 more rows (`cap` rows for a device-side key count) and a
    pitch of D + 8, or -- "pitch", H = 1 -- rows of D + 64 elements with the operand at element 64"""
    B, H, L, D = t.shape
    rows = max(cap or 0, L) + 5
    if layout == "pitch":
        buf = torch.full((B, rows, D + 64), NAN, dtype=dtype, device=DEV)
        buf[:, :L, 64:] = t[:, 0].to(dtype)
        return buf[:, :cap or L, 64:].unsqueeze(1)
    buf = torch.full((B, H, rows, D + 8), NAN, dtype=dtype, device=DEV)
    buf[:, :, :L, :D] = t.to(dtype)
    return buf[:, :, :cap or L, :D]


class Job:
    """one pass of one case: operands laid out, an output canvas, launch() and result() (the output in instance form)"""

    def __init__(self, ops, c, P):
        self.ops, self.c, self.P = ops, c, P
        dt, e = ops.OP16, c["entry"]
        B, H, Lq, D, Dv = c["B"], c["H"], c["Lq"], c["D"], c["Dv"]
        self.lse = None
        if e in ("fwd", "kv64"):
            if c["layout"] == "packed":
                buf = torch.full((B, Lq + 5, 3, H, D), NAN, dtype=dt, device=DEV)
                for i, t in enumerate((P.q, P.k, P.v)):
                    buf[:, :Lq, i] = t.permute(0, 2, 1, 3).to(dt)
                self.q, self.k, self.v = (buf[:, :Lq, i].permute(0, 2, 1, 3) for i in range(3))
            else:
                cap = c["Lk"] if c["dyn"] else None
                self.q = padded4(P.q, dt, "plain")
                self.k, self.v = padded4(P.k, dt, c["layout"], cap), padded4(P.v, dt, c["layout"], cap)
            self.count = torch.tensor([c["dyn"]], dtype=torch.int32, device=DEV) if c["dyn"] else None
            if c["lse"]:
                self.lse_buf = torch.full((B * H * Lq + 16,), 0.0, device=DEV)
                self.lse_buf.view(torch.int32).fill_(SENT32)
                self.lse = self.lse_buf[:B * H * Lq].view(B, H, Lq)
        elif e == "window":
            self.geom()
        else:
            flat = lambda t: t.permute(0, 2, 1, 3).reshape(B * t.shape[2], H * t.shape[3])
            self.q, self.k, self.v = (nan_padded(B * t.shape[2], H * t.shape[3], H * t.shape[3] + 8, dt, flat(t)).unflatten(0, (B, t.shape[2]))
                                      for t in (P.q, P.k, P.v))
        self.canvas = self.new_canvas()

    def geom(self):
        c, P, dt = self.c, self.P, self.ops.OP16
        B, Hh, Ww, heads, ws, D = c["B"], c["Hh"], c["Ww"], c["heads"], c["ws"], c["D"]
        self.wq = ws // 2 if c["pool"] else ws
        self.hq, self.wqi = (Hh // 2, Ww // 2) if c["pool"] else (Hh, Ww)

        def image(t, w, h_img, w_img):                          # [W, heads, w * w, D] -> [B * h_img * w_img, heads * D]
            nwy, nwx = -(-h_img // w), -(-w_img // w)
            x = t.permute(0, 2, 1, 3).reshape(B, nwy, nwx, w, w, heads * D).permute(0, 1, 3, 2, 4, 5).reshape(B, nwy * w, nwx * w, heads * D)
            return x[:, :h_img, :w_img].reshape(B * h_img * w_img, heads * D)
        kimg, vimg = image(P.k, ws, Hh, Ww), image(P.v, ws, Hh, Ww)
        qimg = image(P.q, self.wq, self.hq, self.wqi)
        qfull = qimg if not c["pool"] else torch.full_like(kimg, NAN)       # the q columns of a q-pooled call are not read
        self.qkv = nan_padded(B * Hh * Ww, 3 * heads * D, 3 * heads * D + 8, dt, torch.cat((qfull, kimg, vimg), 1))
        self.qp = nan_padded(qimg.shape[0], heads * D, heads * D + 8, dt, qimg) if c["pool"] else None
        self.bias = torch.cat((torch.full((heads * D,), NAN, dtype=torch.float64, device=DEV), P.kbias.flatten(), P.vbias.flatten())).float()

    def new_canvas(self):
        c = self.c
        if c["entry"] == "window":
            return Canvas(c["B"] * self.hq * self.wqi, c["heads"] * c["D"], self.ops.OP16)
        return Canvas(c["B"] * c["Lq"], c["H"] * c["Dv"], self.ops.OP16)

    def out_view(self, cv):
        c = self.c
        if c["entry"] in ("fwd", "kv64"):
            return cv.view.unflatten(1, (c["H"], c["Dv"])).unflatten(0, (c["B"], c["Lq"])).permute(0, 2, 1, 3)
        if c["entry"] == "small":
            return cv.view.unflatten(0, (c["B"], c["Lq"]))
        return cv.view

    def launch(self, cv=None, mode="fused", workspace=None):
        """mode "fused": the case's own call; "defer": the split pass + attention_merge; "partial": kv64 _partial over the case's
        sub-ranges + attention_merge; "host": a device-side key count replaced by the host-side call on the same keys"""
        ops, c = self.ops, self.c
        out = self.out_view(cv or self.canvas)
        if c["entry"] == "fwd":
            if mode == "defer":
                ws = ops.attention_workspace(c["B"], c["H"], c["Lq"], c["D"], c["splits"], DEV)
                ops.attention(self.q, self.k, self.v, splits=c["splits"], out=out, workspace=ws, defer_merge=True)
                return ops.attention_merge(out, c["Lk"], c["splits"], ws)
            return ops.attention(self.q, self.k, self.v, splits=c["splits"], out=out, lse=self.lse)
        if c["entry"] == "kv64":
            count = None if mode == "host" else self.count
            if mode in ("defer", "partial"):
                ws = ops.attention_workspace(c["B"], c["H"], c["Lq"], 64, c["eff"], DEV)
                if mode == "defer":
                    ops.attention_kv64(self.q, self.k, self.v, splits=c["splits"], out=out, workspace=ws, defer_merge=True, key_count=count)
                else:
                    begin = 0
                    for n in c["partial"]:
                        ops.attention_kv64_partial(self.q, self.k, self.v, splits=c["eff"], split_begin=begin, split_count=n, workspace=ws,
                                                   key_count=count)
                        begin += n
                    assert begin == c["eff"]
                return ops.attention_merge(out, c["Lk"], c["eff"], ws)
            return ops.attention_kv64(self.q, self.k, self.v, splits=c["splits"], out=out, key_count=count)
        if c["entry"] == "window":
            return ops.window_attention(self.qkv, c["B"], c["Hh"], c["Ww"], c["heads"], c["ws"], self.bias, q_pooled=self.qp, out=out)
        return ops.attention_small(self.q, self.k, self.v, c["H"], out=out)

    def result(self, cv=None):
        c, cv = self.c, cv or self.canvas
        if c["entry"] != "window":
            o = self.out_view(cv).double()
            return o if c["entry"] != "small" else o.unflatten(2, (c["H"], c["Dv"])).permute(0, 2, 1, 3)
        B, heads, D, w = c["B"], c["heads"], c["D"], self.wq
        img = cv.view.double().reshape(B, self.hq, self.wqi, heads * D)
        nwy, nwx = -(-self.hq // w), -(-self.wqi // w)
        img = torch.nn.functional.pad(img, (0, 0, 0, nwx * w - self.wqi, 0, nwy * w - self.hq))
        x = img.reshape(B, nwy, w, nwx, w, heads, D).permute(0, 1, 3, 5, 2, 4, 6)
        return x.reshape(B * nwy * nwx, heads, w * w, D)


def run_case(ops, monkeypatch, background, c):
    fp16 = ops.OP16 == torch.float16
    what = AC.case_id(c)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    jobs = {kind: Job(ops, c, AC.build(c, kind, device=DEV, op16=ops.OP16)) for kind in ("sel", "tie", "rand")}
    mode = "partial" if c.get("partial") else "fused"

    launched = kernels_launched(lambda: [j.launch(mode=mode) for j in jobs.values()], "attn_")
    assert_reached(launched, c["expect"], what)

    split = c["eff"] > 1
    for kind, job in jobs.items():
        P = job.P
        assert job.canvas.sentinels_intact(), f"{what} {kind}: wrote outside the output view"
        got = job.result()
        valid = P.q_valid[:, None, :, None]
        ref, A, smax, lse = AC.reference(P.q, P.k, P.v, P.c)
        if kind == "rand":
            bound = AC.attention_error_bound(ref, A, smax, c["keys"], c["D"], P.c, fp16=fp16, mref=c["mref"], split=split, p16=c["p16"])
        else:
            assert ((ref - P.expected).abs() * valid).max().item() < 1e-6
            ref = P.expected
            bound = AC.integer_bound(ref, P.A, c["keys"], split, fp16, P.vmax)
            if kind == "sel" and fp16 and not c["p16"]:
                bound = torch.zeros_like(bound)                              # fp32 arithmetic, p = 1: exact
        err = (got - ref).abs()
        bad = ~(err <= bound) & valid
        print(f"{what} {kind}: max err {(err * valid).nan_to_num(1e30).max().item():.4g}, max err / bound "
              f"{(err / bound.clamp_min(1e-30) * valid).nan_to_num(1e30).max().item():.3g}")
        assert not bad.any(), (f"{what} {kind}: {int(bad.sum())} of {bad.numel()} outside the bound, worst |d| - bound "
                               f"{((err - bound) * valid).nan_to_num(1e30).max().item():.4g}, first at {bad.nonzero()[0].tolist()}")
        if job.lse is not None:
            assert (job.lse_buf[job.lse.numel():].view(torch.int32) == SENT32).all(), f"{what} {kind}: wrote behind the lse rows"
            lb = AC.lse_bound(lse, smax, c["D"], P.c, fp16, c["mref"])
            le = (job.lse.double() - lse).abs()
            print(f"{what} {kind}: lse max err {le.nan_to_num(1e30).max().item():.4g}, max err / bound {(le / lb).nan_to_num(1e30).max().item():.3g}")
            assert (le <= lb).all(), f"{what} {kind}: lse off by {le.nan_to_num(1e30).max().item():.4g}, bound there {lb.flatten()[le.nan_to_num(1e30).argmax()].item():.4g}"

    # reproducibility: the random pass once more beside an independent launch; the other ways to the same result
    job = jobs["rand"]
    first = job.canvas.bits()
    again = job.new_canvas()
    background()
    job.launch(again, mode=mode)
    torch.cuda.synchronize()
    assert torch.equal(again.bits(), first), f"{what}: different bits when launched beside another kernel"
    others = (["fused"] if mode == "partial" else []) + (["defer"] if c.get("defer") else []) + (
        ["host"] if c.get("dyn") == c["Lk"] and mode == "fused" else [])
    for m in others:
        for kind in ("rand", "tie"):
            cv = jobs[kind].new_canvas()
            jobs[kind].launch(cv, mode=m)
            assert torch.equal(cv.bits(), jobs[kind].canvas.bits()), f"{what} {kind}: the {m} call gives other bits than the {mode} one"


@pytest.mark.parametrize("case", AC.CASES, ids=[AC.case_id(c) for c in AC.CASES])
def test_attention_variant(ops, clean_env, background, case):
    run_case(ops, clean_env, background, case)


@pytest.mark.parametrize("case", AC.WINDOW_CASES, ids=[AC.case_id(c) for c in AC.WINDOW_CASES])
def test_window_attention_variant(ops, clean_env, background, case):
    run_case(ops, clean_env, background, case)


@pytest.mark.parametrize("case", AC.SMALL_CASES, ids=[AC.case_id(c) for c in AC.SMALL_CASES])
def test_attention_small_variant(ops, clean_env, background, case):
    run_case(ops, clean_env, background, case)


# (switch, -k expression, cases it must run): the switched kernel is asserted inside the child by the cases' own `expect`
# (attention_cases.G96 / KVX2 follow the environment)
CHILDREN = [
    ("MSAM2_G96_V1", "test_attention_variant and fwd- and x96-", sum(1 for c in AC.CASES if c["D"] == 96)),
    ("MSAM2_G96_X2", "test_attention_variant and fwd- and x96-", sum(1 for c in AC.CASES if c["D"] == 96)),
    ("MSAM2_KV64_V1", "test_attention_variant and kv64-", sum(1 for c in AC.CASES if c["entry"] == "kv64")),
]


@pytest.mark.parametrize("switch,select,count", CHILDREN, ids=[c[0] for c in CHILDREN])
def test_once_per_process_switches_in_a_child_process(switch, select, count):
    """attn_glds_kernel<96,128,4,3> at >= 256 queries (MSAM2_G96_V1), attn_g96x2_kernel<2,4> (MSAM2_G96_X2) and attn_kv64_kernel at >= 256
    queries (MSAM2_KV64_V1) on the cases of the default kernels"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider", "-k", select],
                       env={**os.environ, switch: "1"}, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0 and f"{count} passed" in r.stdout, (r.stdout + r.stderr)[-3000:]
