"""The bf16-operand build of the library (libmsam2_hip_bf16.so, -DMSAM2_OPERAND_BF16; BASELINE.json configs[1] states bf16, and
bench.py's headline line runs on it) through the same parity tests as the fp16 build: a child pytest process with MSAM2_LIB_PATH
pointing at it (the operand type is a property of the loaded library, so it cannot be switched inside one process).

This test is collected LAST and starts the child when it runs: the child has the card to itself (~2.5 minutes; the whole GPU session
stays far inside the driver's 900 s).  With MSAM2_BF16_CHILD_BESIDE=1 the child is started at the BEGINNING of the session instead
(tests/conftest.py: pytest_collection_finish) and runs beside the fp16 tests -- both are mostly host-bound, the box has 16 cores -- which
saves those minutes and was the default until two processes on one card made timing-dependent quantities (atomics-order noise against
its bar; one bit-level mismatch of a re-run launch) part of the verdict (conftest.py has the record).

Tolerances: the e2e tests pick the stated bf16 bars themselves (tests/test_e2e_gpu.py: features 2e-2, logits max 0.3 / mean 0.08, IoU
0.97 per slice / 0.99 pooled -- inside the reference's own fp32-vs-bf16-autocast disagreement); the TIGHT bar
(one value for fp16 and bf16, against the operand-rounding oracle on equal inputs) is in tests/test_modules_gpu.py."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "medical-sam2_amd", "libmsam2_hip_bf16.so")
LOG = os.path.join(ROOT, "gpurun_out", "bf16_suite.log")
# What the bf16 library re-runs: every single-process parity file -- kernels, the GEMM, attention, pointwise, backward and fused-kernel variant matrices (with the
# feature tests of the stage 1-2 fused kernels), modules (incl. the tighter
# operand-rounding comparison), end to end (incl. the 28-slice bank chain and the 64-slice volume at size), the unit-round-off scaling test,
# properties, graphs, backward, gradient goldens, BPTT, the autograd bridge, the captured training step.  Left to the fp16 run only: the
# 512-slice volume (half a minute of CPU oracle that would compete with the fp16 session's own) and the multi-process files, which spawn
# their own children.
FILES = ["tests/test_kernels_gpu.py", "tests/test_gemm_variants_gpu.py", "tests/test_attention_variants_gpu.py", "tests/test_pointwise_variants_gpu.py",
         "tests/test_backward_variants_gpu.py", "tests/test_attention_bwd_variants_gpu.py", "tests/test_fused_variants_gpu.py",
         "tests/test_window_qkv_attention_gpu.py", "tests/test_proj_mlp_fused_gpu.py",
         "tests/test_modules_gpu.py",
         "tests/test_e2e_gpu.py", "tests/test_operand_rounding_gpu.py", "tests/test_properties_gpu.py", "tests/test_graphs_gpu.py", "tests/test_eval_seg.py",
         "tests/test_backward_gpu.py", "tests/test_backward_encoder_gpu.py", "tests/test_grads_golden.py", "tests/test_bptt_gpu.py",
         "tests/test_autograd_gpu.py", "tests/test_train_graph_gpu.py"]
SKIP = "not 512_slices"


def start_child():
    """the child suite as a background process; its output goes straight into gpurun_out/bf16_suite.log, which GROWS while it runs (a
    harness that watches for progress sees it)"""
    assert os.path.exists(LIB), "libmsam2_hip_bf16.so is built by __graft_entry__.build()"
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    env = dict(os.environ, MSAM2_LIB_PATH=LIB, MSAM2_E2E_REPORT="gpurun_out/e2e_report_bf16.json", PYTHONUNBUFFERED="1", MSAM2_BF16_CHILD="1",
               MSAM2_EXPECT_OP16="bfloat16")        # tests/conftest.py refuses to run the child on a library of another operand type
    f = open(LOG, "w")
    return subprocess.Popen([sys.executable, "-u", "-m", "pytest", *FILES, "-q", "-m", "gpu", "-k", SKIP, "--durations=15", "-p", "no:cacheprovider"],
                            cwd=ROOT, env=env, stdout=f, stderr=subprocess.STDOUT)


def test_bf16_build_passes_the_parity_suite(request):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    child = getattr(request.config, "_msam2_bf16_child", None) or start_child()
    rc = child.wait(timeout=3000)
    out = open(LOG).read()
    tail = "\n".join(out.splitlines()[-40:])
    print(tail)
    assert rc == 0, tail
    last = [l for l in out.splitlines() if l.strip()][-1]
    assert " passed" in last and "failed" not in last, tail
