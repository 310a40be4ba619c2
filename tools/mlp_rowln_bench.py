#!/usr/bin/env python3
"""The stage-3 MLP with its residual add and the next LayerNorm at the benchmark's shape (B = 4: 16384 x 384 x 1536): the two launches
(ops.gemm with GELU -> ops.gemm_residual_layernorm) against ops.mlp_residual_layernorm, graph-replay timer.  With a library built with
EXTRA=-DMSAM2_MLP_ROWLN_LADDER (MSAM2_LIB_PATH), also the removal ladder of mlp_rowln_kernel: what the kernel costs without its GELU, its
fc1 / fc2 MFMAs, and its weight stream.  GPU only."""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import medical_sam2_amd.ops as ops  # noqa: E402
from tools.win_attn_bench import timeit  # noqa: E402  (graph-replay timer)

M, N, H = 16384, 384, 1536
g = torch.Generator().manual_seed(0)
a = torch.randn(M, N, generator=g).to(ops.OP16).cuda()
r = torch.randn(M, N, generator=g).cuda()
w1 = (torch.randn(H, N, generator=g) / N ** 0.5).to(ops.OP16).cuda()
w2 = (torch.randn(N, H, generator=g) / H ** 0.5).to(ops.OP16).cuda()
b1, b2 = (0.1 * torch.randn(H, generator=g)).cuda(), (0.1 * torch.randn(N, generator=g)).cuda()
lw, lb = torch.ones(N).cuda(), torch.zeros(N).cuda()
hid = torch.empty(M, H, dtype=ops.OP16, device="cuda")
c32, y16 = torch.empty(M, N, device="cuda"), torch.empty(M, N, dtype=ops.OP16, device="cuda")


def pair():
    ops.gemm(a, w1, b1, act=ops.ACT_GELU, out=hid)
    ops.gemm_residual_layernorm(hid, w2, b2, r, lw, lb, 1e-6, out=c32, out16=y16)


def fused():
    ops.mlp_residual_layernorm(a, w1, b1, w2, b2, r, lw, lb, 1e-6, out=c32, out16=y16)


fl = 4.0 * M * N * H
for rnd in range(3):
    t1 = timeit(lambda: ops.gemm(a, w1, b1, act=ops.ACT_GELU, out=hid))
    t2 = timeit(lambda: ops.gemm_residual_layernorm(hid, w2, b2, r, lw, lb, 1e-6, out=c32, out16=y16))
    tp, tf = timeit(pair), timeit(fused)
    print(f"round {rnd}: fc1+GELU {t1 * 1e6:6.1f} us   fc2+res+LN {t2 * 1e6:6.1f} us   the pair back to back {tp * 1e6:6.1f} us   "
          f"mlp_rowln_kernel {tf * 1e6:6.1f} us ({fl / tf / 1e12:4.0f} TF/s)", flush=True)

L = ops.lib()
if hasattr(L, "msam2_mlp_rowln_ladder"):
    L.msam2_mlp_rowln_ladder.restype = ctypes.c_int
    L.msam2_mlp_rowln_ladder.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 8 + [ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
    names = ["the product kernel", "no GELU", "no GELU, no fc1 MFMAs", "no fc2 MFMAs", "no GELU, no MFMAs at all",
             "no GELU, no MFMAs, no weight stage behind chunk 0", "all the arithmetic, no weight stage behind chunk 0"]
    for lad, name in enumerate(names):
        def run(lad=lad):
            rc = L.msam2_mlp_rowln_ladder(lad, a.data_ptr(), w1.data_ptr(), w2.data_ptr(), r.data_ptr(), c32.data_ptr(), lw.data_ptr(), lb.data_ptr(),
                                          y16.data_ptr(), M, H, torch.cuda.current_stream().cuda_stream)
            assert rc == 0, L.msam2_last_error().decode()
        print(f"ladder {lad}: {timeit(run) * 1e6:6.1f} us   {name}", flush=True)
