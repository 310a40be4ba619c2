"""Shared test helpers."""
import json
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def load_npz(name):
    return dict(np.load(os.path.join(GOLDEN, name)))


def load_meta():
    with open(os.path.join(GOLDEN, "meta.json")) as f:
        return json.load(f)


def sub(t: torch.Tensor, n: int = 4096) -> np.ndarray:
    """Same deterministic strided subsample as tests/golden/make_golden.py:sub."""
    f = t.detach().float().contiguous().flatten()
    step = max(1, f.numel() // n)
    return f[::step][:n].numpy().copy()


def rel_err(a, b) -> float:
    a = torch.as_tensor(np.asarray(a), dtype=torch.float64)
    b = torch.as_tensor(np.asarray(b), dtype=torch.float64)
    return float((a - b).norm() / (b.norm() + 1e-30))


def max_abs(a, b) -> float:
    a = torch.as_tensor(np.asarray(a), dtype=torch.float64)
    b = torch.as_tensor(np.asarray(b), dtype=torch.float64)
    return float((a - b).abs().max())


def op16_is_fp16() -> bool:
    """operand type of the loaded library (fp16 by default; bf16 with MSAM2_LIB_PATH=libmsam2_hip_bf16.so)"""
    import medical_sam2_amd.ops as ops
    return ops.OP16 == torch.float16


def btol(tol_fp16: float, factor: float = 4.0) -> float:
    """The STATED bf16 tolerance of a bound written for the default fp16 operands: bf16 keeps 8 significand bits against fp16's 11, an 8x
    coarser unit round-off per operand; through a few dozen independent roundings the measured error ratios are 2-3.5x (round 3:
    gpurun_out/bf16_suite.log), so the bf16 bound is 4x the fp16 bound unless a test says otherwise."""
    return tol_fp16 if op16_is_fp16() else tol_fp16 * factor


def mask_iou(a, b) -> float:
    a = torch.as_tensor(np.asarray(a)) > 0
    b = torch.as_tensor(np.asarray(b)) > 0
    u = (a | b).sum().item()
    return 1.0 if u == 0 else (a & b).sum().item() / u


def gradient_step_drops(loss_fn, groups: dict, grads: dict, loss0: float, frac: float = 0.02) -> dict:
    """The loss-goes-down statement that the arithmetic guarantees ("the loss is lower after n Adam steps at lr x" is
    not one: Adam's first update moves every parameter by +-lr whatever the gradient's size).  Per group {name: module} with TRUE
    gradients grads[name] = {parameter: tensor}: the plain step p <- p - eta g with eta = frac * loss0 / |g|^2 has a first-order drop of
    frac * loss0.  Returns {name: measured relative drop}; the parameters are restored (loss_fn must rebuild stale weight copies itself,
    which the modules' version-checked caches do)."""
    out = {}
    with torch.no_grad():
        for name, mod in groups.items():
            g = grads[name]
            params = dict(mod.named_parameters())
            g2 = sum(float(v.double().pow(2).sum()) for v in g.values())
            eta = frac * loss0 / g2
            for k in g:
                params[k].add_(g[k].to(params[k].dtype), alpha=-eta)
            out[name] = (loss0 - loss_fn()) / loss0
            for k in g:
                params[k].add_(g[k].to(params[k].dtype), alpha=eta)
    return out


# ---- multi-process GPU tests: the same workers run as gloo ranks sharing the one GPU of the test box (RCCL refuses two ranks on one
# device) and -- tests/test_multigpu_gpu.py, MSAM2_TEST_REAL_DEVICES=1 -- as RCCL ranks on one GPU each
def real_devices() -> bool:
    import os
    return os.environ.get("MSAM2_TEST_REAL_DEVICES") == "1"


def rank_device(rank: int) -> int:
    return rank if real_devices() else 0


def host_cpu_share() -> int:
    """CPUs this process may actually use: the cgroup quota when there is one (the GPU box gives 16 of its 256 hardware threads), else the
    affinity mask -- bench.host_cpu_share's rule.  torch sizes its pool by the host's hardware threads; on all 256 the oracle runs 3x
    slower than on 16 (tests/probes/cpu_threads_probe.py)."""
    import os
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, -(-int(quota) // int(period))))
    except (OSError, ValueError):
        pass
    return n


def init_test_process_group(rank: int, world: int):
    """process group of a spawned test worker: backend nccl (= RCCL over xGMI) with one device per rank under MSAM2_TEST_REAL_DEVICES=1,
    otherwise gloo with every rank on device 0.  MASTER_ADDR / MASTER_PORT are in the environment."""
    import torch.distributed as dist
    torch.set_num_threads(max(1, host_cpu_share() // world))
    torch.cuda.set_device(rank_device(rank))
    if real_devices():
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank_device(rank)))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)


def all_gather_flat(flat: torch.Tensor, world: int):
    """all-gather of one flat tensor per rank for cross-rank comparisons (RCCL moves device tensors, gloo host tensors); returns CPU copies"""
    import torch.distributed as dist
    t = flat.cuda() if real_devices() else flat.cpu()
    out = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(out, t)
    return [o.cpu() for o in out]


# ---- kernel-variant matrices (tests/test_gemm_variants_gpu.py, tests/test_attention_variants_gpu.py)
SENT16, SENT32 = 0x7E5A, 0x7FC0DEAD            # bit patterns no kernel writes in these tests: the canaries around every output view


# Itanium manglings of the builtin types a kernel of this library is templated on -> their demangled spelling, white space removed
_MANGLED_TYPES = (("DF16_", "_Float16"), ("DF16b", "__bf16"), ("u6__bf16", "__bf16"), ("Dh", "__fp16"), ("f", "float"), ("d", "double"), ("i", "int"),
                  ("j", "unsignedint"), ("l", "long"), ("m", "unsignedlong"), ("s", "short"), ("t", "unsignedshort"), ("a", "signedchar"),
                  ("h", "unsignedchar"), ("c", "char"), ("b", "bool"))


def _mangled_template_args(rest: str):
    """the top-level template arguments of 'I<args>E...': integer / bool literals (Li128E, Lb1E, Lin3E) and the element types of
    _MANGLED_TYPES, in order; parsing stops at the closing E or at the first argument of another kind"""
    out, i = [], 1
    while i < len(rest) and rest[i] != "E":
        m = re.match(r"L([a-z])(n?)(\d+)E", rest[i:])
        if m:
            t, neg, v = m.groups()
            out.append(("true" if v == "1" else "false") if t == "b" else ("-" if neg else "") + v)
            i += m.end()
            continue
        for code, spelled in _MANGLED_TYPES:
            if rest.startswith(code, i):
                out.append(spelled)
                i += len(code)
                break
        else:
            break
    return out


def kernel_key(name: str) -> str:
    """'void gemm_kernel<128, 32, 4, 1>(GemmParams)' or its mangled form '_Z11gemm_kernelILi128ELi32ELi4ELi1EEv10GemmParams' ->
    'gemm_kernel<128,32,4,1>'; type arguments keep their demangled spelling: 'void layernorm_kernel<float, _Float16, 2>(...)' and
    '_Z16layernorm_kernelIfDF16_Li2EEv...' -> 'layernorm_kernel<float,_Float16,2>' (__bf16 in the bf16 build); a kernel of an unnamed
    namespace ('(anonymous namespace)::attn_bwd_kernel<...>', '_ZN12_GLOBAL__N_115attn_bwd_kernel...') is keyed by its own name"""
    name = re.sub(r"^_ZN12_GLOBAL__N_1", "_Z", name.strip().replace("(anonymous namespace)::", ""))
    m = re.match(r"_Z(\d+)", name)
    if m:
        n = int(m.group(1))
        base = name[m.end():m.end() + n]
        rest = name[m.end() + n:]
        if not rest.startswith("I"):
            return base
        return base + "<" + ",".join(_mangled_template_args(rest)) + ">"
    name = re.sub(r"^void ", "", name.strip()).split("(")[0]
    if "_Accum" in name:
        # A C++ runtime whose demangler predates the bf16 mangling reads 'DF16b' plus the NEXT character as a fixed-point type and prints
        # 'bool _Accum'.  Most such names then fail to demangle and arrive mangled (handled above); the ones that get through lost
        # exactly that character: the 'f' of a following float argument, or the 'L' of a following literal 1 ('Li1E' -> 'int, E',
        # 'Lb1E' -> 'bool, E').  Undo that.
        name = name.replace("bool _Accum, int, E", "__bf16, 1").replace("bool _Accum, bool, E", "__bf16, true").replace("bool _Accum", "__bf16, float")
    return re.sub(r"\s+", "", name)


def kernels_launched(fn, prefix: str):
    """run fn under torch.profiler (kernel activity) and return the set of kernels it launched whose kernel_key starts with `prefix`"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    keys = {kernel_key(e.name) for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}
    return {k for k in keys if k.startswith(prefix)}


def nan_padded(rows, cols, ld, dtype, src, device="cuda"):
    """src [rows, cols] as the leading block of a [rows + 5, ld] buffer whose other elements are NaN"""
    buf = torch.full((rows + 5, ld), float("nan"), dtype=dtype, device=device)
    buf[:rows, :cols] = src.to(dtype)
    return buf[:rows, :cols]


class Canvas:
    """an [M, N] output view inside a sentinel-filled buffer: `aligned` puts the view on a 16-byte boundary with ldc % 8 == 0 (direct-store
    epilogues), otherwise the view starts one element in and ldc is odd (generic epilogue)"""

    def __init__(self, M, N, dtype, aligned=True, device="cuda"):
        es = dtype.itemsize
        self.itype = torch.int16 if es == 2 else torch.int32
        self.pr, self.pc = 3, (16 // es if aligned else 1)
        ldc = self.pc + N + (16 // es) + 8
        ldc = (ldc + 7) // 8 * 8 if aligned else (ldc | 1)
        self.buf = torch.empty(M + 2 * self.pr, ldc, dtype=dtype, device=device)
        self.sent = SENT16 if es == 2 else SENT32
        self.buf.view(self.itype).fill_(self.sent)
        self.view = self.buf[self.pr:self.pr + M, self.pc:self.pc + N]
        self.inside = torch.zeros(self.buf.shape, dtype=torch.bool, device=device)
        self.inside[self.pr:self.pr + M, self.pc:self.pc + N] = True

    def sentinels_intact(self):
        return bool((self.buf.view(self.itype)[~self.inside] == self.sent).all())

    def bits(self):
        return self.buf.view(self.itype).clone()


class Flat:
    """a contiguous output of `shape` inside a sentinel-filled 1-D buffer (64 guard elements on either side); `offset` moves the view that
    many elements off its 128-byte boundary (misaligned-output paths)"""
    G = 64

    def __init__(self, shape, dtype, offset=0, device="cuda"):
        n = 1
        for s in shape:
            n *= s
        es = dtype.itemsize
        self.itype = torch.int16 if es == 2 else torch.int32
        self.sent = SENT16 if es == 2 else SENT32
        self.buf = torch.empty(2 * self.G + offset + n, dtype=dtype, device=device)
        self.buf.view(self.itype).fill_(self.sent)
        self.lo, self.hi = self.G + offset, self.G + offset + n
        self.view = self.buf[self.lo:self.hi].view(*shape)

    def sentinels_intact(self):
        b = self.buf.view(self.itype)
        return bool((b[:self.lo] == self.sent).all()) and bool((b[self.hi:] == self.sent).all())


def nan_guarded(src, offset=0, guard=64):
    """a contiguous copy of src inside a 1-D buffer with `guard` NaN elements (0xFF bytes for integer types) on either side, `offset` elements
    off the buffer's alignment: a kernel that reads past either end of the tensor returns NaN"""
    n = src.numel()
    buf = torch.empty(2 * guard + offset + n, dtype=src.dtype, device=src.device)
    if src.dtype.is_floating_point:
        buf.fill_(float("nan"))
    else:
        buf.view(torch.uint8).fill_(0xFF)
    v = buf[guard + offset:guard + offset + n].view(src.shape)
    v.copy_(src)
    return v


def K(key: str) -> str:
    """kernel key of a table entry: T16 stands for the library's 16-bit operand type as the demangler spells it"""
    return key.replace("T16", "_Float16" if op16_is_fp16() else "__bf16")


def reached(L, key, prefix, launches):
    """run the launches (callables returning the C entry's code) under the profiler: all succeed, and exactly `key` ran among the kernels
    whose name starts with `prefix` (key None: none)"""
    def go():
        for fn in launches:
            rc = fn()
            assert rc == 0, L.msam2_last_error().decode()
    got = kernels_launched(go, prefix)
    want = set() if key is None else {K(key)}
    assert got == want, f"expected {sorted(want)}, launched {sorted(got)}"


def within(got, ref, bound, what):
    d = (got.double() - ref).abs()
    bad = ~(d <= bound)                                   # a NaN anywhere fails
    if bool(bad.any()):
        i = int((d - bound).masked_fill(~bad, -1).argmax()) if not bool(torch.isnan(d).any()) else int(torch.isnan(d).flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; worst |err| {float(d.flatten()[i]):.3e} "
                             f"against {float(bound.expand_as(d).flatten()[i]):.3e} at flat index {i}")


def same_bits(a, b, what):
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[a.dtype.itemsize]
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    ne = a.contiguous().view(it) != b.contiguous().view(it)
    assert not bool(ne.any()), f"{what}: {int(ne.sum())} of {ne.numel()} elements differ in their bits"


def strided_nan(src, ld, off=0):
    """src [rows, C] as a view with row stride ld inside a NaN-filled buffer, starting `off` elements into it"""
    rows, C = src.shape
    buf = torch.full((off + (rows + 5) * ld + 16,), float("nan"), dtype=src.dtype, device="cuda")
    v = torch.as_strided(buf, (rows, C), (ld, 1), off)
    v.copy_(src)
    return v


class Canvas2:
    """[M, N] output view with row stride ld inside a sentinel-filled buffer, three rows before and after and `left` columns before it
    (left * itemsize is the view's byte offset from a 16-byte boundary when ld * itemsize is a multiple of 16)"""

    def __init__(self, M, N, dtype, ld, left):
        assert ld >= left + N
        es = dtype.itemsize
        self.itype = torch.int16 if es == 2 else torch.int32
        self.sent = SENT16 if es == 2 else SENT32
        self.buf = torch.empty(M + 6, ld, dtype=dtype, device="cuda")
        self.buf.view(self.itype).fill_(self.sent)
        self.view = self.buf[3:3 + M, left:left + N]
        self.inside = torch.zeros(self.buf.shape, dtype=torch.bool, device="cuda")
        self.inside[3:3 + M, left:left + N] = True

    def sentinels_intact(self):
        return bool((self.buf.view(self.itype)[~self.inside] == self.sent).all())
