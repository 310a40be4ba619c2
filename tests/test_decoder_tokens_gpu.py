"""Token-side block kernels of the two-way decoder (csrc/decoder_tokens.hip) on the GPU: every output of the three entries
against the launches they replace on the same inputs, the whole transformer against the oracle beside its multi-launch form, and the
properties a shared workspace, a stale counter or an unordered sum would break (same bits on every run, under graph replay, on two streams).

Bound of the kernel-level comparisons: the attention family's own, 0.02 + 0.01 |ref| (tests/test_window_qkv_attention_gpu.py).  Both paths
round at the same points; what differs is the order of fp32 sums, and through the 16-bit rounding points a value may move by one unit."""
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

from helpers import rel_err, same_bits  # noqa: E402
from oracle import sam2_oracle as O  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, H, CI, HID = 256, 8, 128, 2048
# ragged R, full R = 32, T not a multiple of 8, the T limit, no prompt tokens
SHAPES = [(1, 7), (4, 8), (3, 9), (2, 16), (5, 6)]
L_IMG = 256


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import medical_sam2_amd.ops as ops_mod
    return ops_mod


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


USED = {}


def close(got, ref, what):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    lim = 0.02 + 0.01 * ref.abs()
    frac = float((err / lim).max())
    USED[what] = max(USED.get(what, 0.0), frac)
    print(f"{what}: max |err| {float(err.max()):.4g}, {frac:.3f} of the bound")
    assert not bool(torch.isnan(got).any()) and bool((err <= lim).all()), f"{what}: {int((err > lim).sum())} of {err.numel()} outside 0.02 + 0.01 |ref|"


_W = {}


def weights(ops):
    """one set of block weights (16-bit matrices, fp32 vectors) on the device, shared by the kernel-level tests and left unchanged"""
    if _W:
        return _W
    mat = lambda n, k, seed: rnd(n, k, seed=seed, scale=k ** -0.5).to(ops.OP16).to(DEV)
    vec = lambda n, seed, scale=0.5, base=0.0: (base + rnd(n, seed=seed, scale=scale)).to(DEV)
    _W.update(wqkv=mat(3 * C, C, 1), bqkv=vec(3 * C, 2), wso=mat(C, C, 3), bso=vec(C, 4), n1w=vec(C, 5, 0.1, 1.0), n1b=vec(C, 6, 0.1),
              wcq=mat(CI, C, 7), bcq=vec(CI, 8), wco=mat(C, CI, 9), bco=vec(C, 10), n2w=vec(C, 11, 0.1, 1.0), n2b=vec(C, 12, 0.1),
              w1=mat(HID, C, 13), b1=vec(HID, 14), w2=mat(C, HID, 15), b2=vec(C, 16), n3w=vec(C, 17, 0.1, 1.0), n3b=vec(C, 18, 0.1),
              wkv=mat(C, C, 19), bkv=vec(C, 20), wfq=mat(CI, C, 21), bfq=vec(CI, 22))
    return _W


# ---- the launches the entries replace, as TwoWayAttentionBlock.run / TwoWayTransformer.run issue them
def old_self(ops, x, pe, skip, W, B, T):
    qkv = ops.gemm_tokens(x, W["wqkv"], W["bqkv"], addend=None if skip else pe, add_cols=2 * C).view(B, T, 3 * C)
    o = ops.attention_small(qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:], H).reshape(B * T, C)
    y = ops.gemm(o, W["wso"], W["bso"], residual=None if skip else x, out_dtype=torch.float32)
    y = ops.layernorm(y, W["n1w"], W["n1b"], 1e-5, out_dtype=torch.float32)
    return y, ops.gemm_tokens(y, W["wcq"], W["bcq"], addend=pe, add_cols=CI)


def old_mlp(ops, o, x, pe, W, last):
    y = ops.layernorm(ops.gemm(o, W["wco"], W["bco"], residual=x, out_dtype=torch.float32), W["n2w"], W["n2b"], 1e-5, out_dtype=torch.float32)
    hmid = ops.gemm_tokens(y, W["w1"], W["b1"], act=ops.ACT_RELU)
    y = ops.layernorm(ops.gemm(hmid, W["w2"], W["b2"], residual=y, out_dtype=torch.float32), W["n3w"], W["n3b"], 1e-5, out_dtype=torch.float32)
    kv = ops.gemm_tokens(y, W["wkv"], W["bkv"], addend=pe, add_cols=CI)
    return y, kv, (ops.gemm_tokens(y, W["wfq"], W["bfq"], addend=pe, add_cols=CI) if last else None)


def old_tail(ops, o, x, W):
    return ops.layernorm(ops.gemm(o, W["wco"], W["bco"], residual=x, out_dtype=torch.float32), W["n2w"], W["n2b"], 1e-5, out_dtype=torch.float32)


@pytest.mark.parametrize("skip", [True, False], ids=["skip_first_layer_pe", "with_pe"])
@pytest.mark.parametrize("B,T", SHAPES)
def test_entries_against_the_launches_they_replace(ops, B, T, skip):
    W = weights(ops)
    R = B * T
    assert ops.decoder_tokens_supported(C, H, C, CI, HID, 2, ops.ACT_RELU, B, T)
    x, pe = rnd(R, C, seed=30 + R).to(DEV), rnd(R, C, seed=31 + R).to(DEV)
    o = rnd(R, CI, seed=32 + R).to(ops.OP16).to(DEV)
    # (a) self block
    y, qp = ops.decoder_tokens_self(x, pe, skip, W["wqkv"], W["bqkv"], W["wso"], W["bso"], W["n1w"], W["n1b"], 1e-5, W["wcq"], W["bcq"], B, T, H)
    ry, rqp = old_self(ops, x, pe, skip, W, B, T)
    close(y, ry, "self: queries after norm1")
    close(qp, rqp, "self: tokens -> image query projection")
    # (b) MLP block, as an inner block and as the last one
    for last in (False, True):
        y, kv, fq = ops.decoder_tokens_mlp(o, x, W["wco"], W["bco"], W["n2w"], W["n2b"], 1e-5, W["w1"], W["b1"], W["w2"], W["b2"], W["n3w"], W["n3b"],
                                           1e-5, pe, W["wkv"], W["bkv"], B, T, H, w_fq=W["wfq"] if last else None, b_fq=W["bfq"] if last else None)
        ry, rkv, rfq = old_mlp(ops, o, x, pe, W, last)
        close(y, ry, "mlp: queries after norm3")
        close(kv, rkv, "mlp: image -> token k | v")
        assert (fq is None) == (not last)
        if last:
            close(fq, rfq, "mlp: final attention's query projection")
    # (c) tail
    close(ops.decoder_tokens_tail(o, x, W["wco"], W["bco"], W["n2w"], W["n2b"], 1e-5, B, T, H), old_tail(ops, o, x, W), "tail: queries")
    print("largest fraction of the bound used so far:", max(USED.values()))


# ---- key-split tokens -> image attention: the partials through the kernels that merge them
@pytest.mark.parametrize("L", [100, 256, 4096], ids=lambda L: f"L{L}")     # ranges that divide by neither the split nor 32; one tile; the launcher's limit
@pytest.mark.parametrize("B,T", SHAPES)
def test_keysplit_partials_through_their_consumers(ops, B, T, L):
    W = weights(ops)
    R = B * T
    q = rnd(B, T, CI, seed=33 + R).to(ops.OP16).to(DEV)
    kvq = rnd(B * L, 3 * CI, seed=34 + R + L).to(ops.OP16).to(DEV)         # k | v as column blocks of a wider map, as the decoder has them
    k, v = kvq[:, :CI].view(B, L, CI), kvq[:, CI:2 * CI].view(B, L, CI)
    x, pe = rnd(R, C, seed=30 + R).to(DEV), rnd(R, C, seed=31 + R).to(DEV)
    o = ops.attention_small(q, k, v, H).reshape(R, CI)
    # the merge restated: weights 2^(m_s - M), sums in split order, one rounding to 16 bits
    for splits in (None, 3):
        part, S = ops.attention_fewq_keysplit(q, k, v, H, splits=splits)
        assert S == (splits or max(1, min(8, 128 // (B * H)))) and part.shape == (B * H * S, T, 18)
        pp = part.view(B, H, S, T, 18).double()
        m, l, acc = pp[..., 0], pp[..., 1], pp[..., 2:]
        wgt = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp2(m - m.max(dim=2, keepdim=True).values))
        merged = ((acc * wgt[..., None]).sum(2) / (l * wgt).sum(2)[..., None]).permute(0, 2, 1, 3).reshape(R, CI)
        close(merged, o, f"L {L}: merged partials against the attention's own launch")
        args = (x, W["wco"], W["bco"], W["n2w"], W["n2b"], 1e-5, W["w1"], W["b1"], W["w2"], W["b2"], W["n3w"], W["n3b"], 1e-5, pe, W["wkv"], W["bkv"], B, T, H)
        for got, ref, what in zip(ops.decoder_tokens_mlp((part, S), *args, w_fq=W["wfq"], b_fq=W["bfq"]),
                                  ops.decoder_tokens_mlp(o, *args, w_fq=W["wfq"], b_fq=W["bfq"]), ("queries", "k | v", "final q")):
            close(got, ref, f"L {L}: mlp from partials: {what}")
        targs = (x, W["wco"], W["bco"], W["n2w"], W["n2b"], 1e-5, B, T, H)
        close(ops.decoder_tokens_tail((part, S), *targs), ops.decoder_tokens_tail(o, *targs), f"L {L}: tail from partials")


def test_decoder_takes_the_key_split_at_its_shapes(ops, tw, monkeypatch):
    """L = 1024 image tokens: TwoWayTransformer.run hands partials to the block kernels; MSAM2_NO_FEWQ_KEYSPLIT=1 brings the attention's own launch back"""
    from helpers import kernels_launched
    B, T, L = 4, 8, 1024
    keys, kpe, tok = rnd(B * L, C, seed=55).to(DEV), key_pe(L), rnd(B * T, C, seed=57).to(DEV)
    run = lambda **k: tw.run(keys, kpe, tok, B, T, L, **k)
    with torch.no_grad():
        rq, rk = run()
        fq, fk = run(fused_tokens=True)
        close(fq, rq, "key split: queries")
        close(fk, rk, "key split: keys")
        assert kernels_launched(lambda: run(fused_tokens=True), "attn_fewq16") == {"attn_fewq16_part_kernel<1>"}    # 256 keys per workgroup
        monkeypatch.setenv("MSAM2_NO_FEWQ_KEYSPLIT", "1")
        assert kernels_launched(lambda: run(fused_tokens=True), "attn_fewq16") == {"attn_fewq16_kernel"}
        nq, nk = run(fused_tokens=True)
        close(nq, rq, "no key split: queries")
        close(nk, rk, "no key split: keys")


def make_transformer(seed=0):
    from medical_sam2_amd.modeling.sam_heads import TwoWayTransformer
    torch.manual_seed(seed)
    tw = TwoWayTransformer(depth=2, embedding_dim=C, num_heads=H, mlp_dim=HID)
    with torch.no_grad():                                   # LayerNorms away from (1, 0), biases away from 0
        for n, p in tw.named_parameters():
            if "norm" in n or n.endswith("bias"):
                p.add_(0.1 * torch.randn_like(p))
    return tw.to(DEV).eval()


@pytest.fixture(scope="module")
def tw(ops):
    return make_transformer()


_KPE = {}


def key_pe(L):
    """the dense position encoding of an L-token image: ONE tensor per L for the whole session, as in the decoder, whose modules cache its
    projections by the tensor's identity (_image_side_projections: it is batch-shared and input-independent)"""
    if L not in _KPE:
        _KPE[L] = rnd(L, C, seed=1000 + L).to(DEV)
    return _KPE[L]


def tw_inputs(B, T, seed):
    return (rnd(B * L_IMG, C, seed=seed).to(DEV), key_pe(L_IMG), rnd(B * T, C, seed=seed + 2).to(DEV))


@pytest.mark.parametrize("B,T", SHAPES)
def test_block_and_transformer_against_their_multi_launch_form(ops, tw, B, T):
    """both block kinds (layer 0 skips the position encoding of its first attention) and the tail inside TwoWayTransformer.run, L = 256"""
    keys, kpe, tok = tw_inputs(B, T, 40 + B * T)
    with torch.no_grad():
        for i, blk in enumerate(tw.layers):
            assert blk.tokens_fused(B, T, True) and blk.skip_first_layer_pe == (i == 0)
            fq, fk, fk16, _ = blk.run(tok, keys, tok, kpe, B, T, L_IMG, fused_tokens=True)
            rq, rk, rk16, _ = blk.run(tok, keys, tok, kpe, B, T, L_IMG, fused_tokens=False)
            close(fq, rq, f"block {i}: queries")
            close(fk, rk, f"block {i}: keys")
            close(fk16, rk16, f"block {i}: 16-bit keys")
        fq, fk = tw.run(keys, kpe, tok, B, T, L_IMG, fused_tokens=True)
        rq, rk = tw.run(keys, kpe, tok, B, T, L_IMG)
        close(fq, rq, "transformer: queries")
        close(fk, rk, "transformer: keys")


def test_fused_path_launches_its_kernels_and_none_it_replaces(ops, tw):
    from helpers import kernels_launched
    B, T = 4, 8
    keys, kpe, tok = tw_inputs(B, T, 50)
    with torch.no_grad():
        tw.run(keys, kpe, tok, B, T, L_IMG, fused_tokens=True)         # weight caches filled
        got = kernels_launched(lambda: tw.run(keys, kpe, tok, B, T, L_IMG, fused_tokens=True), "")
    assert {k for k in got if k.startswith("dec_")} == {"dec_self_kernel", "dec_mlp_kernel", "dec_kv_kernel", "dec_tail_kernel"}, sorted(got)
    # (the tokens -> image attention at L = 256 is attn_small_kernel<16>: the self-attention's 32-wide form is the one that left)
    assert not any(k.startswith(("gemm_skinny_kernel", "attn_small_kernel<32>")) for k in got), sorted(got)


# ---- module level: against the oracle, with the model, rel_err and tolerances of tests/test_modules_gpu.py::test_attention_modules_forward
@pytest.fixture(scope="module")
def net(ops):
    import medical_sam2_amd.build_sam as bs
    import medical_sam2_amd.weights as wts
    m = bs.build_sam2("sam2_hiera_s", device="cpu", hydra_overrides_extra=["++model.image_size=256"])
    sd = wts.init_weights("hiera_s", 0)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval(), sd


_NET_PE = {}


@pytest.mark.parametrize("B,T", [(2, 7)] + SHAPES)          # the shape of test_attention_modules_forward, then this file's
@pytest.mark.parametrize("oracle", ["fp32_oracle", "operand_rounding_oracle"])
def test_transformer_against_the_oracle(ops, net, oracle, B, T):
    import contextlib
    from medical_sam2_amd.modeling.common import tokens_of
    m, P = net
    fp16 = ops.OP16 == torch.float16
    tight = oracle == "operand_rounding_oracle"
    tol = 2.0 * (2.0 ** -11 if fp16 else 2.0 ** -8) if tight else (3e-3 if fp16 else 2e-2)
    tw_ = m.sam_mask_decoder.transformer
    q = rnd(B, T, 256, seed=8 + 100 * B + T)
    src, pe = rnd(B, 256, 16, 16, seed=11 + 100 * B + T), rnd(1, 256, 16, 16, seed=12)
    if "kpe" not in _NET_PE:                                # one device tensor for the session (see key_pe)
        _NET_PE["kpe"] = tokens_of(pe.to(DEV))[:256].contiguous()
    with torch.no_grad(), (O.operand_rounding(ops.OP16) if tight else contextlib.nullcontext()):
        rq, rk = O.two_way_transformer(P, "sam_mask_decoder.transformer", src, pe.expand(B, -1, -1, -1), q)
        keys, kpe = tokens_of(src.to(DEV)), _NET_PE["kpe"]
        tok = q.to(DEV).reshape(B * T, 256).contiguous()
        res = {}
        for fused in (True, False):
            qq, kk = tw_.run(keys, kpe, tok, B, T, 256, fused_tokens=fused)
            res[fused] = (rel_err(qq.view(B, T, 256).cpu().float(), rq), rel_err(kk.view(B, 256, 256).cpu().float(), rk))
    print(f"{oracle} B {B} T {T}: rel_err (queries, keys) fused {res[True][0]:.3e} {res[True][1]:.3e}, multi-launch {res[False][0]:.3e} {res[False][1]:.3e}, tol {tol:.3e}")
    assert max(res[True]) < tol and max(res[False]) < tol, (res, tol)


# ---- same bits every time
def run_fused(tw, keys, kpe, tok, B, T):
    with torch.no_grad():
        return tw.run(keys, kpe, tok, B, T, L_IMG, fused_tokens=True)


def test_two_runs_give_the_same_bits(ops, tw):
    B, T = 4, 8
    keys, kpe, tok = tw_inputs(B, T, 60)
    a = run_fused(tw, keys, kpe, tok, B, T)
    b = run_fused(tw, keys, kpe, tok, B, T)
    same_bits(a[0], b[0], "queries of two runs")
    same_bits(a[1], b[1], "keys of two runs")


def test_graph_replays_equal_eager_runs(ops, tw):
    B, T = 3, 9
    keys, kpe, tok = tw_inputs(B, T, 70)                    # keys and tok are this test's own tensors: overwritten in place below
    run_fused(tw, keys, kpe, tok, B, T)                     # weight caches filled outside the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run_fused(tw, keys, kpe, tok, B, T)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gq, gk = run_fused(tw, keys, kpe, tok, B, T)
    for rep in range(3):
        nk, _, nt = tw_inputs(B, T, 71 + 3 * rep)
        keys.copy_(nk)
        tok.copy_(nt)
        g.replay()
        torch.cuda.synchronize()
        rq, rk = gq.clone(), gk.clone()
        eq, ek = run_fused(tw, keys, kpe, tok, B, T)
        same_bits(rq, eq, f"queries of replay {rep}")
        same_bits(rk, ek, f"keys of replay {rep}")


def test_two_streams_through_one_module_equal_their_serial_runs(ops, tw):
    B, T = 4, 8
    ins = [tw_inputs(B, T, 80), tw_inputs(B, T, 90)]
    serial = [run_fused(tw, *i, B, T) for i in ins]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for rep in range(4):                                    # interleaved issue: the two instances' kernels overlap on the device
        outs = []
        for s, i in zip(streams, ins):
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                outs.append(run_fused(tw, *i, B, T))
        torch.cuda.synchronize()
        for j, (o, r) in enumerate(zip(outs, serial)):
            print(f"stream {j}, round {rep}: max |queries - serial| {float((o[0] - r[0]).abs().max()):.3g}, keys {float((o[1] - r[1]).abs().max()):.3g}")
            same_bits(o[0], r[0], f"queries of stream {j}, round {rep}")
            same_bits(o[1], r[1], f"keys of stream {j}, round {rep}")


def test_same_file_on_the_bf16_library(ops):
    """the operand type is a property of the loaded library: the tests of this file once more in a child process on libmsam2_hip_bf16.so (the library the benchmark's headline runs on), as tests/test_bf16_build_gpu.py runs its files"""
    if os.environ.get("MSAM2_LIB_PATH"):
        assert str(ops.OP16).endswith(os.environ.get("MSAM2_EXPECT_OP16", "")), ops.OP16
        return                                              # this IS a run on a chosen library
    lib = os.path.join(ROOT, "medical-sam2_amd", "libmsam2_hip_bf16.so")
    assert os.path.exists(lib), "libmsam2_hip_bf16.so is built by __graft_entry__.build()"
    env = dict(os.environ, MSAM2_LIB_PATH=lib, MSAM2_EXPECT_OP16="bfloat16", PYTHONUNBUFFERED="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-30:])
    print(tail)
    assert r.returncode == 0 and " passed" in tail and "failed" not in tail, tail
