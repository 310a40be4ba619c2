"""The loss-scale and link rules that the three training drivers share (medical_sam2_amd.links) and the calibration state that
`DecoderAdam` declares: host logic on CPU tensors, the decoder backward replaced by a linear stand-in."""
import math
import os
import random
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import medical_sam2_amd.links as links  # noqa: E402

B, NM, H, W, C = 1, 2, 1, 1, 3
N_MASK, N_TOK = B * NM * 4 * H * 4 * W, B * NM * C
U = 2.0 ** -24                                             # fp32 unit round-off


def test_pow2_scale_values():
    assert links.pow2_scale(1.0) == 2.0 ** -3
    assert links.pow2_scale(0.75) == 2.0 ** -3
    assert links.pow2_scale(2.0 ** -20) == 2.0 ** 17
    assert links.pow2_scale(3.0) == 2.0 ** -5
    for a in (0.0, math.inf, math.nan):
        assert links.pow2_scale(a) == 1.0
    rng = random.Random(0)
    for _ in range(1000):
        a = 10.0 ** rng.uniform(-30.0, 30.0)
        assert 2.0 ** -4 < a * links.pow2_scale(a) <= 2.0 ** -3, a
    assert links.pow2_scale_of(torch.tensor([[0.25, -3.0], [1.0, 0.0]])) == 2.0 ** -5


def test_bce_loss_scale_values():
    assert links.bce_loss_scale(2 ** 20, 1.0, False) == 2.0 ** 16
    assert links.bce_loss_scale(2 ** 20, 1.0, True) == 2.0 ** 12
    assert links.bce_loss_scale(2 ** 20, 2.0, False) == 2.0 ** 15
    assert links.bce_loss_scale(2 ** 20, 2.0, True) == 2.0 ** 11
    assert links.bce_loss_scale(3 * 2 ** 18, 1.0, False) == links.bce_loss_scale(2 ** 19, 1.0, False) == 2.0 ** 15
    assert links.bce_loss_scale(2 ** 20, 0.5, False) == 2.0 ** 16      # a pos_weight below 1 does not raise the bound on |dloss/dlogit|


class LinearBackward:
    """Stand-in for `backward.mask_decoder_backward`: every output is a fixed random fp32 matrix applied to x = [d_masks | d_mask_tokens]
    flattened (an absent token gradient counts as zero), so the link's control flow is visible in `calls` and its recombination can be
    compared with the same linear map on the un-scaled inputs."""
    OUTS = {"d_src": 5, "d_sparse": 4, "g.w": 6, "g.b": 2, "d_feat_s0": 7, "d_feat_s1": 3}

    def __init__(self):
        gen = torch.Generator().manual_seed(0)
        self.M = {k: torch.randn(n, N_MASK + N_TOK, generator=gen) for k, n in self.OUTS.items()}
        self.calls = []

    def __call__(self, dec, src, pe, sparse, f0, f1, b, h, w, d_masks, aux=None, d_mask_tokens=None):
        assert (b, h, w) == (B, H, W) and d_masks.shape == (B, NM, 4 * H, 4 * W) and d_masks.dtype == torch.float32
        self.calls.append((d_masks.clone(), None if d_mask_tokens is None else d_mask_tokens.clone()))
        x = torch.cat([d_masks.reshape(-1), torch.zeros(N_TOK) if d_mask_tokens is None else d_mask_tokens.reshape(-1)])
        y = {k: m @ x for k, m in self.M.items()}
        aux["d_feat_s0"], aux["d_feat_s1"] = y["d_feat_s0"], y["d_feat_s1"]
        return y["d_src"], y["d_sparse"], {"w": y["g.w"], "b": y["g.b"]}


def _args():
    dec = types.SimpleNamespace(num_mask_tokens=NM, transformer_dim=C)
    return (dec, torch.zeros(B * H * W, C), None, None, None, None, B, H, W)


def _inputs(a_m: float, a_t: float):
    """fixed random gradients whose maxima are a_m and a_t (as fp32 rounds them), each carried by the last element"""
    gen = torch.Generator().manual_seed(1)
    dm, dt = (torch.rand(B, NM, 4 * H, 4 * W, generator=gen) - 0.5) * a_m, (torch.rand(B, NM, C, generator=gen) - 0.5) * a_t
    dm.view(-1)[-1], dt.view(-1)[-1] = -a_m, a_t
    return dm, dt


def _check_unscaled(fn: LinearBackward, link, dm, dt):
    """link's outputs / s_d against the stand-in's map on the un-scaled inputs in float64.  Every scaling is by a power of two (exact),
    so what differs is fp32 round-off of dot products of n = N_MASK + N_TOK terms in whatever order (relative n * U of sum |m_j x_j| per
    dot product, Higham 3.5) plus the recombining addition and the rounding of its result: (n + 2) * U * (|M| |x|) per element."""
    d_src, d_sparse, g, aux, s_d = link
    got = {"d_src": d_src, "d_sparse": d_sparse, "g.w": g["w"], "g.b": g["b"], "d_feat_s0": aux["d_feat_s0"], "d_feat_s1": aux["d_feat_s1"]}
    x = torch.cat([dm.reshape(-1), dt.reshape(-1)]).double()
    n = x.numel()
    for k, m in fn.M.items():
        want, bound = m.double() @ x, (n + 2) * U * (m.double().abs() @ x.abs())
        err = (got[k].double() / s_d - want).abs()
        assert bool((err <= bound).all()), (k, float(err.max()), float(bound.min()))
        assert float(bound.max()) < 1e-4 * float(want.abs().max())            # the bound is round-off, not a tolerance that hides a missing term


def test_decoder_link_joint_below_the_threshold():
    fn = LinearBackward()
    dm, dt = _inputs(2.0 ** -10, 2.0 ** -9)
    a_m, a_t = float(dm.abs().max()), float(dt.abs().max())
    s_d = links.pow2_scale(a_m)
    assert a_t * s_d <= 1024.0
    link = links.decoder_link(_args(), dm, dt, backward=fn)
    assert len(fn.calls) == 1 and link[4] == s_d
    assert torch.equal(fn.calls[0][0], dm * s_d) and torch.equal(fn.calls[0][1], dt * s_d)
    _check_unscaled(fn, link, dm, dt)


def test_decoder_link_splits_over_the_threshold():
    fn = LinearBackward()
    dm, dt = _inputs(1e-6, 1.0)
    a_m, a_t = float(dm.abs().max()), float(dt.abs().max())
    s_d, s_t = links.pow2_scale(a_m), links.pow2_scale(a_t)
    assert a_t * s_d > 1024.0
    link = links.decoder_link(_args(), dm, dt, backward=fn)
    assert len(fn.calls) == 2 and link[4] == s_d
    assert torch.equal(fn.calls[0][0], dm * s_d) and fn.calls[0][1] is None
    assert not fn.calls[1][0].any() and torch.equal(fn.calls[1][1], dt * s_t)
    _check_unscaled(fn, link, dm, dt)


@pytest.mark.parametrize("a_t, n_calls", [(8192.0, 1), (8192.0 * (1 + 2.0 ** -10), 2)])
def test_decoder_link_threshold_is_exclusive(a_t, n_calls):
    """a_m = 1 -> s_d = 2^-3: a_t = 8192 gives a_t * s_d == 1024.0 exactly, which still takes the joint path"""
    fn = LinearBackward()
    dm, dt = _inputs(1.0, a_t)
    assert float(dt.abs().max()) * links.pow2_scale(float(dm.abs().max())) == a_t * 2.0 ** -3
    link = links.decoder_link(_args(), dm, dt, backward=fn)
    assert len(fn.calls) == n_calls and link[4] == 2.0 ** -3
    _check_unscaled(fn, link, dm, dt)


def test_decoder_link_tokens_only_takes_its_scale_from_the_tokens():
    for d_masks in (None, torch.zeros(B, NM, 4 * H, 4 * W)):
        fn = LinearBackward()
        _, dt = _inputs(1.0, 2.0 ** -12)
        link = links.decoder_link(_args(), d_masks, dt, backward=fn)
        s = links.pow2_scale(float(dt.abs().max()))
        assert len(fn.calls) == 1 and link[4] == s == 2.0 ** 9
        assert not fn.calls[0][0].any() and torch.equal(fn.calls[0][1], dt * s)
        _check_unscaled(fn, link, torch.zeros(B, NM, 4 * H, 4 * W), dt)


def test_decoder_link_masks_only():
    for d_tokens in (None, torch.zeros(B, NM, C)):
        fn = LinearBackward()
        dm, _ = _inputs(3.0, 1.0)
        link = links.decoder_link(_args(), dm, d_tokens, backward=fn)
        assert len(fn.calls) == 1 and link[4] == 2.0 ** -5
        assert torch.equal(fn.calls[0][0], dm * 2.0 ** -5) and fn.calls[0][1] is None
        _check_unscaled(fn, link, dm, torch.zeros(B, NM, C))


def test_decoder_link_nothing_to_do():
    zm, zt = torch.zeros(B, NM, 4 * H, 4 * W), torch.zeros(B, NM, C)
    for d_masks, d_tokens in ((None, None), (zm, zt), (zm, None), (None, zt)):
        fn = LinearBackward()
        assert links.decoder_link(_args(), d_masks, d_tokens, backward=fn) is None and fn.calls == []


def test_accumulate_order_and_new_keys():
    a, b = torch.tensor([1.0, 2.0 ** -24]), torch.tensor([2.0 ** -24, 1.0])
    dst = {"k": a}
    links.accumulate(dst, {"k": b, "new": b.to(torch.float16)}, 0.5)
    assert torch.equal(dst["k"], a + b * 0.5) and torch.equal(dst["new"], b.to(torch.float16).float() * 0.5) and dst["new"].dtype == torch.float32
    links.accumulate(dst, {"k": b})
    assert torch.equal(dst["k"], (a + b * 0.5) + b)


def test_decoder_adam_declares_its_calibration_state():
    import medical_sam2_amd.training as tr
    opt = tr.DecoderAdam(torch.nn.Linear(1, 1, bias=False))                   # (no device needed to construct one)
    assert opt.calibrated_loss_scales == {} and opt.calibrated_block_scales == {} and opt.scale_monitor == {}
    opt.calibrated_loss_scales[None] = 4.0
    opt.calibrated_block_scales[None] = {"block0": 2.0, "_amax": {}}
    opt.scale_monitor["_amax"] = {"mem_scale": torch.zeros(1)}
    held = opt.calibrated_block_scales
    opt.reset_calibration()
    assert opt.calibrated_loss_scales == {} and opt.calibrated_block_scales == {} and opt.scale_monitor == {}
    assert held == {None: {"block0": 2.0, "_amax": {}}}                       # fresh dicts: what a captured graph's owner still holds is untouched
    step = types.SimpleNamespace(optimizers=[opt])
    assert list(tr.GraphedStep._scale_dicts(step)) == []
    opt.scale_monitor["_amax"] = {}
    opt.calibrated_block_scales[0] = {"done": True}
    assert list(tr.GraphedStep._scale_dicts(step)) == [opt.scale_monitor, opt.calibrated_block_scales[0]]
