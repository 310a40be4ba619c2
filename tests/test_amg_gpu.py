"""N prompt sets on one image, set_image_batch / predict_batch, the automatic-mask-generation kernels and the SAM2AutomaticMaskGenerator
pipeline on the MI355X.

- many prompt sets through SAM2ImagePredictor._predict against the CPU oracle on the device's own image features (bars of
  test_mask_decoder_cell_nums_prompt_repetition);
- the decoder's shared image operands (stride-0 embedding and skip maps) bit-identical to explicitly repeated ones;
- mask_stats / mask_rle / box_nms equal, integer for integer, to torch reductions / a CPU RLE over ops.bilinear_upsample's output and to
  a CPU greedy NMS;
- generate() record for record equal to a CPU restatement of the reference pipeline fed with the device predictor's own outputs."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import sam2_oracle as O  # noqa: E402
import medical_sam2_amd.weights as wts  # noqa: E402
from helpers import rel_err  # noqa: E402
import amg_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = 256


@pytest.fixture(scope="module")
def model():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import medical_sam2_amd.build_sam as bs
    sd = wts.init_weights("hiera_t", 0)
    m = bs.build_sam2("sam2_hiera_t", device="cpu", hydra_overrides_extra=[f"++model.image_size={S}"])
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval(), sd, O.model_config("hiera_t", S)


@pytest.fixture(autouse=True)
def _no_grad():
    """Inference only; the grad mode of the session is restored after each test (later files train)."""
    with torch.no_grad():
        yield


@pytest.fixture(scope="module")
def tol():
    import medical_sam2_amd.ops as ops
    return 3e-3 if ops.OP16 == torch.float16 else 2e-2


def blob_u8(seed, h=S, w=S):
    import medical_sam2_amd.synthetic as syn
    img, _ = syn.blob_image(seed, max(h, w))
    return img[:, :h, :w].clamp(0, 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().numpy()


def oracle_predict(sd, cfg, pred, pts, labels, boxes, mask_input, multimask):
    """The decoder of the oracle on the predictor's image features, N prompt sets repeated explicitly (eval mode: one output = the
    stability-selected mask of mask_decoder.py:269-317)."""
    concat = (pts, labels) if pts is not None else None
    if boxes is not None:
        bc, bl = boxes.reshape(-1, 2, 2), torch.tensor([[2, 3]], dtype=torch.int).repeat(boxes.shape[0], 1)
        concat = (bc, bl) if concat is None else (torch.cat([bc, concat[0]], 1), torch.cat([bl, concat[1]], 1))
    sparse, dense = O.prompt_encoder(sd, cfg, concat, None, mask_input)
    n = sparse.shape[0]
    emb = pred._features["image_embed"].float().cpu()
    hr = [f.float().cpu().expand(n, -1, -1, -1) for f in pred._features["high_res_feats"]]
    pe = pred.model.sam_prompt_encoder.get_dense_pe().float().cpu()
    low, iou, _, _ = O.mask_decoder(sd, cfg, emb.expand(n, -1, -1, -1), pe, sparse, dense.expand(n, -1, -1, -1), multimask, hr)
    return low, iou


def count_shared_shuffles(monkeypatch):
    """Counts the calls of ops.convt2x2_shuffle_shared (the decoder's stride-0 skip path): a silent fall-back to N copies of the skip
    maps would leave the results right and the count at 0."""
    import medical_sam2_amd.ops as ops
    calls = []
    real = ops.convt2x2_shuffle_shared

    def counting(*a, **k):
        calls.append(a[5])                                              # B: the prompt sets served by one skip map
        return real(*a, **k)
    monkeypatch.setattr(ops, "convt2x2_shuffle_shared", counting)
    return calls


def test_many_prompt_sets_vs_oracle(model, tol, monkeypatch):
    from medical_sam2_amd.image_predictor import SAM2ImagePredictor
    m, sd, cfg = model
    pred = SAM2ImagePredictor(m)
    pred.set_image(blob_u8(3))
    g = torch.Generator().manual_seed(11)
    pts5 = torch.rand(5, 2, 2, generator=g) * S
    lab5 = torch.tensor([[1, 0], [1, 1], [0, 1], [1, 1], [1, 0]], dtype=torch.int)
    xy = torch.rand(3, 2, generator=g) * (S / 2)
    box3 = torch.cat([xy, xy + S / 4 + torch.rand(3, 2, generator=g) * (S / 4)], 1)
    pts64 = torch.rand(64, 1, 2, generator=g) * S
    masks_in = torch.randn(3, 1, S // 4, S // 4, generator=g) * 4
    cases = [("points5", pts5, lab5, None, None, True), ("boxes3", None, None, box3, None, False),
             ("boxes+points", pts5[:3, :1], lab5[:3, :1], box3, None, True), ("mask_input", pts5[:3], lab5[:3], None, masks_in, False),
             ("points64", pts64, torch.ones(64, 1, dtype=torch.int), None, None, True)]
    d = lambda t: None if t is None else t.to(DEV)
    shared = count_shared_shuffles(monkeypatch)
    for name, p, l, b, mi, mm in cases:
        del shared[:]
        masks, iou, low = pred._predict(d(p), d(l), d(b), d(mi), multimask_output=mm, return_logits=True)
        n, c = (p if p is not None else b).shape[0], 3 if mm else 1
        assert shared == [n, n], (name, shared)                         # both up-scaling steps read the one image's skip maps
        assert masks.shape == (n, c, S, S) and iou.shape == (n, c) and low.shape == (n, c, S // 4, S // 4), name
        ref_low, ref_iou = oracle_predict(sd, cfg, pred, p, l, b, mi, mm)
        assert rel_err(low.cpu(), ref_low.clamp(-32, 32)) < 2 * tol, name
        assert rel_err(iou.cpu(), ref_iou) < 2 * tol, name
        # one prompt set per call gives the same within the same bars
        for i in (0, n - 1):
            one = pred._predict(d(p[i:i + 1]) if p is not None else None, d(l[i:i + 1]) if l is not None else None,
                                d(b[i:i + 1]) if b is not None else None, d(mi[i:i + 1]) if mi is not None else None, multimask_output=mm,
                                return_logits=True)
            assert rel_err(one[2].cpu(), low[i:i + 1].cpu()) < 2 * tol and rel_err(one[1].cpu(), iou[i:i + 1].cpu()) < 2 * tol, name
    # the numpy front end: boxes [N, 4] and points [N, P, 2] in image pixels; only a leading 1 is squeezed
    masks, iou, low = pred.predict(point_coords=pts5.numpy(), point_labels=lab5.numpy(), box=None, multimask_output=True)
    assert masks.shape == (5, 3, S, S) and iou.shape == (5, 3) and low.shape == (5, 3, S // 4, S // 4)
    masks, iou, low = pred.predict(box=box3[:1].numpy(), multimask_output=False)
    assert masks.shape == (1, S, S) and iou.shape == (1,) and low.shape == (1, S // 4, S // 4)


@pytest.mark.parametrize("skip_dtype", ["fp32", "op16"])
def test_shared_decoder_operands_bit_identical(model, skip_dtype, monkeypatch):
    import medical_sam2_amd.ops as ops
    shared = count_shared_shuffles(monkeypatch)
    m, _, _ = model
    dec = m.sam_mask_decoder
    E, n = S // 16, 16
    g = torch.Generator().manual_seed(21)
    dt = torch.float32 if skip_dtype == "fp32" else ops.OP16
    emb = torch.randn(1, 256, E, E, generator=g).to(DEV)
    pe = m.sam_prompt_encoder.get_dense_pe()
    sparse = torch.randn(n, 2, 256, generator=g).to(DEV)
    hr = [torch.randn(1, 32, 4 * E, 4 * E, generator=g).to(DEV, dt), torch.randn(1, 64, 2 * E, 2 * E, generator=g).to(DEV, dt)]
    for dense in (torch.randn(1, 256, 1, 1, generator=g).to(DEV).expand(1, 256, E, E), torch.randn(n, 256, E, E, generator=g).to(DEV)):
        del shared[:]
        a = dec(image_embeddings=emb, image_pe=pe, sparse_prompt_embeddings=sparse, dense_prompt_embeddings=dense, multimask_output=True,
                repeat_image=True, high_res_features=hr)
        assert shared == [n, n], shared                                 # the stride-0 path ran ...
        b = dec(image_embeddings=emb.expand(n, -1, -1, -1).contiguous(), image_pe=pe, sparse_prompt_embeddings=sparse,
                dense_prompt_embeddings=dense, multimask_output=True, repeat_image=True,
                high_res_features=[h.expand(n, -1, -1, -1).contiguous() for h in hr])
        assert shared == [n, n], shared                                 # ... and the repeated operands took the plain entries
        for x, y in zip(a, b):
            assert x.shape == y.shape and torch.equal(x, y)


def test_set_image_batch_predict_batch(model, tol):
    from medical_sam2_amd.image_predictor import SAM2ImagePredictor
    m, _, _ = model
    imgs = [blob_u8(5), blob_u8(6, 200, 300)]
    pts = [np.array([[[60.0, 80.0]], [[150.0, 40.0]]]), np.array([[120.0, 90.0], [30.0, 20.0]])]
    labs = [np.array([[1], [1]]), np.array([1, 0])]
    pred = SAM2ImagePredictor(m)
    with pytest.raises(AssertionError):
        pred.predict_batch(pts, labs)
    pred.set_image_batch(imgs)
    assert pred._is_batch and pred._orig_hw == [(S, S), (200, 300)]
    masks, ious, lows = pred.predict_batch(pts, labs, multimask_output=True)
    assert [x.shape for x in masks] == [(2, 3, S, S), (3, 200, 300)]
    assert [x.shape for x in ious] == [(2, 3), (3,)] and [x.shape for x in lows] == [(2, 3, S // 4, S // 4), (3, S // 4, S // 4)]
    for i, img in enumerate(imgs):
        alone = SAM2ImagePredictor(m)
        alone.set_image(img)
        mk, io, lo = alone.predict(pts[i], labs[i], multimask_output=True)
        assert mk.shape == masks[i].shape
        assert rel_err(lo, lows[i]) < 2 * tol and rel_err(io, ious[i]) < 2 * tol
    pred.reset_predictor()
    assert not pred._is_batch and not pred._is_image_set


def _kernel_logits(M, seed):
    g = torch.Generator().manual_seed(seed)
    smooth = torch.nn.functional.interpolate(torch.randn(M, 1, 16, 16, generator=g), size=(256, 256), mode="bilinear",
                                             align_corners=False)[:, 0] * 4
    edge = torch.full((6, 256, 256), -50.0)
    edge[0] = -3.0                                                  # all negative
    edge[1] = 3.0                                                   # all positive
    edge[2] = torch.where(torch.rand(256, 256, generator=g) > 0.5, 1.0, -1.0)   # values at thr +- off exactly
    edge[3] = torch.where(torch.rand(256, 256, generator=g) > 0.7, 1.0, 0.0)     # and at thr exactly
    edge[4, 0, 0] = 1.0                                             # tiny masks at the corners
    edge[5, 255, 255] = 1.0
    edge[5, 0, 255] = 1.0
    return torch.cat([smooth, edge]).contiguous()


@pytest.mark.parametrize("crop,frame", [((1024, 1024), (0, 0, 1024, 1024)), ((333, 517), (411, 250, 1000, 700)),
                                        ((1500, 1000), (0, 0, 1000, 1500)), ((1024, 1024), (37, 64, 1100, 1100))])
def test_mask_kernels_exact(crop, frame):
    import medical_sam2_amd.ops as ops
    h, w = crop
    x0, y0, W, H = frame
    logits = _kernel_logits(6, h + w).to(DEV)
    thr, off = 0.0, 1.0
    up = ops.bilinear_upsample(logits, h, w)
    counts, boxes = ops.mask_stats(logits, h, w, thr, off)
    ref_counts = torch.stack([(up > thr + off).sum((1, 2)), (up > thr - off).sum((1, 2)), (up > thr).sum((1, 2))], 1).to(torch.int32)
    assert torch.equal(counts.cpu(), ref_counts.cpu())
    binary = up > thr
    assert torch.equal(boxes.cpu().long(), R.boxes_of(binary))
    assert int(ref_counts[0, 2]) > 0 and int(ref_counts[6, 2]) == 0 and int(ref_counts[7, 2]) == h * w
    rles = ops.mask_rle(logits, h, w, (x0, y0), (H, W), thr)
    b = binary.cpu().numpy()
    for k in range(logits.shape[0]):
        full = np.zeros((H, W), dtype=bool)
        full[y0:y0 + h, x0:x0 + w] = b[k]
        assert rles[k] == R.rle_encode(full), k
    # another threshold and offset (values of the random planes sit on both sides)
    counts2, boxes2 = ops.mask_stats(logits, h, w, 0.5, 0.25)
    assert torch.equal(counts2.cpu()[:, 2], (up > 0.5).sum((1, 2)).to(torch.int32).cpu())
    assert torch.equal(counts2.cpu()[:, 0], (up > 0.75).sum((1, 2)).to(torch.int32).cpu())
    assert torch.equal(boxes2.cpu().long(), R.boxes_of(up > 0.5))


def test_mask_stats_graph_capture_and_replay():
    """Four replays over two logit sets into caller-owned counts, boxes and workspace, poisoned before every replay: the pre-sets of counts and
    of the workspace are nodes of the graph."""
    import medical_sam2_amd.ops as ops
    from medical_sam2_amd import _lib
    M, (lh, lw), (h, w), thr, off = 3, (8, 8), (32, 32), 0.0, 1.0
    sets = [torch.randn(M, lh, lw, generator=torch.Generator().manual_seed(seed)) * 4 for seed in (5, 6)]
    x = sets[0].to(DEV)
    counts = torch.empty(M, 3, dtype=torch.int32, device=DEV)
    boxes = torch.empty(M, 4, dtype=torch.int32, device=DEV)
    nb = _lib.lib().msam2_mask_stats_workspace_bytes(M)
    ws = torch.empty(nb // 4, dtype=torch.int32, device=DEV)

    def call():
        rc = _lib.lib().msam2_mask_stats(ops._p(x), M, lh, lw, h, w, thr, thr + off, thr - off, ops._p(counts), ops._p(boxes), ops._p(ws), nb,
                                         ops._stream())
        assert rc == 0, _lib.lib().msam2_last_error().decode()
    call()                                                          # eager first: nothing is set up inside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for logits in (sets[1], sets[0], sets[1], sets[0]):            # the replay reads what the buffer holds now
        x.copy_(logits.to(DEV))
        counts.fill_(-7), boxes.fill_(-7), ws.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        eager_counts, eager_boxes = ops.mask_stats(x, h, w, thr, off)
        assert torch.equal(counts, eager_counts) and torch.equal(boxes, eager_boxes)
        up = ops.bilinear_upsample(x, h, w)
        ref_counts = torch.stack([(up > thr + off).sum((1, 2)), (up > thr - off).sum((1, 2)), (up > thr).sum((1, 2))], 1).to(torch.int32)
        assert torch.equal(counts.cpu(), ref_counts.cpu()) and torch.equal(boxes.cpu().long(), R.boxes_of(up > thr))
        assert 0 < int(ref_counts[:, 2].min()) and int(ref_counts[:, 2].max()) < h * w          # not vacuous


@pytest.mark.parametrize("K", [0, 1, 7, 64, 1000, 5000, 16384])
def test_box_nms_exact(K):
    import medical_sam2_amd.ops as ops
    g = torch.Generator().manual_seed(K)
    xy = torch.randint(0, 200, (K, 2), generator=g).float()
    wh = torch.randint(0, 40, (K, 2), generator=g).float()            # includes zero-width / zero-height boxes
    boxes = torch.cat([xy, xy + wh], 1)
    if K >= 7:
        boxes[3] = boxes[1]                                             # exact duplicates
    scores = (torch.randint(0, 8, (K,), generator=g).float() / 8)     # many ties
    for thr in (0.7, 0.5, 1 / 3):
        got = ops.box_nms(boxes.to(DEV), scores.to(DEV), thr).cpu().tolist()
        assert got == R.nms_cpu(boxes.numpy(), scores.numpy(), thr), (K, thr)


def _records_equal(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert set(x) == set(y)
        for k in ("area", "bbox", "point_coords", "crop_box", "predicted_iou", "stability_score"):
            assert x[k] == y[k] and type(x[k]) is type(y[k]), (i, k, x[k], y[k])
        if isinstance(y["segmentation"], np.ndarray):
            assert x["segmentation"].dtype == bool and np.array_equal(x["segmentation"], y["segmentation"]), i
        else:
            assert x["segmentation"] == y["segmentation"], i


@pytest.mark.parametrize("case", ["ragged_binary", "crop_layer_rle", "m2m", "min_region"])
def test_generate_matches_restated_pipeline(model, case):
    from medical_sam2_amd.automatic_mask_generator import SAM2AutomaticMaskGenerator
    m, _, _ = model
    # random weights give many near-duplicate masks: a high NMS bar leaves enough records to compare (NMS still removes some)
    kw = dict(points_per_side=10, points_per_batch=64, output_mode="binary_mask", box_nms_thresh=0.95, crop_nms_thresh=0.95)
    image = blob_u8(9, 240, 256)
    if case == "crop_layer_rle":
        kw.update(crop_n_layers=1, output_mode="uncompressed_rle", points_per_side=6)
    elif case == "m2m":
        kw.update(use_m2m=True, output_mode="uncompressed_rle")
    elif case == "min_region":
        kw.update(min_mask_region_area=25)
    # thresholds from this fixture's own score distribution (random weights rarely reach the 0.8 / 0.95 defaults)
    cal = SAM2AutomaticMaskGenerator(m, pred_iou_thresh=0.0, stability_score_thresh=0.0, **kw)
    seen = {}
    R.generate(cal, image, seen)
    iou_thr = float(np.quantile(np.asarray(seen["ious"]), 0.15))
    stab_thr = float(np.nanquantile(np.asarray(seen["stabs"], dtype=np.float64), 0.15))
    gen = SAM2AutomaticMaskGenerator(m, pred_iou_thresh=iou_thr, stability_score_thresh=stab_thr, **kw)
    stats = {}
    ref = R.generate(gen, image, stats)
    got = gen.generate(image)
    _records_equal(got, ref)
    counts = (len(ref), stats["iou_removed"], stats["stab_removed"], stats["nms_removed"])
    # not vacuous: every filter and NMS removed masks, and records are left.  The masks of this random-weight model are few and nearly
    # coincide once refined (use_m2m: NMS keeps 3 of ~210 even at IoU 0.95) or filled (min_mask_region_area: 8 left; a denser grid
    # leaves no more), hence the lower bars of those two cases (all cases are deterministic)
    assert len(ref) >= {"m2m": 3, "min_region": 8}.get(case, 10) and min(counts[1:]) > 0, counts
