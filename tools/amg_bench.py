#!/usr/bin/env python3
"""Automatic mask generation at 1024^2 (hiera_s, random weights, a blob image, 32 x 32 grid, 64 points per batch):

- `SAM2AutomaticMaskGenerator.generate()` wall time;
- the decoder on one 64-point batch: shared image operands (stride 0) against explicitly repeated ones;
- the post-processing of one 64-point batch ([192, 256, 256] low-res logits): the fused kernels (mask_stats + mask_rle) against the
  unfused composition of the reference (bilinear_upsample to [192, 1024, 1024] + torch reductions for the stability counts and boxes + a
  torch RLE with nonzero() and a host copy per mask), with the peak device memory of each.

Prints one line per figure and a JSON line at the end."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import medical_sam2_amd.build_sam as bs  # noqa: E402
import medical_sam2_amd.ops as ops  # noqa: E402
import medical_sam2_amd.synthetic as syn  # noqa: E402
import medical_sam2_amd.weights as wts  # noqa: E402
from medical_sam2_amd.automatic_mask_generator import SAM2AutomaticMaskGenerator  # noqa: E402

S = 1024


def wall(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def unfused(logits, h, w, thr=0.0, off=1.0):
    """What the reference does per batch: high-res logits, then stability / boxes / RLE from them."""
    up = ops.bilinear_upsample(logits, h, w)
    inter = (up > thr + off).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
    union = (up > thr - off).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
    stab = inter / union
    m = up > thr
    rows, cols = m.any(-1), m.any(-2)
    ar_h, ar_w = torch.arange(h, device=m.device), torch.arange(w, device=m.device)
    bottom = (rows * ar_h).amax(-1)
    top = (rows * ar_h + h * ~rows).amin(-1)
    right = (cols * ar_w).amax(-1)
    left = (cols * ar_w + w * ~cols).amin(-1)
    boxes = torch.stack([left, top, right, bottom], -1)
    flat = m.permute(0, 2, 1).flatten(1)
    change = (flat[:, 1:] ^ flat[:, :-1]).nonzero()
    rles = []
    for i in range(flat.shape[0]):
        idx = change[change[:, 0] == i, 1]
        idx = torch.cat([idx.new_zeros(1), idx + 1, idx.new_full((1,), h * w)])
        counts = [] if not bool(flat[i, 0]) else [0]
        counts.extend((idx[1:] - idx[:-1]).cpu().tolist())
        rles.append(counts)
    return stab, boxes, rles


def fused(logits, h, w, thr=0.0, off=1.0):
    counts, boxes = ops.mask_stats(logits, h, w, thr, off)
    stab = counts[:, 0] / counts[:, 1]
    rles = ops.mask_rle(logits, h, w, (0, 0), (h, w), thr)
    return stab, boxes, rles


def main():
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    m = bs.build_sam2("sam2_hiera_s", device="cpu")
    m.load_state_dict(wts.init_weights("hiera_s", 0), strict=True)
    m = m.to(dev).eval()
    img, _ = syn.blob_image(0, S)
    u8 = img.clamp(0, 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().numpy()
    res = {}

    gen = SAM2AutomaticMaskGenerator(m, points_per_side=32, points_per_batch=64)
    t_gen = wall(lambda: gen.generate(u8), reps=3, warm=1)
    low = SAM2AutomaticMaskGenerator(m, points_per_side=32, points_per_batch=64, pred_iou_thresh=0.0, stability_score_thresh=0.0)
    t_gen0 = wall(lambda: low.generate(u8), reps=3, warm=1)
    n_rec = len(low.generate(u8))
    res.update(generate_s=t_gen, generate_no_filters_s=t_gen0, records_no_filters=n_rec)
    print(f"generate(): {t_gen * 1e3:.1f} ms at the default thresholds, {t_gen0 * 1e3:.1f} ms with the score filters off ({n_rec} records)")

    pred = gen.predictor
    pred.set_image(u8)
    pts = torch.as_tensor(gen.point_grids[0][:64] * S, device=dev)
    ip = pred._transform_coords(pts, True, (S, S))[:, None, :]
    lab = torch.ones(64, 1, dtype=torch.int, device=dev)
    t_dec = wall(lambda: pred._predict_low_res(ip, lab), reps=10)
    feats = pred._features
    sparse, dense = m.sam_prompt_encoder(points=(ip, lab), boxes=None, masks=None)
    pe = m.sam_prompt_encoder.get_dense_pe()
    hr1 = feats["high_res_feats"]
    emb1 = feats["image_embed"]

    def shared():
        return m.sam_mask_decoder(image_embeddings=emb1, image_pe=pe, sparse_prompt_embeddings=sparse, dense_prompt_embeddings=dense,
                                  multimask_output=True, repeat_image=True, high_res_features=hr1)

    def materialised():
        return m.sam_mask_decoder(image_embeddings=emb1.expand(64, -1, -1, -1).contiguous(), image_pe=pe, sparse_prompt_embeddings=sparse,
                                  dense_prompt_embeddings=dense, multimask_output=True, repeat_image=True,
                                  high_res_features=[f.expand(64, -1, -1, -1).contiguous() for f in hr1])
    t_sh, t_mat = wall(shared, reps=10), wall(materialised, reps=10)
    p_sh, p_mat = peak(shared), peak(materialised)
    res.update(predict_batch64_s=t_dec, decoder_shared_s=t_sh, decoder_materialised_s=t_mat, decoder_shared_peak_bytes=p_sh,
               decoder_materialised_peak_bytes=p_mat)
    print(f"decoder, 64 prompt sets: shared operands {t_sh * 1e3:.2f} ms (peak {p_sh / 2**20:.0f} MiB), materialised "
          f"{t_mat * 1e3:.2f} ms (peak {p_mat / 2**20:.0f} MiB); _predict_low_res of the batch {t_dec * 1e3:.2f} ms")

    logits, _, _ = pred._predict_low_res(ip, lab)
    logits = logits.flatten(0, 1).contiguous()                   # [192, 256, 256]
    fs, fb, fr = fused(logits, S, S)
    us, ub, ur = unfused(logits, S, S)
    same = torch.equal(fs, us) or torch.equal(torch.nan_to_num(fs, nan=-1.0), torch.nan_to_num(us, nan=-1.0))
    assert same and torch.equal(fb.long(), ub.long()) and [r["counts"] for r in fr] == ur, "fused and unfused post-processing disagree"
    t_stats = wall(lambda: ops.mask_stats(logits, S, S, 0.0, 1.0), reps=20)
    t_f, t_u = wall(lambda: fused(logits, S, S)), wall(lambda: unfused(logits, S, S), reps=3, warm=1)
    up_only = wall(lambda: ops.bilinear_upsample(logits, S, S), reps=20)
    pf, pu = peak(lambda: fused(logits, S, S)), peak(lambda: unfused(logits, S, S))
    res.update(post_fused_s=t_f, post_unfused_s=t_u, mask_stats_s=t_stats, upsample_only_s=up_only, post_fused_peak_bytes=pf,
               post_unfused_peak_bytes=pu, masks_per_batch=int(logits.shape[0]))
    print(f"post-processing of one batch ({logits.shape[0]} masks at {S}^2): fused {t_f * 1e3:.2f} ms (mask_stats alone {t_stats * 1e3:.3f} ms, "
          f"peak {pf / 2**20:.1f} MiB) | unfused {t_u * 1e3:.2f} ms (bilinear_upsample alone {up_only * 1e3:.3f} ms, peak {pu / 2**20:.0f} MiB)")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
