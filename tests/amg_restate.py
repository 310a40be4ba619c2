"""CPU / torch restatement of automatic mask generation, written from the behaviour of the reference pipeline
(sam2_train/automatic_mask_generator.py + utils/amg.py): the yardstick of tests/test_amg_cpu.py and tests/test_amg_gpu.py.  It works on
up-sampled high-res logits with plain torch reductions, encodes RLEs pixel by pixel and runs a greedy NMS in numpy fp32 -- the unfused
composition the device kernels replace."""
from typing import Any, Dict, List

import numpy as np
import torch


def nms_cpu(boxes: np.ndarray, scores: np.ndarray, thr: float) -> List[int]:
    """torchvision.ops.nms on the CPU: stable descending order, fp32 IoU = inter / (area_i + area_j - inter), suppress when the IoU
    (compared in double precision, as torchvision's C++ kernel does) exceeds thr."""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    s = np.asarray(scores, dtype=np.float32).reshape(-1)
    order = np.argsort(-s, kind="stable")
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    removed = np.zeros(len(b), dtype=bool)
    keep = []
    for r, i in enumerate(order):
        if removed[i]:
            continue
        keep.append(int(i))
        rest = order[r + 1:]
        xx1 = np.maximum(b[i, 0], b[rest, 0])
        yy1 = np.maximum(b[i, 1], b[rest, 1])
        xx2 = np.minimum(b[i, 2], b[rest, 2])
        yy2 = np.minimum(b[i, 3], b[rest, 3])
        inter = np.maximum(np.float32(0), xx2 - xx1) * np.maximum(np.float32(0), yy2 - yy1)
        with np.errstate(invalid="ignore", divide="ignore"):
            iou = inter / (area[i] + area[rest] - inter)
        removed[rest[iou.astype(np.float64) > thr]] = True
    return keep


def rle_encode(mask: np.ndarray) -> Dict[str, Any]:
    """Uncompressed RLE of a bool [h, w] mask: column-major runs alternating 0 / 1, starting with a 0-run (of length 0 if pixel 0 is set)."""
    h, w = mask.shape
    flat = np.asarray(mask, dtype=bool).T.reshape(-1)
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    edges = np.concatenate([[0], change, [h * w]])
    counts = np.diff(edges).tolist()
    if flat[0]:
        counts = [0] + counts
    return {"size": [h, w], "counts": [int(c) for c in counts]}


def boxes_of(binary: torch.Tensor) -> torch.Tensor:
    """Inclusive xyxy int64 boxes of bool [n, h, w] masks, zeros for an empty one."""
    n, h, w = binary.shape
    out = torch.zeros(n, 4, dtype=torch.int64)
    rows, cols = binary.any(-1).cpu(), binary.any(-2).cpu()
    for k in range(n):
        ys, xs = torch.nonzero(rows[k]).flatten(), torch.nonzero(cols[k]).flatten()
        if len(ys):
            out[k] = torch.tensor([int(xs[0]), int(ys[0]), int(xs[-1]), int(ys[-1])])
    return out


def _f32(x: float) -> torch.Tensor:
    return torch.tensor(x, dtype=torch.float32)


def generate(gen, image: np.ndarray, stats: Dict[str, int] = None) -> List[Dict[str, Any]]:
    """The pipeline on `gen`'s predictor and settings, stage by stage on high-res logits.  `stats` (optional) receives how many masks
    the iou filter, the stability filter and the NMS passes removed, and all iou / stability values seen."""
    from medical_sam2_amd import automatic_mask_generator as A
    st = stats if stats is not None else {}
    for k in ("iou_removed", "stab_removed", "nms_removed"):
        st.setdefault(k, 0)
    st.setdefault("ious", [])
    st.setdefault("stabs", [])
    pred = gen.predictor
    dev = pred.device
    H, W = image.shape[:2]
    ppb = gen.points_per_batch
    crop_boxes, layers = A.generate_crop_boxes((H, W), gen.crop_n_layers, gen.crop_overlap_ratio)
    per_crop = []
    for ci, (cb, li) in enumerate(zip(crop_boxes, layers)):
        x0, y0, x1, y1 = cb
        crop = image[y0:y1, x0:x1, :]
        ch, cw = crop.shape[:2]
        pred.set_image(crop)
        pts = gen.point_grids[li] * np.array([[cw, ch]])
        recs = {"rles": [], "boxes": [], "iou": [], "points": [], "stab": []}
        for s in range(0, len(pts), ppb):
            p = torch.as_tensor(pts[s:s + ppb], device=dev)
            ip = pred._transform_coords(p, True, (ch, cw))
            masks, iou, low = pred._predict(ip[:, None, :], torch.ones(len(ip), 1, dtype=torch.int, device=dev),
                                            multimask_output=gen.multimask_output, return_logits=True)
            nc = masks.shape[1]
            masks, iou, low, p = masks.flatten(0, 1), iou.flatten(0, 1), low.flatten(0, 1), p.repeat_interleave(nc, 0)
            if gen.use_m2m:
                rp = pred._transform_coords(p, True, (ch, cw))
                mm, ii = [], []
                for t in range(0, len(rp), ppb):
                    m2, i2, _ = pred._predict(rp[t:t + ppb, None, :], torch.ones(len(rp[t:t + ppb]), 1, dtype=torch.int, device=dev),
                                              mask_input=low[t:t + ppb, None], multimask_output=False, return_logits=True)
                    mm.append(m2)
                    ii.append(i2)
                masks, iou = torch.cat(mm).squeeze(1), torch.cat(ii).squeeze(1)
            st["ious"] += iou.cpu().tolist()
            if gen.pred_iou_thresh > 0.0:
                k = iou > gen.pred_iou_thresh
                st["iou_removed"] += int((~k).sum())
                masks, iou, p = masks[k], iou[k], p[k]
            inter = (masks > _f32(gen.mask_threshold + gen.stability_score_offset).to(dev)).sum((-1, -2)).to(torch.int32)
            union = (masks > _f32(gen.mask_threshold - gen.stability_score_offset).to(dev)).sum((-1, -2)).to(torch.int32)
            stab = inter / union
            st["stabs"] += stab.cpu().tolist()
            if gen.stability_score_thresh > 0.0:
                k = stab >= gen.stability_score_thresh
                st["stab_removed"] += int((~k).sum())
                masks, iou, p, stab = masks[k], iou[k], p[k], stab[k]
            binary = masks > _f32(gen.mask_threshold).to(dev)
            bx = boxes_of(binary)
            ub = (bx + torch.tensor([x0, y0, x0, y0])).float()
            near_crop = (ub - torch.tensor(cb, dtype=torch.float)).abs() <= 20.0
            near_img = (ub - torch.tensor([0, 0, W, H], dtype=torch.float)).abs() <= 20.0
            k = ~(near_crop & ~near_img).any(1)
            for j in torch.nonzero(k).flatten().tolist():
                full = np.zeros((H, W), dtype=bool)
                full[y0:y1, x0:x1] = binary[j].cpu().numpy()
                recs["rles"].append(rle_encode(full))
            recs["boxes"].append(bx[k])
            recs["iou"].append(iou[k.to(dev)].cpu())
            recs["points"].append(p[k.to(dev)].cpu())
            recs["stab"].append(stab[k.to(dev)].cpu())
        pred.reset_predictor()
        boxes, iou, points, stab = (torch.cat(recs[k]) for k in ("boxes", "iou", "points", "stab"))
        keep = nms_cpu(boxes.float().numpy(), iou.numpy(), gen.box_nms_thresh)
        st["nms_removed"] += len(boxes) - len(keep)
        per_crop.append({"rles": [recs["rles"][i] for i in keep], "boxes": boxes[keep] + torch.tensor([[x0, y0, x0, y0]]),
                         "iou": iou[keep], "points": points[keep] + torch.tensor([[x0, y0]]), "stab": stab[keep],
                         "crop": torch.tensor([cb] * len(keep), dtype=torch.int64).reshape(-1, 4)})
    d = {k: (sum((c[k] for c in per_crop), []) if k == "rles" else torch.cat([c[k] for c in per_crop])) for k in per_crop[0]}
    if len(crop_boxes) > 1:
        area = (d["crop"][:, 2] - d["crop"][:, 0]) * (d["crop"][:, 3] - d["crop"][:, 1])
        keep = nms_cpu(d["boxes"].float().numpy(), (1 / area).numpy(), gen.crop_nms_thresh)
        st["nms_removed"] += len(d["boxes"]) - len(keep)
        d = {k: ([v[i] for i in keep] if k == "rles" else v[keep]) for k, v in d.items()}
    out = []
    for i in range(len(d["rles"])):
        b = d["boxes"][i].float().numpy()
        c = d["crop"][i].float().numpy()
        rle = d["rles"][i]
        seg = {"binary_mask": None, "uncompressed_rle": rle}[gen.output_mode] if gen.output_mode != "binary_mask" else \
            np.repeat((np.arange(len(rle["counts"])) % 2).astype(bool), rle["counts"]).reshape(W, H).T
        out.append({"segmentation": seg, "area": int(sum(rle["counts"][1::2])),
                    "bbox": [float(b[0]), float(b[1]), float(b[2] - b[0]), float(b[3] - b[1])],
                    "predicted_iou": float(d["iou"][i].float().numpy()), "point_coords": [d["points"][i].float().numpy().tolist()],
                    "stability_score": float(d["stab"][i].float().numpy()),
                    "crop_box": [float(c[0]), float(c[1]), float(c[2] - c[0]), float(c[3] - c[1])]})
    return out
