"""Drop-in for `sam2_train/automatic_mask_generator.py` ("segment everything"): same constructor arguments and defaults, and
`generate(image)` returns the same records in the same order with the same Python types.

What differs is where the work happens.  The reference up-samples every batch of low-res logits to the crop size ([64, 3, 1024, 1024]
fp32 per 64-point batch at 1024^2), reads them again for the stability score, the boxes and an RLE built with nonzero() and a host loop
per mask, and runs torchvision's batched_nms.  Here each batch's low-res logits go through one fused pass (`ops.mask_stats`: both
stability counts, the area and the box, the bilinear up-sampling re-evaluated per pixel and never stored), NMS runs on the device
(`ops.box_nms`), only the survivors' low-res logits (256 KiB each) are kept, and they are run-length encoded on the device after NMS
(`ops.mask_rle`) with one copy of all counts to the host per crop.  Every quantity is bit-identical to the one computed from the
up-sampled logits, so the records are those of the reference pipeline on the same predictor outputs.

The helpers of `sam2_train/utils/amg.py` the pipeline needs (point grids, crop boxes, uncropping, the crop-edge test, RLE decoding) are
restated below from their behaviour.  `postprocess_small_regions` (OpenCV, never called by `generate`) is not provided.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import ops
from .image_predictor import SAM2ImagePredictor


# -- grids and crops -------------------------------------------------------------------------------------------------------------------
def build_point_grid(n_per_side: int) -> np.ndarray:
    """[n^2, 2] (x, y) points in [0, 1]^2, cell centres of an n x n grid, x varying fastest."""
    centres = np.linspace(1 / (2 * n_per_side), 1 - 1 / (2 * n_per_side), n_per_side)
    xs, ys = np.meshgrid(centres, centres)
    return np.stack([xs, ys], axis=-1).reshape(-1, 2)


def build_all_layer_point_grids(n_per_side: int, n_layers: int, scale_per_layer: int) -> List[np.ndarray]:
    """One grid per crop layer 0..n_layers; layer i has int(n_per_side / scale_per_layer**i) points per side."""
    return [build_point_grid(int(n_per_side / (scale_per_layer ** i))) for i in range(n_layers + 1)]


def generate_crop_boxes(im_size: Tuple[int, ...], n_layers: int, overlap_ratio: float) -> Tuple[List[List[int]], List[int]]:
    """xyxy crop boxes and their layer: the whole image (layer 0), then for layer i >= 1 a 2^i x 2^i tiling whose neighbours overlap by
    int(overlap_ratio * short side * 2 / 2^i) pixels, boxes ordered x-major (all y for the first x, ...)."""
    im_h, im_w = im_size
    short = min(im_h, im_w)
    boxes, layers = [[0, 0, im_w, im_h]], [0]
    for layer in range(1, n_layers + 1):
        n = 2 ** layer
        overlap = int(overlap_ratio * short * (2 / n))
        cw = int(math.ceil((overlap * (n - 1) + im_w) / n))
        ch = int(math.ceil((overlap * (n - 1) + im_h) / n))
        for x0 in [int((cw - overlap) * i) for i in range(n)]:
            for y0 in [int((ch - overlap) * i) for i in range(n)]:
                boxes.append([x0, y0, min(x0 + cw, im_w), min(y0 + ch, im_h)])
                layers.append(layer)
    return boxes, layers


def is_box_near_crop_edge(boxes: torch.Tensor, crop_box: List[int], orig_box: List[int], atol: float = 20.0) -> torch.Tensor:
    """Per crop-frame xyxy box: does any side lie within atol of the crop's border where that border is not the image's border."""
    off = torch.tensor([crop_box[0], crop_box[1], crop_box[0], crop_box[1]], device=boxes.device)
    b = (boxes + off).float()
    crop_t = torch.as_tensor(crop_box, dtype=torch.float, device=boxes.device)[None, :]
    orig_t = torch.as_tensor(orig_box, dtype=torch.float, device=boxes.device)[None, :]
    at_crop = torch.isclose(b, crop_t, atol=atol, rtol=0)
    at_image = torch.isclose(b, orig_t, atol=atol, rtol=0)
    return (at_crop & ~at_image).any(dim=1)


def box_xyxy_to_xywh(box: np.ndarray) -> np.ndarray:
    out = np.array(box, copy=True)
    out[2] = out[2] - out[0]
    out[3] = out[3] - out[1]
    return out


# -- RLE -------------------------------------------------------------------------------------------------------------------------------
def rle_to_mask(rle: Dict[str, Any]) -> np.ndarray:
    """bool [h, w] from an uncompressed RLE (runs alternate 0 / 1 starting with 0, column-major)."""
    h, w = rle["size"]
    counts = np.asarray(rle["counts"], dtype=np.int64)
    values = (np.arange(len(counts)) % 2).astype(bool)
    return np.repeat(values, counts).reshape(w, h).T


def area_from_rle(rle: Dict[str, Any]) -> int:
    """Pixels set: the odd-numbered runs."""
    return int(np.sum(rle["counts"][1::2], dtype=np.int64))


def coco_encode_rle(rle: Dict[str, Any]) -> Dict[str, Any]:
    """COCO's compressed RLE (pycocotools), counts as a str so that the record serialises to JSON."""
    from pycocotools import mask as coco_mask  # type: ignore

    enc = coco_mask.frPyObjects(rle, *rle["size"])
    enc["counts"] = enc["counts"].decode("utf-8")
    return enc


# -- the generator ---------------------------------------------------------------------------------------------------------------------
class SAM2AutomaticMaskGenerator:
    def __init__(self, model, points_per_side: Optional[int] = 32, points_per_batch: int = 64, pred_iou_thresh: float = 0.8,
                 stability_score_thresh: float = 0.95, stability_score_offset: float = 1.0, mask_threshold: float = 0.0,
                 box_nms_thresh: float = 0.7, crop_n_layers: int = 0, crop_nms_thresh: float = 0.7, crop_overlap_ratio: float = 512 / 1500,
                 crop_n_points_downscale_factor: int = 1, point_grids: Optional[List[np.ndarray]] = None, min_mask_region_area: int = 0,
                 output_mode: str = "binary_mask", use_m2m: bool = False, multimask_output: bool = True) -> None:
        assert (points_per_side is None) != (point_grids is None), "give points_per_side or point_grids (one of the two)"
        if points_per_side is not None:
            self.point_grids = build_all_layer_point_grids(points_per_side, crop_n_layers, crop_n_points_downscale_factor)
        else:
            self.point_grids = point_grids
        assert output_mode in ("binary_mask", "uncompressed_rle", "coco_rle"), f"output_mode {output_mode!r} is not one of binary_mask, uncompressed_rle, coco_rle"
        if output_mode == "coco_rle":
            import pycocotools.mask  # type: ignore  # noqa: F401  (ImportError where it is absent, as upstream)
        self.predictor = SAM2ImagePredictor(model, max_hole_area=min_mask_region_area, max_sprinkle_area=min_mask_region_area)
        self.points_per_batch = points_per_batch
        self.pred_iou_thresh = pred_iou_thresh
        self.stability_score_thresh = stability_score_thresh
        self.stability_score_offset = stability_score_offset
        self.mask_threshold = mask_threshold
        self.box_nms_thresh = box_nms_thresh
        self.crop_n_layers = crop_n_layers
        self.crop_nms_thresh = crop_nms_thresh
        self.crop_overlap_ratio = crop_overlap_ratio
        self.crop_n_points_downscale_factor = crop_n_points_downscale_factor
        self.min_mask_region_area = min_mask_region_area
        self.output_mode = output_mode
        self.use_m2m = use_m2m
        self.multimask_output = multimask_output

    @torch.no_grad()
    def generate(self, image: np.ndarray) -> List[Dict[str, Any]]:
        """Records of every mask found in the HWC uint8 `image`: segmentation (bool HxW array, or an RLE dict), area, bbox (xywh),
        predicted_iou, point_coords, stability_score, crop_box (xywh)."""
        d = self._generate_masks(image)
        if self.output_mode == "coco_rle":
            segs = [coco_encode_rle(r) for r in d["rles"]]
        elif self.output_mode == "binary_mask":
            segs = [rle_to_mask(r) for r in d["rles"]]
        else:
            segs = d["rles"]
        return [{"segmentation": segs[i], "area": area_from_rle(d["rles"][i]), "bbox": box_xyxy_to_xywh(d["boxes"][i]).tolist(),
                 "predicted_iou": d["iou_preds"][i].item(), "point_coords": [d["points"][i].tolist()],
                 "stability_score": d["stability_score"][i].item(), "crop_box": box_xyxy_to_xywh(d["crop_boxes"][i]).tolist()}
                for i in range(len(segs))]

    def _generate_masks(self, image: np.ndarray) -> Dict[str, Any]:
        orig_size = image.shape[:2]
        crop_boxes, crop_layers = generate_crop_boxes(image.shape[:2], self.crop_n_layers, self.crop_overlap_ratio)
        crops = [self._process_crop(image, cb, li, orig_size) for cb, li in zip(crop_boxes, crop_layers)]
        dev = self.predictor.device
        cat = lambda k: torch.cat([c[k] for c in crops], 0)
        boxes, iou, points, stab = cat("boxes"), cat("iou_preds"), cat("points"), cat("stability_score")
        crop_of = torch.cat([torch.full((c["boxes"].shape[0],), i, dtype=torch.int64) for i, c in enumerate(crops)], 0)
        local = torch.cat([torch.arange(c["boxes"].shape[0], dtype=torch.int64) for c in crops], 0)
        crop_tab = torch.tensor(crop_boxes, dtype=torch.int64)
        if len(crop_boxes) > 1:
            # across crops: the mask from the smaller crop wins (score 1 / crop area, ties to the earlier record)
            areas = (crop_tab[crop_of, 2] - crop_tab[crop_of, 0]) * (crop_tab[crop_of, 3] - crop_tab[crop_of, 1])
            keep = ops.box_nms(boxes.float(), (1 / areas).to(dev), self.crop_nms_thresh).cpu()
            boxes, iou, points, stab = boxes[keep.to(dev)], iou[keep.to(dev)], points[keep.to(dev)], stab[keep.to(dev)]
            crop_of, local = crop_of[keep], local[keep]
        # run-length encode the survivors, one device pass and one copy to the host per crop
        rles: List[Optional[Dict[str, Any]]] = [None] * len(crop_of)
        for ci, c in enumerate(crops):
            sel = (crop_of == ci).nonzero().flatten()
            if sel.numel() == 0:
                continue
            x0, y0, x1, y1 = crop_boxes[ci]
            logits = c["logits"][local[sel].to(dev)].contiguous()
            for j, r in zip(sel.tolist(), ops.mask_rle(logits, y1 - y0, x1 - x0, (x0, y0), orig_size, self.mask_threshold)):
                rles[j] = r
        return {"rles": rles, "boxes": boxes.float().cpu().numpy(), "iou_preds": iou.float().cpu().numpy(),
                "points": points.float().cpu().numpy(), "stability_score": stab.float().cpu().numpy(),
                "crop_boxes": crop_tab[crop_of].float().numpy()}

    def _process_crop(self, image: np.ndarray, crop_box: List[int], crop_layer_idx: int, orig_size: Tuple[int, ...]) -> Dict[str, Any]:
        x0, y0, x1, y1 = crop_box
        cropped = image[y0:y1, x0:x1, :]
        crop_hw = cropped.shape[:2]
        self.predictor.set_image(cropped)
        pts = self.point_grids[crop_layer_idx] * np.array(crop_hw)[None, ::-1]
        parts = [self._process_batch(pts[s: s + self.points_per_batch], crop_hw, crop_box, orig_size)
                 for s in range(0, len(pts), self.points_per_batch)]
        self.predictor.reset_predictor()
        d = {k: torch.cat([p[k] for p in parts], 0) for k in parts[0]}
        keep = ops.box_nms(d["boxes"].float(), d["iou_preds"], self.box_nms_thresh)
        d = {k: v[keep] for k, v in d.items()}
        dev = d["boxes"].device
        d["boxes"] = d["boxes"] + torch.tensor([[x0, y0, x0, y0]], device=dev)
        d["points"] = d["points"] + torch.tensor([[x0, y0]], device=dev)
        return d

    def _process_batch(self, points: np.ndarray, im_size: Tuple[int, ...], crop_box: List[int], orig_size: Tuple[int, ...]) -> Dict[str, torch.Tensor]:
        orig_h, orig_w = orig_size
        pred = self.predictor
        points = torch.as_tensor(points, device=pred.device)
        in_points = pred._transform_coords(points, True, im_size)
        in_labels = torch.ones_like(in_points[:, 0], dtype=torch.int)
        logits, iou, low_res = pred._predict_low_res(in_points[:, None, :], in_labels[:, None], multimask_output=self.multimask_output)
        n_out = logits.shape[1]
        logits, iou, low_res = logits.flatten(0, 1), iou.flatten(0, 1), low_res.flatten(0, 1)
        points = points.repeat_interleave(n_out, dim=0)
        if self.use_m2m:
            # refine_with_m2m: every mask once more, its clamped low-res logits as the mask prompt, one output per prompt
            rp = pred._transform_coords(points, True, im_size)
            rl = torch.ones(rp.shape[0], dtype=torch.int, device=rp.device)
            outs = [pred._predict_low_res(rp[s: s + self.points_per_batch, None, :], rl[s: s + self.points_per_batch, None],
                                          mask_input=low_res[s: s + self.points_per_batch, None, :], multimask_output=False)
                    for s in range(0, rp.shape[0], self.points_per_batch)]
            logits = torch.cat([o[0] for o in outs], 0).squeeze(1)
            iou = torch.cat([o[1] for o in outs], 0).squeeze(1)
        if self.pred_iou_thresh > 0.0:
            keep = iou > self.pred_iou_thresh
            logits, iou, points = logits[keep], iou[keep], points[keep]
        logits = logits.contiguous()
        counts, boxes = ops.mask_stats(logits, im_size[0], im_size[1], self.mask_threshold, self.stability_score_offset)
        stability = counts[:, 0] / counts[:, 1]
        boxes = boxes.long()
        if self.stability_score_thresh > 0.0:
            keep = stability >= self.stability_score_thresh
            logits, iou, points, stability, boxes = logits[keep], iou[keep], points[keep], stability[keep], boxes[keep]
        keep = ~is_box_near_crop_edge(boxes, crop_box, [0, 0, orig_w, orig_h])
        return {"logits": logits[keep], "iou_preds": iou[keep], "points": points[keep], "stability_score": stability[keep], "boxes": boxes[keep]}
