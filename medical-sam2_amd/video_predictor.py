"""Drop-in for `sam2_train/sam2_video_predictor.py` (SAM2VideoPredictor): the interactive / volumetric state machine on top of the
MI355X `SAM2Base` mirror -- same method names, arguments, `inference_state` keys and return values, so `func_3d/function.py`
and the upstream notebooks drive it unchanged:

    state = predictor.val_init_state(imgs_tensor)              | init_state(jpeg_dir)          (sam2_video_predictor.py:39-177)
    predictor.add_new_points / add_new_bbox / add_new_mask(...)                                (293-423, 557-639)
    for frame_idx, obj_ids, video_res_masks in predictor.propagate_in_video(state): ...        (1041-1124)

What is re-designed without changing any result:
  * the reference caches the backbone features of ONE frame (`cached_features = {frame_idx: ...}`, 1270-1281), so every prompted
    slice is encoded twice (once when the prompt is added, once when its memory is encoded in the preflight) and every revisit
    re-runs the image encoder.  Here the cache keeps every frame (`feature_cache_frames`, default: all of them -- 17 MB per
    1024^2 slice in fp32, 288 GB of HBM) and `prefetch_features` encodes the not-yet-seen frames in batches, where the trunk's
    kernels are far better filled than at batch 1;
  * frames are normalised on the device by one kernel-free broadcast; hole filling runs the batched HIP connected-components
    path (`ops.fill_holes_`); resizing uses the HIP bilinear kernel.
The `train_*` entry points of the fork (179-248, 425-555, 641-722, 971-1039, 1126-1208: the same code without
`torch.inference_mode`) are the same method bodies run WITHOUT `torch.no_grad()`: with the net in `train()` mode every `track_step` /
`_encode_new_memory` / `forward_image` then goes through the torch.autograd bridge (`autograd.py`), the state machine's own arithmetic
(resizes, per-object consolidation, hole filling) stays differentiable torch, and the loop of `func_3d/function.py:130-191` --
`train_add_new_* -> train_propagate_in_video -> non_prompt_loss.backward(retain_graph=True) / prompt_loss.backward() ->
optimizer.step()` -- runs against this class as written.  (The explicit, graph-capturable training steps live in `training*.py`.)

PROVENANCE: this file is a DERIVED work, not a re-design.  SURVEY.md section 2 #13 marks the predictor state machine "keep as-is": its
`inference_state` dictionary layout, method signatures and the order of the consolidation / preflight / propagation steps ARE the
contract that `func_3d/function.py` and the notebooks program against, so the host-side control flow below follows
`sam2_train/sam2_video_predictor.py` step by step (condensed; the hot path it drives -- `SAM2Base.track_step` and everything under it
-- is the from-scratch HIP implementation).  It is not counted as original work in DESIGN.md.
"""
from __future__ import annotations

import os
from collections import OrderedDict
from typing import Optional

import numpy as np
import torch

from . import ops
from .modeling.sam2_base import NO_OBJ_SCORE, SAM2Base

F32 = torch.float32
_IMG_MEAN = (0.485, 0.456, 0.406)
_IMG_STD = (0.229, 0.224, 0.225)


def concat_points(old_point_inputs, new_points, new_labels):
    """utils/misc.py:261-269."""
    if old_point_inputs is None:
        points, labels = new_points, new_labels
    else:
        points = torch.cat([old_point_inputs["point_coords"], new_points], dim=1)
        labels = torch.cat([old_point_inputs["point_labels"], new_labels], dim=1)
    return {"point_coords": points, "point_labels": labels}


def _normalise(images: torch.Tensor, device) -> torch.Tensor:
    """(x - mean) / std per channel, fp32 (utils/misc.py:205-211, 240-244)."""
    images = images.to(device=device, dtype=F32)
    mean = torch.tensor(_IMG_MEAN, dtype=F32, device=device)[:, None, None]
    std = torch.tensor(_IMG_STD, dtype=F32, device=device)[:, None, None]
    return (images - mean) / std


def load_video_frames_from_data(imgs_tensor: torch.Tensor, offload_video_to_cpu: bool = False, async_loading_frames: bool = False):
    """utils/misc.py:215-244: [T,3,S,S] values in 0..255 -> normalised fp32 frames."""
    dev = torch.device("cpu") if offload_video_to_cpu else torch.device("cuda")
    return _normalise(imgs_tensor / 255.0, dev)


def load_video_frames(video_path, image_size: int, offload_video_to_cpu: bool = False, async_loading_frames: bool = False):
    """utils/misc.py:163-212: a directory of "<frame_index>.jpg" files, resized to image_size (PIL bilinear-free default resize,
    like the reference) and normalised."""
    from PIL import Image
    if not (isinstance(video_path, str) and os.path.isdir(video_path)):
        raise NotImplementedError("Only JPEG frames are supported at this moment")
    names = [p for p in os.listdir(video_path) if os.path.splitext(p)[-1] in [".jpg", ".jpeg", ".JPG", ".JPEG"]]
    names.sort(key=lambda p: int(os.path.splitext(p)[0]))
    if not names:
        raise RuntimeError(f"no images found in {video_path}")
    images = torch.zeros(len(names), 3, image_size, image_size, dtype=F32)
    video_height = video_width = None
    for n, name in enumerate(names):
        img_pil = Image.open(os.path.join(video_path, name))
        img_np = np.array(img_pil.convert("RGB").resize((image_size, image_size)))
        if img_np.dtype != np.uint8:
            raise RuntimeError(f"Unknown image dtype: {img_np.dtype} on {name}")
        images[n] = torch.from_numpy(img_np / 255.0).permute(2, 0, 1)
        video_width, video_height = img_pil.size
    dev = torch.device("cpu") if offload_video_to_cpu else torch.device("cuda")
    return _normalise(images, dev), video_height, video_width


class SAM2VideoPredictor(SAM2Base):
    """sam2_video_predictor.py:17-1441 (see the module docstring for the mapping)."""

    def __init__(self, fill_hole_area=0, non_overlap_masks=False, clear_non_cond_mem_around_input=False,
                 clear_non_cond_mem_for_multi_obj=False, feature_cache_frames: Optional[int] = None, use_hip_graphs: bool = False,
                 **kwargs):
        super().__init__(**kwargs)
        # replay the prompt-free per-frame forward of propagate_in_video as hipGraphs (graphs.GraphedPropagation: one graph per
        # memory-bank bucket).  Off by default: the graphs bake in the current weights and hold their own activation pool.
        self.use_hip_graphs = use_hip_graphs
        self.fill_hole_area = fill_hole_area
        self.non_overlap_masks = non_overlap_masks
        self.clear_non_cond_mem_around_input = clear_non_cond_mem_around_input
        self.clear_non_cond_mem_for_multi_obj = clear_non_cond_mem_for_multi_obj
        self.feature_cache_frames = feature_cache_frames     # None = keep every frame's features (reference: 1)

    # ------------------------------------------------------------------------------------------------------------ state
    def _new_state(self, images, video_height, video_width, offload_video_to_cpu, offload_state_to_cpu):
        dev = torch.device("cuda")
        s = {
            "images": images, "num_frames": len(images), "offload_video_to_cpu": offload_video_to_cpu,
            "offload_state_to_cpu": offload_state_to_cpu, "video_height": video_height, "video_width": video_width,
            "device": dev, "storage_device": torch.device("cpu") if offload_state_to_cpu else dev,
            "point_inputs_per_obj": {}, "mask_inputs_per_obj": {}, "cached_features": {}, "constants": {},
            "obj_id_to_idx": OrderedDict(), "obj_idx_to_id": OrderedDict(), "obj_ids": [],
            "output_dict": {"cond_frame_outputs": {}, "non_cond_frame_outputs": {}},
            "output_dict_per_obj": {}, "temp_output_dict_per_obj": {},
            "consolidated_frame_inds": {"cond_frame_outputs": set(), "non_cond_frame_outputs": set()},
            "tracking_has_started": False, "frames_already_tracked": {},
        }
        # warm up the backbone and cache frame 0, like the reference
        self._get_image_feature(s, frame_idx=0, batch_size=1)
        return s

    @torch.no_grad()
    def init_state(self, video_path, offload_video_to_cpu=False, offload_state_to_cpu=False, async_loading_frames=False):
        images, h, w = load_video_frames(video_path, self.image_size, offload_video_to_cpu, async_loading_frames)
        return self._new_state(images, h, w, offload_video_to_cpu, offload_state_to_cpu)

    def _val_init_state(self, imgs_tensor, video_height=None, video_width=None, offload_video_to_cpu=False,
                       offload_state_to_cpu=False, async_loading_frames=False):
        if video_height is None or video_width is None:
            video_height = video_width = self.image_size
        images = load_video_frames_from_data(imgs_tensor, offload_video_to_cpu, async_loading_frames)
        return self._new_state(images, video_height, video_width, offload_video_to_cpu, offload_state_to_cpu)

    @torch.no_grad()
    def init_state_from_volume(self, raw, window=None, video_height=None, video_width=None, offload_state_to_cpu=False, **prepare_args):
        """State from a raw slice stack ([T, H0, W0] or [T, Cin, H0, W0]; uint8, int16 or float32; window: see volume_prep.prepare_volume):
        windowed, resized as Pillow does and normalised on the device, where the frames stay.  video_height / video_width default to the
        model's input size, as in val_init_state: masks then come out on the grid of volume_prep.prepare_labels."""
        from .volume_prep import prepare_volume
        if video_height is None or video_width is None:
            video_height = video_width = self.image_size
        images = prepare_volume(raw, window, size=self.image_size, **prepare_args)
        return self._new_state(images, video_height, video_width, False, offload_state_to_cpu)

    def _obj_id_to_idx(self, inference_state, obj_id):
        obj_idx = inference_state["obj_id_to_idx"].get(obj_id, None)
        if obj_idx is not None:
            return obj_idx
        if inference_state["tracking_has_started"]:
            raise RuntimeError(f"Cannot add new object id {obj_id} after tracking starts. "
                               f"All existing object ids: {inference_state['obj_ids']}. "
                               f"Please call 'reset_state' to restart from scratch.")
        obj_idx = len(inference_state["obj_id_to_idx"])
        inference_state["obj_id_to_idx"][obj_id] = obj_idx
        inference_state["obj_idx_to_id"][obj_idx] = obj_id
        inference_state["obj_ids"] = list(inference_state["obj_id_to_idx"])
        inference_state["point_inputs_per_obj"][obj_idx] = {}
        inference_state["mask_inputs_per_obj"][obj_idx] = {}
        inference_state["output_dict_per_obj"][obj_idx] = {"cond_frame_outputs": {}, "non_cond_frame_outputs": {}}
        inference_state["temp_output_dict_per_obj"][obj_idx] = {"cond_frame_outputs": {}, "non_cond_frame_outputs": {}}
        return obj_idx

    def _obj_idx_to_id(self, inference_state, obj_idx):
        return inference_state["obj_idx_to_id"][obj_idx]

    def _get_obj_num(self, inference_state):
        return len(inference_state["obj_idx_to_id"])

    # ---------------------------------------------------------------------------------------------------------- prompts
    def _frame_role(self, inference_state, frame_idx):
        is_init_cond_frame = frame_idx not in inference_state["frames_already_tracked"]
        reverse = False if is_init_cond_frame else inference_state["frames_already_tracked"][frame_idx]["reverse"]
        is_cond = is_init_cond_frame or self.add_all_frames_to_correct_as_cond
        return is_init_cond_frame, reverse, is_cond, ("cond_frame_outputs" if is_cond else "non_cond_frame_outputs")

    def _finish_interaction(self, inference_state, frame_idx, is_cond):
        consolidated_out = self._consolidate_temp_output_across_obj(inference_state, frame_idx, is_cond=is_cond, run_mem_encoder=False,
                                                                    consolidate_at_video_res=True)
        _, video_res_masks = self._get_orig_video_res_output(inference_state, consolidated_out["pred_masks_video_res"])
        return frame_idx, inference_state["obj_ids"], video_res_masks

    def _add_new_points(self, inference_state, frame_idx, obj_id, points, labels, clear_old_points=True, normalize_coords=True):
        obj_idx = self._obj_id_to_idx(inference_state, obj_id)
        point_inputs_per_frame = inference_state["point_inputs_per_obj"][obj_idx]
        mask_inputs_per_frame = inference_state["mask_inputs_per_obj"][obj_idx]
        if not isinstance(points, torch.Tensor):
            points = torch.tensor(points, dtype=F32)
        if not isinstance(labels, torch.Tensor):
            labels = torch.tensor(labels, dtype=torch.int32)
        if points.dim() == 2:
            points = points.unsqueeze(0)
        if labels.dim() == 1:
            labels = labels.unsqueeze(0)
        if normalize_coords:
            scale = torch.tensor([inference_state["video_width"], inference_state["video_height"]]).to(points.device)
            points = points / scale
        points = (points * self.image_size).to(inference_state["device"])
        labels = labels.to(inference_state["device"])
        point_inputs = concat_points(None if clear_old_points else point_inputs_per_frame.get(frame_idx, None), points, labels)
        point_inputs_per_frame[frame_idx] = point_inputs
        mask_inputs_per_frame.pop(frame_idx, None)
        is_init_cond_frame, reverse, is_cond, storage_key = self._frame_role(inference_state, frame_idx)
        obj_output_dict = inference_state["output_dict_per_obj"][obj_idx]
        obj_temp_output_dict = inference_state["temp_output_dict_per_obj"][obj_idx]
        # previous mask logits of this object on this frame feed the SAM decoder together with the new clicks
        prev_out = obj_temp_output_dict[storage_key].get(frame_idx)
        if prev_out is None:
            prev_out = obj_output_dict["cond_frame_outputs"].get(frame_idx)
            if prev_out is None:
                prev_out = obj_output_dict["non_cond_frame_outputs"].get(frame_idx)
        prev_sam_mask_logits = None
        if prev_out is not None and prev_out["pred_masks"] is not None:
            prev_sam_mask_logits = torch.clamp(prev_out["pred_masks"].to(inference_state["device"], non_blocking=True), -32.0, 32.0)
        current_out, _ = self._run_single_frame_inference(
            inference_state=inference_state, output_dict=obj_output_dict, frame_idx=frame_idx, batch_size=1,
            is_init_cond_frame=is_init_cond_frame, point_inputs=point_inputs, mask_inputs=None, reverse=reverse,
            run_mem_encoder=False, prev_sam_mask_logits=prev_sam_mask_logits)
        obj_temp_output_dict[storage_key][frame_idx] = current_out
        return self._finish_interaction(inference_state, frame_idx, is_cond)

    def _add_new_bbox(self, inference_state, frame_idx, obj_id, bbox, clear_old_points=True, normalize_coords=True):
        if not isinstance(bbox, torch.Tensor):
            bbox = torch.tensor(bbox, dtype=F32)
        return self._add_new_points(inference_state=inference_state, frame_idx=frame_idx, obj_id=obj_id, points=bbox.reshape(-1, 2, 2),
                                   labels=torch.tensor([2, 3], dtype=torch.int), clear_old_points=clear_old_points,
                                   normalize_coords=normalize_coords)

    def _add_new_mask(self, inference_state, frame_idx, obj_id, mask):
        obj_idx = self._obj_id_to_idx(inference_state, obj_id)
        point_inputs_per_frame = inference_state["point_inputs_per_obj"][obj_idx]
        mask_inputs_per_frame = inference_state["mask_inputs_per_obj"][obj_idx]
        if not isinstance(mask, torch.Tensor):
            mask = torch.tensor(mask, dtype=torch.bool)
        assert mask.dim() == 2
        mask_H, mask_W = mask.shape
        mask_inputs_orig = mask[None, None].float().to(inference_state["device"])
        if mask_H != self.image_size or mask_W != self.image_size:
            mask_inputs = torch.nn.functional.interpolate(mask_inputs_orig, size=(self.image_size, self.image_size), align_corners=False,
                                                          mode="bilinear", antialias=True)
            mask_inputs = (mask_inputs >= 0.5).float()
        else:
            mask_inputs = mask_inputs_orig
        mask_inputs_per_frame[frame_idx] = mask_inputs
        point_inputs_per_frame.pop(frame_idx, None)
        is_init_cond_frame, reverse, is_cond, storage_key = self._frame_role(inference_state, frame_idx)
        current_out, _ = self._run_single_frame_inference(
            inference_state=inference_state, output_dict=inference_state["output_dict_per_obj"][obj_idx], frame_idx=frame_idx,
            batch_size=1, is_init_cond_frame=is_init_cond_frame, point_inputs=None, mask_inputs=mask_inputs, reverse=reverse,
            run_mem_encoder=False)
        inference_state["temp_output_dict_per_obj"][obj_idx][storage_key][frame_idx] = current_out
        return self._finish_interaction(inference_state, frame_idx, is_cond)

    # ---------------------------------------------------------------------------------------------------- consolidation
    def _resize(self, masks: torch.Tensor, H: int, W: int) -> torch.Tensor:
        """F.interpolate(mode="bilinear", align_corners=False) on [n,1,h,w] fp32 (HIP kernel)."""
        if masks.shape[-2:] == (H, W):
            return masks
        if torch.is_grad_enabled() and masks.requires_grad:      # train_* twins: keep the graph (the same kernel behind an autograd Function)
            from .autograd import bilinear_upsample
            return bilinear_upsample(masks, H, W)
        return ops.bilinear_upsample(masks.to(F32).contiguous(), H, W)

    def _get_orig_video_res_output(self, inference_state, any_res_masks):
        device = inference_state["device"]
        any_res_masks = any_res_masks.to(device, non_blocking=True)
        video_res_masks = self._resize(any_res_masks, inference_state["video_height"], inference_state["video_width"])
        if self.non_overlap_masks:
            video_res_masks = self._apply_non_overlapping_constraints(video_res_masks)
        return any_res_masks, video_res_masks

    def _consolidate_temp_output_across_obj(self, inference_state, frame_idx, is_cond, run_mem_encoder, consolidate_at_video_res=False):
        batch_size = self._get_obj_num(inference_state)
        storage_key = "cond_frame_outputs" if is_cond else "non_cond_frame_outputs"
        if consolidate_at_video_res:
            assert not run_mem_encoder, "memory encoder cannot run at video resolution"
            H, W, key = inference_state["video_height"], inference_state["video_width"], "pred_masks_video_res"
        else:
            H = W = self.image_size // 4
            key = "pred_masks"
        consolidated_out = {
            "maskmem_features": None, "maskmem_pos_enc": None,
            key: torch.full((batch_size, 1, H, W), NO_OBJ_SCORE, dtype=F32, device=inference_state["storage_device"]),
            "obj_ptr": torch.full((batch_size, self.hidden_dim), NO_OBJ_SCORE, dtype=F32, device=inference_state["device"]),
        }
        empty_mask_ptr = None
        for obj_idx in range(batch_size):
            out = inference_state["temp_output_dict_per_obj"][obj_idx][storage_key].get(frame_idx, None)
            obj_output_dict = inference_state["output_dict_per_obj"][obj_idx]
            if out is None:
                out = obj_output_dict["cond_frame_outputs"].get(frame_idx, None)
            if out is None:
                out = obj_output_dict["non_cond_frame_outputs"].get(frame_idx, None)
            if out is None:
                # placeholder object on this frame: NO_OBJ_SCORE mask; its pointer comes from an empty mask when memory is encoded
                if run_mem_encoder:
                    if empty_mask_ptr is None:
                        empty_mask_ptr = self._get_empty_mask_ptr(inference_state, frame_idx)
                    consolidated_out["obj_ptr"][obj_idx: obj_idx + 1] = empty_mask_ptr
                continue
            obj_mask = out["pred_masks"]
            dst = consolidated_out[key]
            dst[obj_idx: obj_idx + 1] = self._resize(obj_mask.to(inference_state["device"]), H, W).to(dst.device)
            consolidated_out["obj_ptr"][obj_idx: obj_idx + 1] = out["obj_ptr"]
        if run_mem_encoder:
            device = inference_state["device"]
            high_res_masks = self._resize(consolidated_out["pred_masks"].to(device, non_blocking=True), self.image_size, self.image_size)
            if self.non_overlap_masks_for_mem_enc:
                high_res_masks = self._apply_non_overlapping_constraints(high_res_masks)
            maskmem_features, maskmem_pos_enc = self._run_memory_encoder(
                inference_state=inference_state, frame_idx=frame_idx, batch_size=batch_size, high_res_masks=high_res_masks,
                is_mask_from_pts=True)
            consolidated_out["maskmem_features"] = maskmem_features
            consolidated_out["maskmem_pos_enc"] = maskmem_pos_enc
        return consolidated_out

    def _get_empty_mask_ptr(self, inference_state, frame_idx):
        mask_inputs = torch.zeros((1, 1, self.image_size, self.image_size), dtype=F32, device=inference_state["device"])
        _, _, feats, pos, sizes = self._get_image_feature(inference_state, frame_idx, 1)
        current_out = self.track_step(frame_idx=frame_idx, is_init_cond_frame=True, current_vision_feats=feats,
                                      current_vision_pos_embeds=pos, feat_sizes=sizes, point_inputs=None, mask_inputs=mask_inputs,
                                      output_dict={}, num_frames=inference_state["num_frames"], track_in_reverse=False,
                                      run_mem_encoder=False, prev_sam_mask_logits=None)
        return current_out["obj_ptr"]

    # -------------------------------------------------------------------------------------------------------- propagation
    def _propagate_in_video_preflight(self, inference_state):
        inference_state["tracking_has_started"] = True
        batch_size = self._get_obj_num(inference_state)
        temp_output_dict_per_obj = inference_state["temp_output_dict_per_obj"]
        output_dict = inference_state["output_dict"]
        consolidated_frame_inds = inference_state["consolidated_frame_inds"]
        clear_non_cond_mem = self.clear_non_cond_mem_around_input and (self.clear_non_cond_mem_for_multi_obj or batch_size <= 1)
        for is_cond in [False, True]:
            storage_key = "cond_frame_outputs" if is_cond else "non_cond_frame_outputs"
            temp_frame_inds = set()
            for obj_temp_output_dict in temp_output_dict_per_obj.values():
                temp_frame_inds.update(obj_temp_output_dict[storage_key].keys())
            consolidated_frame_inds[storage_key].update(temp_frame_inds)
            for frame_idx in sorted(temp_frame_inds):
                consolidated_out = self._consolidate_temp_output_across_obj(inference_state, frame_idx, is_cond=is_cond,
                                                                            run_mem_encoder=True)
                output_dict[storage_key][frame_idx] = consolidated_out
                self._add_output_per_object(inference_state, frame_idx, consolidated_out, storage_key)
                if clear_non_cond_mem:
                    self._clear_non_cond_mem_around_input(inference_state, frame_idx)
            for obj_temp_output_dict in temp_output_dict_per_obj.values():
                obj_temp_output_dict[storage_key].clear()
        # a frame that became a conditioning frame is no longer a non-conditioning one
        for frame_idx in output_dict["cond_frame_outputs"]:
            output_dict["non_cond_frame_outputs"].pop(frame_idx, None)
        for obj_output_dict in inference_state["output_dict_per_obj"].values():
            for frame_idx in obj_output_dict["cond_frame_outputs"]:
                obj_output_dict["non_cond_frame_outputs"].pop(frame_idx, None)
        for frame_idx in consolidated_frame_inds["cond_frame_outputs"]:
            assert frame_idx in output_dict["cond_frame_outputs"]
            consolidated_frame_inds["non_cond_frame_outputs"].discard(frame_idx)
        all_consolidated = consolidated_frame_inds["cond_frame_outputs"] | consolidated_frame_inds["non_cond_frame_outputs"]
        input_frames_inds = set()
        for per_frame in inference_state["point_inputs_per_obj"].values():
            input_frames_inds.update(per_frame.keys())
        for per_frame in inference_state["mask_inputs_per_obj"].values():
            input_frames_inds.update(per_frame.keys())
        assert all_consolidated == input_frames_inds

    def _propagate_in_video(self, inference_state, start_frame_idx=None, max_frame_num_to_track=None, reverse=False):
        self._propagate_in_video_preflight(inference_state)
        output_dict = inference_state["output_dict"]
        consolidated_frame_inds = inference_state["consolidated_frame_inds"]
        obj_ids = inference_state["obj_ids"]
        num_frames = inference_state["num_frames"]
        batch_size = self._get_obj_num(inference_state)
        if len(output_dict["cond_frame_outputs"]) == 0:
            raise RuntimeError("No points are provided; please add points first")
        clear_non_cond_mem = self.clear_non_cond_mem_around_input and (self.clear_non_cond_mem_for_multi_obj or batch_size <= 1)
        if start_frame_idx is None:
            start_frame_idx = min(output_dict["cond_frame_outputs"])
        if max_frame_num_to_track is None:
            max_frame_num_to_track = num_frames
        if reverse:
            end_frame_idx = max(start_frame_idx - max_frame_num_to_track, 0)
            processing_order = range(start_frame_idx, end_frame_idx - 1, -1) if start_frame_idx > 0 else []
        else:
            end_frame_idx = min(start_frame_idx + max_frame_num_to_track, num_frames - 1)
            processing_order = range(start_frame_idx, end_frame_idx + 1)
        for frame_idx in processing_order:
            if frame_idx in consolidated_frame_inds["cond_frame_outputs"]:
                storage_key = "cond_frame_outputs"
                current_out = output_dict[storage_key][frame_idx]
                pred_masks = current_out["pred_masks"]
                if clear_non_cond_mem:
                    self._clear_non_cond_mem_around_input(inference_state, frame_idx)
            elif frame_idx in consolidated_frame_inds["non_cond_frame_outputs"]:
                storage_key = "non_cond_frame_outputs"
                current_out = output_dict[storage_key][frame_idx]
                pred_masks = current_out["pred_masks"]
            else:
                storage_key = "non_cond_frame_outputs"
                current_out, pred_masks = self._run_single_frame_inference(
                    inference_state=inference_state, output_dict=output_dict, frame_idx=frame_idx, batch_size=batch_size,
                    is_init_cond_frame=False, point_inputs=None, mask_inputs=None, reverse=reverse, run_mem_encoder=True)
                output_dict[storage_key][frame_idx] = current_out
            self._add_output_per_object(inference_state, frame_idx, current_out, storage_key)
            inference_state["frames_already_tracked"][frame_idx] = {"reverse": reverse}
            _, video_res_masks = self._get_orig_video_res_output(inference_state, pred_masks)
            yield frame_idx, obj_ids, video_res_masks

    def _add_output_per_object(self, inference_state, frame_idx, current_out, storage_key):
        maskmem_features = current_out["maskmem_features"]
        assert maskmem_features is None or isinstance(maskmem_features, torch.Tensor)
        maskmem_pos_enc = current_out["maskmem_pos_enc"]
        assert maskmem_pos_enc is None or isinstance(maskmem_pos_enc, list)
        for obj_idx, obj_output_dict in inference_state["output_dict_per_obj"].items():
            sl = slice(obj_idx, obj_idx + 1)
            obj_out = {"maskmem_features": None, "maskmem_pos_enc": None, "pred_masks": current_out["pred_masks"][sl],
                       "obj_ptr": current_out["obj_ptr"][sl]}
            if maskmem_features is not None:
                obj_out["maskmem_features"] = maskmem_features[sl]
            if maskmem_pos_enc is not None:
                obj_out["maskmem_pos_enc"] = [x[sl] for x in maskmem_pos_enc]
            obj_output_dict[storage_key][frame_idx] = obj_out

    def reset_state(self, inference_state):
        self._reset_tracking_results(inference_state)
        for k in ("obj_id_to_idx", "obj_idx_to_id", "obj_ids", "point_inputs_per_obj", "mask_inputs_per_obj", "output_dict_per_obj",
                  "temp_output_dict_per_obj"):
            inference_state[k].clear()

    def _reset_tracking_results(self, inference_state):
        for k in ("point_inputs_per_obj", "mask_inputs_per_obj"):
            for v in inference_state[k].values():
                v.clear()
        for k in ("output_dict_per_obj", "temp_output_dict_per_obj"):
            for v in inference_state[k].values():
                v["cond_frame_outputs"].clear()
                v["non_cond_frame_outputs"].clear()
        for k in ("output_dict", "consolidated_frame_inds"):
            inference_state[k]["cond_frame_outputs"].clear()
            inference_state[k]["non_cond_frame_outputs"].clear()
        inference_state["tracking_has_started"] = False
        inference_state["frames_already_tracked"].clear()

    # ----------------------------------------------------------------------------------------------------- per-frame work
    def _cache_put(self, inference_state, frame_idx, image, backbone_out):
        cache = inference_state["cached_features"]
        cache[frame_idx] = (image, backbone_out)
        limit = self.feature_cache_frames
        if limit is not None:
            while len(cache) > max(1, limit):
                cache.pop(next(iter(cache)))          # oldest first (dicts keep insertion order)

    @torch.no_grad()
    def prefetch_features(self, inference_state, frame_indices=None, batch: int = 8):
        """Encode the listed (default: all) not-yet-cached frames `batch` at a time.  Results are identical to encoding them one by
        one (every kernel is batch-invariant); the trunk just runs far better filled."""
        todo = [t for t in (range(inference_state["num_frames"]) if frame_indices is None else frame_indices)
                if t not in inference_state["cached_features"]]
        dev = inference_state["device"]
        for i in range(0, len(todo), batch):
            ids = todo[i: i + batch]
            imgs = torch.stack([inference_state["images"][t] for t in ids]).to(dev).float()
            bo = self.forward_image(imgs)
            for j, t in enumerate(ids):
                one = {"backbone_fpn": [f[j: j + 1] for f in bo["backbone_fpn"]], "vision_pos_enc": [p[:1] for p in bo["vision_pos_enc"]]}
                self._cache_put(inference_state, t, imgs[j: j + 1], one)

    def _get_image_feature(self, inference_state, frame_idx, batch_size):
        image, backbone_out = inference_state["cached_features"].get(frame_idx, (None, None))
        if backbone_out is None:
            image = inference_state["images"][frame_idx].to(inference_state["device"]).float().unsqueeze(0)
            backbone_out = self.forward_image(image)
            self._cache_put(inference_state, frame_idx, image, backbone_out)
        expanded_image = image.expand(batch_size, -1, -1, -1)
        expanded = {"backbone_fpn": [f.expand(batch_size, -1, -1, -1) for f in backbone_out["backbone_fpn"]],
                    "vision_pos_enc": [p.expand(batch_size, -1, -1, -1) for p in backbone_out["vision_pos_enc"]]}
        return (expanded_image,) + self._prepare_backbone_features(expanded)

    def _run_single_frame_inference(self, inference_state, output_dict, frame_idx, batch_size, is_init_cond_frame, point_inputs,
                                    mask_inputs, reverse, run_mem_encoder, prev_sam_mask_logits=None):
        assert point_inputs is None or mask_inputs is None
        graphed = (self.use_hip_graphs and not is_init_cond_frame and point_inputs is None and mask_inputs is None and run_mem_encoder
                   and prev_sam_mask_logits is None and not self.training and self.num_maskmem > 0
                   and inference_state["storage_device"] == inference_state["device"])
        if graphed:
            current_out = self._graphed_track(inference_state, output_dict, frame_idx, batch_size, reverse)
        else:
            _, _, feats, pos, sizes = self._get_image_feature(inference_state, frame_idx, batch_size)
            current_out = self._eager_track(inference_state, output_dict, frame_idx, is_init_cond_frame, feats, pos, sizes, point_inputs,
                                            mask_inputs, reverse, run_mem_encoder, prev_sam_mask_logits)
        return self._compact(inference_state, current_out)

    def _graphed_track(self, inference_state, output_dict, frame_idx, batch_size, reverse):
        from .graphs import GraphedPropagation, pointer_capacity
        self._get_image_feature(inference_state, frame_idx, batch_size)          # fills the feature cache
        _, one = inference_state["cached_features"][frame_idx]
        one = {"backbone_fpn": one["backbone_fpn"][-self.num_feature_levels:], "vision_pos_enc": one["vision_pos_enc"][-self.num_feature_levels:]}
        cap = pointer_capacity(self, len(output_dict["cond_frame_outputs"]), inference_state["num_frames"])
        props = inference_state.setdefault("graphed_propagation", {})
        prop = props.get((batch_size, cap))
        if prop is None:
            prop = props[(batch_size, cap)] = GraphedPropagation(self, batch_size, inference_state["num_frames"], cap)
        return prop.track(frame_idx, one, output_dict, track_in_reverse=reverse)

    def _eager_track(self, inference_state, output_dict, frame_idx, is_init_cond_frame, feats, pos, sizes, point_inputs, mask_inputs,
                     reverse, run_mem_encoder, prev_sam_mask_logits):
        return self.track_step(frame_idx=frame_idx, is_init_cond_frame=is_init_cond_frame, current_vision_feats=feats,
                               current_vision_pos_embeds=pos, feat_sizes=sizes, point_inputs=point_inputs, mask_inputs=mask_inputs,
                               output_dict=output_dict, num_frames=inference_state["num_frames"], track_in_reverse=reverse,
                               run_mem_encoder=run_mem_encoder, prev_sam_mask_logits=prev_sam_mask_logits)

    def _compact(self, inference_state, current_out):
        storage_device = inference_state["storage_device"]
        maskmem_features = current_out["maskmem_features"]
        if maskmem_features is not None:
            maskmem_features = maskmem_features.to(storage_device, non_blocking=True)
        pred_masks_gpu = current_out["pred_masks"]
        if self.fill_hole_area > 0:
            filled = ops.fill_holes_(pred_masks_gpu.detach().to(F32).contiguous().clone(), self.fill_hole_area)
            if torch.is_grad_enabled() and pred_masks_gpu.requires_grad:
                # torch.where(is_hole, 0.1, mask) of utils/misc.py:247-258: the gradient flows through the pixels that were kept
                pred_masks_gpu = torch.where(filled != pred_masks_gpu.detach(), filled, pred_masks_gpu)
            else:
                pred_masks_gpu = filled
        pred_masks = pred_masks_gpu.to(storage_device, non_blocking=True)
        compact_current_out = {"maskmem_features": maskmem_features, "maskmem_pos_enc": self._get_maskmem_pos_enc(inference_state, current_out),
                               "pred_masks": pred_masks, "obj_ptr": current_out["obj_ptr"]}
        return compact_current_out, pred_masks_gpu

    def _run_memory_encoder(self, inference_state, frame_idx, batch_size, high_res_masks, is_mask_from_pts):
        _, _, feats, _, sizes = self._get_image_feature(inference_state, frame_idx, batch_size)
        maskmem_features, maskmem_pos_enc = self._encode_new_memory(current_vision_feats=feats, feat_sizes=sizes,
                                                                    pred_masks_high_res=high_res_masks, is_mask_from_pts=is_mask_from_pts)
        maskmem_features = maskmem_features.to(inference_state["storage_device"], non_blocking=True)
        return maskmem_features, self._get_maskmem_pos_enc(inference_state, {"maskmem_pos_enc": maskmem_pos_enc})

    def _get_maskmem_pos_enc(self, inference_state, current_out):
        """`maskmem_pos_enc` is the same for every frame and object: one copy per session (1399-1422)."""
        out_pos = current_out["maskmem_pos_enc"]
        if out_pos is None:
            return None
        constants = inference_state["constants"]
        if "maskmem_pos_enc" not in constants:
            assert isinstance(out_pos, list)
            constants["maskmem_pos_enc"] = [x[0:1].clone() for x in out_pos]
        batch_size = out_pos[0].size(0)
        return [x.expand(batch_size, -1, -1, -1) for x in constants["maskmem_pos_enc"]]

    def _clear_non_cond_mem_around_input(self, inference_state, frame_idx):
        r = self.memory_temporal_stride_for_eval
        non_cond = inference_state["output_dict"]["non_cond_frame_outputs"]
        for t in range(frame_idx - r * self.num_maskmem, frame_idx + r * self.num_maskmem + 1):
            non_cond.pop(t, None)
            for obj_output_dict in inference_state["output_dict_per_obj"].values():
                obj_output_dict["non_cond_frame_outputs"].pop(t, None)

    # public entry points: the inference forms run under torch.no_grad() (the reference: torch.inference_mode), the fork's train_*
    # twins are the SAME bodies in the caller's gradient mode (sam2_video_predictor.py:179-248, 425-555, 641-722, 971-1039, 1126-1208)
    val_init_state = torch.no_grad()(_val_init_state)
    add_new_points = torch.no_grad()(_add_new_points)
    add_new_bbox = torch.no_grad()(_add_new_bbox)
    add_new_mask = torch.no_grad()(_add_new_mask)
    propagate_in_video_preflight = torch.no_grad()(_propagate_in_video_preflight)
    propagate_in_video = torch.no_grad()(_propagate_in_video)
    train_init_state = _val_init_state
    train_add_new_points = _add_new_points
    train_add_new_bbox = _add_new_bbox
    train_add_new_mask = _add_new_mask
    train_propagate_in_video_preflight = _propagate_in_video_preflight
    train_propagate_in_video = _propagate_in_video
