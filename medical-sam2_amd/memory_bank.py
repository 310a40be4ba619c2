"""The self-sorting memory bank of the 2-D path (func_2d/function.py:87-116 draw, 205-243 replacement) on the device.

The reference keeps a Python list of [maskmem_features, maskmem_pos_enc, iou, image_embed] and, per step, stacks and normalises all
embeddings, rebuilds the bank's similarity matrix once per batch element and branches on device scalars (a host sync each).  Here the
bank owns fixed device storage and small device tables; a step is a fixed sequence of launches with no host sync and no allocation
once the bank is full, so it can be captured into a hipGraph together with the model's step.

Storage, by PHYSICAL slot (capacity = bank_size + max_batch - 1, the reference's fill overshoot):
  feats, pos  fp32 [cap, HW, mem_dim]    token-major, what `sample` gathers 256-byte runs from
  embed       fp32 [cap, hidden_dim*HW]  image_embed[b].reshape(-1): (channel, pixel) flat order
Tables: gram fp32 [32, 32] raw dots of the stored features (diagonal = squared norms), iou fp32 [32], order int32 [32] (logical position ->
physical slot).  The live slots are always 0 .. len-1; a replacement re-uses the slot it pops and only `order` shifts.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from . import ops

F32 = torch.float32


def _chw(t: torch.Tensor) -> torch.Tensor:
    """[B, C, H, W] (any strides) -> [B, C, H*W]; a view for NCHW views of token-major maps and for batch-expanded tables."""
    if t.dtype != F32:
        t = t.float()
    return t.reshape(t.shape[0], t.shape[1], -1)


class MemoryBank2D:
    def __init__(self, bank_size: int = 16, max_batch: int = 4, mem_dim: int = 64, hidden_dim: int = 256, feat_hw: Tuple[int, int] = (64, 64),
                 device="cuda"):
        self.bank_size, self.max_batch, self.mem_dim, self.hidden_dim = int(bank_size), int(max_batch), int(mem_dim), int(hidden_dim)
        self.feat_hw = (int(feat_hw[0]), int(feat_hw[1]))
        self.capacity = self.bank_size + self.max_batch - 1
        if not (1 <= self.max_batch <= ops.BANK_MAX_ROWS and 1 <= self.bank_size and self.capacity <= ops.BANK_MAX):
            raise ValueError(f"MemoryBank2D: max_batch <= {ops.BANK_MAX_ROWS} and bank_size + max_batch - 1 <= {ops.BANK_MAX}")
        if self.mem_dim % 4:
            raise ValueError("MemoryBank2D: mem_dim must be a multiple of 4")
        self.device = torch.device(device)
        HW = self.feat_hw[0] * self.feat_hw[1]
        dev, cap, mb = self.device, self.capacity, self.max_batch
        self.feats = torch.zeros(cap, HW, self.mem_dim, dtype=F32, device=dev)
        self.pos = torch.zeros(cap, HW, self.mem_dim, dtype=F32, device=dev)
        self.embed = torch.zeros(cap, self.hidden_dim * HW, dtype=F32, device=dev)
        self.gram = torch.zeros(ops.BANK_MAX, ops.BANK_MAX, dtype=F32, device=dev)
        self.iou = torch.zeros(ops.BANK_MAX, dtype=F32, device=dev)
        self.order = torch.arange(ops.BANK_MAX, dtype=torch.int32, device=dev)
        self._len = 0
        # per-step scratch and results, allocated once (the tensors `sample` returns are re-used by the next call)
        self._ws = ops.bank_dots_workspace(mb, ops.BANK_MAX, dev)
        self._dots = torch.empty(mb * (cap + mb), dtype=F32, device=dev)
        self._xx = torch.empty(mb, dtype=F32, device=dev)
        self._yy = torch.empty(ops.BANK_MAX, dtype=F32, device=dev)
        self.accept = torch.zeros(mb, dtype=torch.int32, device=dev)             # flags of the last update, per candidate
        self.slot_cand = torch.full((ops.BANK_MAX,), -1, dtype=torch.int32, device=dev)
        self.last_iou = torch.zeros(1, dtype=F32, device=dev)                    # the reference's scalar of the last update
        self._out = {}

    def __len__(self) -> int:
        return self._len

    # ---- draw -----------------------------------------------------------------------------------------------------------------------
    def sample(self, curr_feats: torch.Tensor, u: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None):
        """curr_feats [HW, B, C] (the top-level vision features before memory attention).  Returns (memory, memory_pos fp32 [S*HW, B, mem_dim],
        indices int32 [B, S]) with S = B draws per image, or None for an empty bank (the reference's zero-add branch: skip memory
        attention).  u fp32 [B, S] in [0, 1): the uniforms of the inverse-CDF draw (torch.rand on the device when not given)."""
        N = self._len
        if N == 0:
            return None
        HW, B, C = curr_feats.shape
        if HW != self.feat_hw[0] * self.feat_hw[1] or C != self.hidden_dim or B > self.max_batch:
            raise ValueError(f"MemoryBank2D.sample: curr_feats {tuple(curr_feats.shape)} does not fit the bank")
        if curr_feats.dtype != F32:
            curr_feats = curr_feats.float()
        S = B
        if u is None:
            u = torch.rand(B, S, dtype=F32, device=self.device, generator=generator)
        if tuple(u.shape) != (B, S) or u.dtype != F32 or not u.is_contiguous():
            raise ValueError(f"MemoryBank2D.sample: u must be fp32 contiguous [{B}, {S}]")
        # the stored embedding is in (channel, pixel) flat order, the current features are flattened token-major (function.py:102-107);
        # the reference multiplies the two flat vectors as they are, and so does this: both are read as [HW, C] maps of unit inner stride
        x = curr_feats.permute(1, 0, 2)
        y = self.embed[:N].view(N, HW, C)
        dots = self._dots[: B * N].view(B, N)
        ops.bank_dots(x, y, dots=dots, xx=self._xx, yy=self._yy, workspace=self._ws)
        key = (B, S)
        if key not in self._out:
            self._out[key] = (torch.empty(S * HW, B, self.mem_dim, dtype=F32, device=self.device),
                              torch.empty(S * HW, B, self.mem_dim, dtype=F32, device=self.device),
                              torch.empty(B, S, dtype=torch.int32, device=self.device))
        memory, memory_pos, indices = self._out[key]
        ops.bank_sample(dots, self._xx, self._yy, self.order, N, N, u, indices=indices)
        ops.bank_gather(self.feats, self.pos, self.order, indices, N, memory=memory, memory_pos=memory_pos)
        return memory, memory_pos, indices

    # ---- replacement ----------------------------------------------------------------------------------------------------------------
    def update(self, maskmem_features: torch.Tensor, maskmem_pos_enc, iou_predictions: torch.Tensor, image_embed: torch.Tensor) -> None:
        """maskmem_features, maskmem_pos_enc [B, mem_dim, H, W], iou_predictions [B, M], image_embed [B, hidden_dim, H, W] of one step.
        While len < bank_size all B are appended; afterwards each candidate replaces the bank entry most similar to the entry least
        similar to it, if it is less similar than that pair and passes the IoU gate.  The flags land in `self.accept` (device)."""
        if isinstance(maskmem_pos_enc, (list, tuple)):
            maskmem_pos_enc = maskmem_pos_enc[0]
        f, p, e = _chw(maskmem_features), _chw(maskmem_pos_enc), _chw(image_embed)
        B, N = f.shape[0], self._len
        HW = self.feat_hw[0] * self.feat_hw[1]
        if f.shape != (B, self.mem_dim, HW) or p.shape != f.shape or e.shape != (B, self.hidden_dim, HW) or B > self.max_batch:
            raise ValueError("MemoryBank2D.update: tensor shapes do not fit the bank")
        iou_pred = iou_predictions.reshape(B, -1)
        if iou_pred.dtype != F32 or not iou_pred.is_contiguous():
            iou_pred = iou_pred.float().contiguous()
        fill = N < self.bank_size
        dots = self._dots[: B * (N + B)].view(B, N + B)
        if N:
            ops.bank_dots(f, self.feats[:N].permute(0, 2, 1), f, dots=dots, workspace=self._ws)
        else:
            ops.bank_dots(f, f, dots=dots, workspace=self._ws)
        ops.bank_decide(self.gram, self.iou, self.order, N, self.capacity, dots, iou_pred, fill, accept=self.accept[:B], slot_cand=self.slot_cand,
                        iou_out=self.last_iou)
        ops.bank_commit(self.slot_cand, f, p, e, self.feats, self.pos, self.embed)
        if fill:
            self._len = N + B

    # ---- checkpointing --------------------------------------------------------------------------------------------------------------
    _STATE = ("feats", "pos", "embed", "gram", "iou", "order")

    def state_dict(self) -> dict:
        """Copies of the stores and tables by physical slot, and the length."""
        return {**{k: getattr(self, k).clone() for k in self._STATE}, "len": self._len}

    def load_state_dict(self, state: dict) -> None:
        for k in self._STATE:
            getattr(self, k).copy_(state[k])
        self._len = int(state["len"])

    def load_entries(self, entries: List[list]) -> None:
        """Restores a bank from the list `entries()` returns (logical order becomes slot order); the Gram table is recomputed on the device."""
        N = len(entries)
        if N > self.capacity:
            raise ValueError(f"MemoryBank2D.load_entries: {N} entries exceed the capacity {self.capacity}")
        for n, (f, p, iou, e) in enumerate(entries):
            self.feats[n].copy_(f.reshape(self.mem_dim, -1).t())
            self.pos[n].copy_(p.reshape(self.mem_dim, -1).t())
            self.iou[n] = float(iou)
            self.embed[n].copy_(e.reshape(-1))
        self.order.copy_(torch.arange(ops.BANK_MAX, dtype=torch.int32))
        self.gram.zero_()
        y = self.feats[:N].permute(0, 2, 1)
        for r0 in range(0, N, ops.BANK_MAX_ROWS):
            d = ops.bank_dots(y[r0:r0 + ops.BANK_MAX_ROWS], y)
            self.gram[r0:r0 + d.shape[0], :N] = d
        self._len = N

    # ---- inspection -----------------------------------------------------------------------------------------------------------------
    def tables(self) -> dict:
        """Host copies of the tables in LOGICAL order (one sync): order [N], iou [N], gram [N, N]."""
        N = self._len
        order = self.order[:N].cpu().long()
        gram = self.gram.cpu()
        return {"order": order, "iou": self.iou.cpu()[order], "gram": gram[order][:, order]}

    def entries(self) -> List[list]:
        """The bank as the reference's memory_bank_list, in logical order: [feats [1, mem_dim, H, W], pos [1, mem_dim, H, W], iou (0-dim),
        embed [hidden_dim*H*W]] per entry (copies)."""
        H, W = self.feat_hw
        out = []
        for s in self.order[: self._len].cpu().tolist():
            out.append([self.feats[s].view(H, W, self.mem_dim).permute(2, 0, 1).unsqueeze(0).contiguous(),
                        self.pos[s].view(H, W, self.mem_dim).permute(2, 0, 1).unsqueeze(0).contiguous(),
                        self.iou[s].clone(), self.embed[s].clone()])
        return out


def step_2d(model, bank: MemoryBank2D, imgs: torch.Tensor, pts: torch.Tensor, labels: torch.Tensor, u: Optional[torch.Tensor] = None,
            generator: Optional[torch.Generator] = None):
    """The SAM2 sub-sequence of func_2d/function.py:70-243 with the bank live: image encoder, draw + memory attention (skipped while the
    bank is empty), prompt encoder, mask decoder, bilinear x4 high-res mask, memory encoder, bank update.
    Returns (low_res_masks, iou_predictions, maskmem_features, indices or None)."""
    B = imgs.shape[0]
    backbone_out = model.forward_image(imgs)
    _, vision_feats, vision_pos_embeds, feat_sizes = model._prepare_backbone_features(backbone_out)
    drawn = bank.sample(vision_feats[-1], u=u, generator=generator)
    indices = None
    if drawn is not None:
        memory, memory_pos, indices = drawn
        vision_feats[-1] = model.memory_attention(curr=[vision_feats[-1]], curr_pos=[vision_pos_embeds[-1]], memory=memory,
                                                  memory_pos=memory_pos, num_obj_ptr_tokens=0)
    feats = [f.permute(1, 2, 0).view(B, -1, *s) for f, s in zip(vision_feats[::-1], feat_sizes[::-1])][::-1]
    image_embed, high_res_feats = feats[-1], feats[:-1]
    se, de = model.sam_prompt_encoder(points=(pts, labels), boxes=None, masks=None, batch_size=B)
    low_res, iou, _, _ = model.sam_mask_decoder(image_embeddings=image_embed, image_pe=model.sam_prompt_encoder.get_dense_pe(),
                                                sparse_prompt_embeddings=se, dense_prompt_embeddings=de, multimask_output=False,
                                                repeat_image=False, cell_nums=None, high_res_features=high_res_feats)
    size = int(model.image_size)
    high_res = ops.bilinear_upsample(low_res.contiguous(), size, size)
    maskmem_features, maskmem_pos_enc = model._encode_new_memory(current_vision_feats=vision_feats, feat_sizes=feat_sizes,
                                                                 pred_masks_high_res=high_res, is_mask_from_pts=True)
    bank.update(maskmem_features, maskmem_pos_enc, iou, image_embed)
    return low_res, iou, maskmem_features, indices
