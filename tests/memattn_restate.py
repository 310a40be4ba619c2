"""Torch restatement of what gemm_rowln_kernel's "merged" A source computes from a split-KV workspace (the attention ABI's layout:
[splits][rows][D] 16-bit partials, then [splits][rows][2] fp32 (max, sum) pairs, maxima in the log2 domain)."""
import torch


def pack_workspace(part16: torch.Tensor, mx: torch.Tensor, sm: torch.Tensor) -> torch.Tensor:
    """part16 [splits, rows, D] 16-bit, mx / sm [splits, rows] fp32 -> the workspace as bytes"""
    pairs = torch.stack([mx.float(), sm.float()], -1).contiguous()
    return torch.cat([part16.contiguous().view(torch.uint8).flatten(), pairs.view(torch.uint8).flatten()])


def unpack_workspace(ws: torch.Tensor, rows: int, D: int, splits: int, dtype):
    """the two regions of a workspace: partials [splits, rows, D] in `dtype`, pairs [splits, rows, 2] fp32"""
    nb = splits * rows * D * 2
    part = ws[:nb].view(dtype).view(splits, rows, D)
    pairs = ws[nb:nb + splits * rows * 8].view(torch.float32).view(splits, rows, 2)
    return part, pairs


def merged_rows(ws: torch.Tensor, rows: int, D: int, splits: int, dtype) -> torch.Tensor:
    """attn_merge_kernel's rule in fp32, rounded to `dtype` once: M = max over the splits; splits with max = -inf are skipped;
    w = l * exp2(m - M); L += w; acc += w * O; o = acc * (1 / L)"""
    part, pairs = unpack_workspace(ws, rows, D, splits, dtype)
    M = pairs[:, :, 0].max(0).values
    L = torch.zeros(rows)
    acc = torch.zeros(rows, D)
    for s in range(splits):
        m, l = pairs[s, :, 0], pairs[s, :, 1]
        live = m != float("-inf")
        w = torch.where(live, l * torch.exp2(m - M), torch.zeros(()))
        L = L + w
        acc = acc + torch.where(live[:, None], w[:, None] * part[s].float(), torch.zeros(()))
    return (acc * (1.0 / L)[:, None]).to(dtype)
