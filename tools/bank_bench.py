#!/usr/bin/env python3
"""Times the 2-D memory bank at the workload's shape (N = 16 entries, B = 4 images, 64 x 64 feature maps, 64 / 256 channels):
`MemoryBank2D.sample` + `update` with HIP events, and in the same process a torch-op restatement of the same arithmetic written the way
func_2d/function.py does it (stack + F.normalize + mm for the draw; per candidate a stacked, normalised Gram matrix and a host-side `if`).
Also bank_dots alone at the draw's and the replacement's shapes, with its achieved fraction of HBM time on its algorithmic bytes
((R + Cn) rows of K fp32, each read once) at 8 TB/s.

The step around the bank touches far more than the 256 MiB Infinity Cache, so the headline figures rotate through enough banks that every
call reads its operands from HBM; the cache-resident figures (one bank, back to back) are printed next to them.  One JSON line."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12
N, B, SIDE, MEM, HID = 16, 4, 64, 64, 256


def timed(fn, iters, warmup=5):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e-3


def torch_sample(entries, curr, u):
    """function.py:92-116 with the multinomial replaced by the same inverse-CDF draw"""
    Bc = curr.shape[1]
    mem = torch.stack([e[0].flatten(2).permute(2, 0, 1) for e in entries])
    pos = torch.stack([e[1].flatten(2).permute(2, 0, 1) for e in entries])
    emb = F.normalize(torch.stack([e[3] for e in entries]), p=2, dim=1)
    cur = F.normalize(curr.permute(1, 0, 2).reshape(Bc, -1), p=2, dim=1)
    p = F.softmax(torch.mm(emb, cur.t()).t(), dim=1)
    idx = torch.searchsorted(torch.cumsum(p, 1), u, right=True).clamp_(max=len(entries) - 1)
    m = mem[idx].squeeze(3).permute(1, 2, 0, 3)
    q = pos[idx].squeeze(3).permute(1, 2, 0, 3)
    return m.reshape(-1, m.size(2), m.size(3)), q.reshape(-1, m.size(2), m.size(3)), idx


def torch_update(entries, feats, pos, iou_pred, image_embed):
    """function.py:213-243 (host-side branches on device scalars)"""
    iou = iou_pred.max(dim=1).values.mean()
    for b in range(feats.size(0)):
        flat = F.normalize(torch.stack([e[0].reshape(-1) for e in entries]), p=2, dim=1)
        sim = torch.mm(flat, flat.t())
        sim.fill_diagonal_(float("-inf"))
        key = F.normalize(feats[b].reshape(-1), p=2, dim=0).unsqueeze(1)
        s = torch.mm(flat, key).squeeze()
        i = torch.argmin(s)
        j = torch.argmax(sim[i])
        if s[i] < sim[i][j]:
            if iou > entries[j][2] - 0.1:
                entries.pop(j)
                entries.append([feats[b].unsqueeze(0), pos[b].unsqueeze(0), iou, image_embed[b].reshape(-1)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--banks", type=int, default=5, help="banks rotated through (5 x 114 MiB > the 256 MiB Infinity Cache)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bank_bench needs the MI355X"
    from medical_sam2_amd import ops
    from medical_sam2_amd.memory_bank import MemoryBank2D
    dev = "cuda"
    torch.set_grad_enabled(False)
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev)
    HW = SIDE * SIDE

    def candidates():
        # layouts of the model: features = NCHW view of a token-major map, embedding = view of seq-first [HW, B, C]
        f = rnd(B, SIDE, SIDE, MEM).permute(0, 3, 1, 2)
        p = rnd(1, SIDE, SIDE, MEM).permute(0, 3, 1, 2).expand(B, -1, -1, -1)
        e = rnd(HW, B, HID).permute(1, 2, 0).view(B, HID, SIDE, SIDE)
        return f, p, 0.5 + 0.4 * torch.rand(B, 1, generator=g, device=dev), e
    banks, lists = [], []
    for _ in range(args.banks):
        bank = MemoryBank2D(bank_size=N, max_batch=B, mem_dim=MEM, hidden_dim=HID, feat_hw=(SIDE, SIDE), device=dev)
        for _ in range(N // B):
            bank.update(*candidates())
        banks.append(bank)
        lists.append(bank.entries())
    steps = [(rnd(HW, B, HID), torch.rand(B, B, generator=g, device=dev), candidates()) for _ in range(args.banks)]

    def hip_step(i, nb=args.banks):
        bank, (curr, u, cand) = banks[i % nb], steps[i % nb]
        bank.sample(curr, u=u)
        bank.update(*cand)

    def torch_step(i, nb=args.banks):
        ent, (curr, u, cand) = lists[i % nb], steps[i % nb]
        torch_sample(ent, curr, u)
        torch_update(ent, *[t.contiguous() for t in cand])
    out = {"shape": {"N": N, "B": B, "hw": [SIDE, SIDE], "mem_dim": MEM, "hidden_dim": HID}, "iters": args.iters, "banks_rotated": args.banks}
    out["hip_sample_update_ms"] = timed(hip_step, args.iters) * 1e3
    out["hip_sample_update_resident_ms"] = timed(lambda i: hip_step(i, 1), args.iters) * 1e3
    out["torch_restatement_ms"] = timed(torch_step, max(args.iters // 4, 10)) * 1e3
    out["torch_restatement_resident_ms"] = timed(lambda i: torch_step(i, 1), max(args.iters // 4, 10)) * 1e3

    # bank_dots alone: the draw (4 current maps against 16 stored embeddings, K = 256 * 4096) and the replacement (4 candidates against 16
    # stored feature maps and themselves, K = 64 * 4096)
    ws = ops.bank_dots_workspace(B, 32, dev)
    d = torch.empty(B * 32, device=dev)
    for name, K, rows in (("draw", HID * HW, B + N), ("replacement", MEM * HW, N + B)):
        def dots(i, nb=args.banks):
            bank, (curr, _, cand) = banks[i % nb], steps[i % nb]
            if name == "draw":
                ops.bank_dots(curr.permute(1, 0, 2), bank.embed[:N].view(N, HW, HID), dots=d[: B * N].view(B, N), xx=bank._xx, yy=bank._yy, workspace=ws)
            else:
                f = cand[0].reshape(B, MEM, HW)
                ops.bank_dots(f, bank.feats[:N].permute(0, 2, 1), f, dots=d[: B * (N + B)].view(B, N + B), workspace=ws)
        nbytes = rows * K * 4
        for tag, nb in (("", args.banks), ("_resident", 1)):
            t = timed(lambda i: dots(i, nb), args.iters * 2)
            out[f"bank_dots_{name}{tag}_us"] = t * 1e6
            out[f"bank_dots_{name}{tag}_hbm_fraction"] = nbytes / HBM_PEAK / t
        out[f"bank_dots_{name}_algorithmic_bytes"] = nbytes
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
