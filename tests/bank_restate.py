"""Float64 restatement of the 2-D memory bank (medical_sam2_amd/memory_bank.py), written from the behaviour, plus the seeded fixtures the
CPU and GPU bank tests share.

Draw: cosine of every stored embedding (flat, as stored) with every image's current features (flat, token-major), each norm clamped at
1e-12; softmax over the entries; S draws per image by inverse CDF from given uniforms.  The drawn entries' features and position
encodings are laid out [S*HW, B, C]: sample-major, then pixel, then image.

Replacement: while the bank holds fewer than bank_size entries a step appends all its B candidates.  Otherwise, candidate by candidate:
i = the entry whose features are least similar (cosine) to the candidate's, j = the other entry most similar to entry i; the candidate
replaces entry j (j is popped, the candidate appended at the end) iff cos(i, candidate) < cos(i, j) and iou > iou_j - 0.1, where iou is
the step's scalar mean_b max_m iou_predictions[b, m].  Ties go to the first index.

Everything that DECIDES is float64.  The one stored number the bank computes itself, the step's iou scalar, is data and is formed the way
an fp32 bank forms it: maxima, then a left-to-right fp32 sum, then one fp32 division.

Every function also reports the smallest margin it met: the gap of each `<` / `>` it evaluated, of each argmin / argmax against its
runner-up, and of each u against the nearest CDF edge.  A fixture whose margin is far above fp32 rounding has one right answer.
"""
import math

import torch

F64 = torch.float64
EPS = 1e-12


class Margin:
    def __init__(self):
        self.value = math.inf

    def note(self, gap):
        self.value = min(self.value, abs(float(gap)))


def _first_argmin(vals, skip=None):
    """(index of the first minimum, gap to the runner-up) over a list of floats; `skip` is left out."""
    idx = [n for n in range(len(vals)) if n != skip]
    i = idx[0]
    for n in idx[1:]:
        if vals[n] < vals[i]:
            i = n
    rest = [vals[n] for n in idx if n != i]
    return i, (min(rest) - vals[i] if rest else math.inf)


def _norms(sq):
    return torch.clamp(sq.to(F64).sqrt(), min=EPS)


# ---- draw ---------------------------------------------------------------------------------------------------------------------------------
def draw_cdf(embeds, curr_flat):
    """embeds [N, K] (logical order), curr_flat [B, K] -> float64 (probabilities [B, N], inclusive CDF [B, N])."""
    e, c = embeds.to(F64), curr_flat.to(F64)
    cos = (c @ e.t()) / (_norms((c * c).sum(1))[:, None] * _norms((e * e).sum(1))[None, :])
    p = torch.softmax(cos, dim=1)
    return p, torch.cumsum(p, dim=1)


def midpoint_uniforms(cdf, picks):
    """u [B, S] at the midpoint of the CDF interval of entry picks[b][s]."""
    lo = torch.cat([torch.zeros(cdf.shape[0], 1, dtype=F64), cdf[:, :-1]], dim=1)
    mid = 0.5 * (lo + cdf)
    return torch.gather(mid, 1, torch.as_tensor(picks, dtype=torch.long)).to(torch.float32)


def draw(embeds, curr_flat, u, margin=None):
    """indices [B, S] (long, logical positions): the first n with u < cdf[n]."""
    margin = margin if margin is not None else Margin()
    _, cdf = draw_cdf(embeds, curr_flat)
    B, N = cdf.shape
    uu = u.to(F64)
    out = torch.zeros(uu.shape, dtype=torch.long)
    for b in range(B):
        for s in range(uu.shape[1]):
            idx = N - 1                               # the last edge is 1 and u < 1 always
            for n in range(N - 2, -1, -1):
                margin.note(uu[b, s] - cdf[b, n])
                if uu[b, s] < cdf[b, n]:
                    idx = n
            out[b, s] = idx
    return out, margin


def gather(entries, indices):
    """entries: the logical list [feats [1, C, H, W], pos, iou, embed]; indices [B, S] -> memory, memory_pos [S*HW, B, C]."""
    B, S = indices.shape
    outs = []
    for k in (0, 1):
        maps = torch.stack([e[k][0].flatten(1).t() for e in entries])          # [N, HW, C]
        picked = maps[indices]                                                 # [B, S, HW, C]
        outs.append(picked.permute(1, 2, 0, 3).reshape(-1, B, maps.shape[2]).contiguous())
    return outs[0], outs[1]


# ---- replacement --------------------------------------------------------------------------------------------------------------------------
def step_iou(iou_predictions):
    """The step's scalar as an fp32 bank forms it (see the module docstring); a 0-dim fp32 tensor."""
    m = iou_predictions.to(torch.float32).max(dim=1).values
    s = m[0].clone()
    for b in range(1, m.shape[0]):
        s = s + m[b]
    return s / torch.tensor(float(m.shape[0]), dtype=torch.float32)


def replace_loop(G, ids, ious, n_old, B, iou, margin=None):
    """The per-candidate loop on a full Gram matrix.  G [n_old + B, n_old + B] float64: raw dots of the vectors the bank held before the
    step (rows 0 .. n_old-1, any order) and of the step's candidates (rows n_old ..).  ids: the bank in logical order as rows of G;
    ious: their IoUs (floats), same order.  Both lists are edited in place.  Returns the accept flags."""
    margin = margin if margin is not None else Margin()
    nrm = _norms(torch.diagonal(G))
    cos = lambda a, b: float(G[a, b] / (nrm[a] * nrm[b]))
    flags = []
    for b in range(B):
        c = n_old + b
        if len(ids) < 2:
            flags.append(False)
            continue
        to_cand = [cos(a, c) for a in ids]
        i, gap = _first_argmin(to_cand)
        margin.note(gap)
        to_i = [-cos(ids[i], a) for a in ids]                                   # argmax as the argmin of the negation
        j, gap = _first_argmin(to_i, skip=i)
        margin.note(gap)
        sim_ij = -to_i[j]
        margin.note(sim_ij - to_cand[i])
        ok = to_cand[i] < sim_ij
        if ok:
            margin.note(float(iou) - (ious[j] - 0.1))
            ok = float(iou) > ious[j] - 0.1
        if ok:
            ids.pop(j)
            ious.pop(j)
            ids.append(c)
            ious.append(float(iou))
        flags.append(ok)
    return flags


class BankRestate:
    """The bank as a list of [feats [1, C, H, W], pos [1, C, H, W], iou (0-dim fp32), embed [Ce*H*W]] (fp32 data, float64 decisions)."""

    def __init__(self, bank_size):
        self.bank_size = bank_size
        self.entries = []
        self.margin = Margin()

    def sample(self, curr_feats, u):
        """curr_feats [HW, B, C] -> (memory, memory_pos, indices) or None."""
        if not self.entries:
            return None
        B = curr_feats.shape[1]
        curr_flat = curr_feats.permute(1, 0, 2).reshape(B, -1)                  # token-major flattening of every image
        idx, _ = draw(torch.stack([e[3] for e in self.entries]), curr_flat, u, self.margin)
        mem, pos = gather(self.entries, idx)
        return mem, pos, idx

    def update(self, feats, pos, iou_predictions, image_embed):
        """feats, pos [B, C, H, W], iou_predictions [B, M], image_embed [B, Ce, H, W]; returns the accept flags."""
        B = feats.shape[0]
        iou = step_iou(iou_predictions)
        new = [[feats[b:b + 1].clone().contiguous(), pos[b:b + 1].clone().contiguous(), iou.clone(), image_embed[b].reshape(-1).clone()]
               for b in range(B)]
        if len(self.entries) < self.bank_size:
            self.entries += new
            return [True] * B
        n_old = len(self.entries)
        V = torch.stack([e[0].reshape(-1) for e in self.entries + new]).to(F64)
        ids = list(range(n_old))
        ious = [float(e[2]) for e in self.entries]
        flags = replace_loop(V @ V.t(), ids, ious, n_old, B, iou, self.margin)
        pool = self.entries + new
        self.entries = [pool[a] for a in ids]
        return flags


# ---- seeded fixtures shared by tests/test_memory_bank_cpu.py (validity: margin >= 1e-3) and tests/test_memory_bank_gpu.py -----------------
HW_SIDE, MEM_DIM, HIDDEN = 16, 64, 256


def mixture(gen, n, K, lo=0.15, hi=0.95):
    """n unit-ish vectors t * common + sqrt(1 - t^2) * private: the cosine of two of them is close to t_a t_b."""
    common = torch.randn(K, generator=gen)
    common = common / common.norm()
    t = lo + (hi - lo) * torch.rand(n, generator=gen)
    private = torch.randn(n, K, generator=gen)
    private = private / private.norm(dim=1, keepdim=True)
    scale = 0.5 + torch.rand(n, 1, generator=gen)                              # norms differ: a raw dot is not a cosine
    return (t[:, None] * common[None, :] + (1 - t * t).sqrt()[:, None] * private) * scale


SAMPLE_SEEDS = {(1, 1): 11, (1, 4): 12, (4, 1): 13, (4, 4): 14, (16, 1): 15, (16, 4): 16, (19, 1): 17, (19, 4): 18}


def sample_fixture(N, B):
    """A bank of N entries (as a BankRestate, logical order = insertion order), curr_feats [HW, B, HIDDEN] and u [B, B] at CDF midpoints."""
    gen = torch.Generator().manual_seed(SAMPLE_SEEDS[(N, B)])
    HW, K = HW_SIDE * HW_SIDE, HIDDEN * HW_SIDE * HW_SIDE
    vec = mixture(gen, N + B, K)
    bank = BankRestate(bank_size=N)
    for n in range(N):
        bank.entries.append([torch.randn(1, MEM_DIM, HW_SIDE, HW_SIDE, generator=gen), torch.randn(1, MEM_DIM, HW_SIDE, HW_SIDE, generator=gen),
                             torch.rand((), generator=gen), (vec[n] * 3.0).clone()])
    curr = vec[N:].reshape(B, HW, HIDDEN).permute(1, 0, 2).contiguous()
    # sharpen the distribution a little less than uniform: cosines of the mixture span about [0.02, 0.9]
    _, cdf = draw_cdf(torch.stack([e[3] for e in bank.entries]), curr.permute(1, 0, 2).reshape(B, -1))
    picks = torch.randint(0, N, (B, B), generator=gen)
    return bank, curr, midpoint_uniforms(cdf, picks), picks


# chosen by the validity condition of tests/test_memory_bank_cpu.py (margin >= 1e-3, accepts and rejects both frequent)
UPDATE_SEEDS = {16: 229, 6: 321}
UPDATE_STEPS, UPDATE_B = 12, 4


def update_fixture(bank_size, seed=None):
    """12 steps of (feats, pos [B, MEM_DIM, 16, 16], iou_predictions [B, 1], image_embed [B, HIDDEN, 16, 16]) with controlled cosines."""
    gen = torch.Generator().manual_seed(UPDATE_SEEDS[bank_size] if seed is None else seed)
    n = UPDATE_STEPS * UPDATE_B
    f = mixture(gen, n, MEM_DIM * HW_SIDE * HW_SIDE).reshape(UPDATE_STEPS, UPDATE_B, MEM_DIM, HW_SIDE, HW_SIDE)
    steps = []
    for s in range(UPDATE_STEPS):
        steps.append((f[s].contiguous(), torch.randn(UPDATE_B, MEM_DIM, HW_SIDE, HW_SIDE, generator=gen),
                      0.3 + 0.65 * torch.rand(UPDATE_B, 1, generator=gen), torch.randn(UPDATE_B, HIDDEN, HW_SIDE, HW_SIDE, generator=gen)))
    return steps


def run_updates(bank_size, steps):
    """Drives a BankRestate through the steps; returns (bank, [flags per step])."""
    bank = BankRestate(bank_size)
    return bank, [bank.update(*st) for st in steps]
