"""Geometry and inputs shared by tests/test_kd.py and tests/test_gpu_kd.py (knowledge distillation on the pruned band).

B=2 T=12 S=5 r=3, the shapes of tests/test_gpu_lowp.py; utterance 1 is ragged (t_end 9, s_end 3) and its band climbs one row
past s_end, so it has invalid nodes both by frame (t >= 9) and by s > s_end."""
import math

import numpy as np

B, T, S, R = 2, 12, 5, 3
BOUNDARY = np.array([[0, 0, S, T], [0, 0, 3, 9]], np.int32)


def band_ranges():
    """A band built by hand: ranges[b,t,0] climbs from 0 to `top` over the utterance's frames, steps <= 1; `top` is
    s_end + 1 - r for utterance 0 and one more for utterance 1, whose last band row then lies past s_end."""
    rg = np.zeros((B, T, R), np.int32)
    for b in range(B):
        top, te = max(int(BOUNDARY[b, 2]) + 1 - R, 0) + b, int(BOUNDARY[b, 3])
        s0 = np.minimum((np.arange(T) * top + te - 2) // max(te - 1, 1), top)
        rg[b] = s0[:, None] + np.arange(R)[None, :]
    assert rg.max() <= S
    return rg


def symbols_for(C, blank_last, seed):
    """(symbols [B,S], blank): one symbol sits in column 3, the last of a lane's 4-vector; none is the blank"""
    rng = np.random.default_rng(seed)
    sym = rng.integers(1, C - 1, (B, S)).astype(np.int32)
    sym[:, 0] = 3
    return sym, (C - 1 if blank_last else 0)


def logits_pair(C, blank_last, collapsed, seed=None):
    """(student, teacher float32 [B,T,r,C], symbols, blank): standard normal x 3.  For the collapsed mode ln C is added to the
    blank and the correct-symbol columns of both tensors, so that each of the three classes carries mass (on plain random
    rows the rest class holds all but ~2/C of it, and float32 loses the loss in 1 - that)."""
    seed = 3000 + C if seed is None else seed
    sym, blank = symbols_for(C, blank_last, seed)
    rng = np.random.default_rng(seed + 1)
    x = (3.0 * rng.standard_normal((B, T, R, C))).astype(np.float32)
    y = (3.0 * rng.standard_normal((B, T, R, C))).astype(np.float32)
    if collapsed:
        rg = band_ranges()
        boost = np.float32(math.log(C))
        for a in (x, y):
            a[..., blank] += boost
            for b in range(B):
                for t in range(T):
                    for k in range(R):
                        if rg[b, t, k] < S:
                            a[b, t, k, sym[b, rg[b, t, k]]] += boost
    return x, y, sym, blank


def kd_loss_torch(x, y, symbols, ranges, blank, boundary, mode, tau):
    """The same loss composed from torch ops (any device, any float dtype of x; differentiable in x): per-utterance loss [B].
    full: log_softmax twice + kl_div; collapsed: gathers and a masked logsumexp."""
    import torch
    import torch.nn.functional as F
    Bn, Tn, r, C = x.shape
    Sn = symbols.shape[1]
    symbols, ranges = symbols.long(), ranges.long()
    if boundary is None:
        boundary = torch.tensor([[0, 0, Sn, Tn]] * Bn, device=x.device)
    bd = boundary.long()
    t = torch.arange(Tn, device=x.device)[None, :, None]
    sb, tb, se, te = (bd[:, i][:, None, None] for i in range(4))
    valid = (t >= tb) & (t < te) & (ranges >= sb) & (ranges <= se)
    # invalid rows may hold anything: they are replaced before the softmax, not multiplied by 0 after it
    xs = torch.where(valid[..., None], x, torch.zeros((), dtype=x.dtype, device=x.device))
    ys = torch.where(valid[..., None], y.to(x.dtype), torch.zeros((), dtype=x.dtype, device=x.device))
    logq = F.log_softmax(xs / tau, dim=-1)
    logp = F.log_softmax(ys / tau, dim=-1)
    if mode == "full":
        node = F.kl_div(logq, logp, reduction="none", log_target=True).sum(-1)
    else:
        sym_at = torch.gather(F.pad(symbols, (0, 1), value=blank), 1, ranges.clamp(0, Sn).reshape(Bn, Tn * r)).reshape(Bn, Tn, r)
        has_sym = (ranges < se) & (sym_at != blank) & valid
        sym_at = torch.where(has_sym, sym_at, torch.full_like(sym_at, blank))
        cols = torch.arange(C, device=x.device)
        rest = (cols != blank) & (cols[None, None, None, :] != sym_at[..., None])
        ninf = torch.full((), float("-inf"), dtype=x.dtype, device=x.device)

        def classes(lp):
            lb = lp[..., blank]
            ls = torch.where(has_sym, torch.gather(lp, 3, sym_at[..., None])[..., 0], ninf)
            lr = torch.logsumexp(torch.where(rest, lp, ninf), dim=-1)
            return torch.stack([lb, ls, lr], -1)
        cq, cp = classes(logq), classes(logp)
        p = cp.exp()
        node = torch.where(p == 0, torch.zeros_like(p), p * (cp - cq)).sum(-1)
    return torch.where(valid, node, torch.zeros_like(node)).sum((1, 2))
