"""Geometry, inputs and the torch composition shared by tests/test_kd_fact.py and tests/test_gpu_kd_fact.py (factored
knowledge distillation on the pruned band, rnnt_kd_loss_pruned_factored).

B=2 T=6 S=4 r=3; utterance 1 is cut short (t_end 4, s_end 2) and its band climbs one row past s_end, so it has invalid nodes
both by frame (t >= 4) and by s > s_end."""
import math

import numpy as np

B, T, S, R = 2, 6, 4, 3
BOUNDARY = np.array([[0, 0, S, T], [0, 0, 2, 4]], np.int32)
FACTS = ("softmax", "hat", "tdt")


def band_ranges():
    """ranges[b,t,0] climbs from 0 to `top` over the utterance's frames in steps <= 1; `top` is s_end + 1 - r for utterance 0
    and one more for utterance 1, whose last band row then lies past s_end (tests/kd_cases.py, these sizes)."""
    rg = np.zeros((B, T, R), np.int32)
    for b in range(B):
        top, te = max(int(BOUNDARY[b, 2]) + 1 - R, 0) + b, int(BOUNDARY[b, 3])
        s0 = np.minimum((np.arange(T) * top + te - 2) // max(te - 1, 1), top)
        rg[b] = s0[:, None] + np.arange(R)[None, :]
    assert rg.max() <= S
    return rg


def symbols_for(C, blank_last, seed):
    """(symbols [B,S], blank) for C token columns: one symbol sits in column 3 (the last of a lane's quad) when there is
    one; none is the blank"""
    rng = np.random.default_rng(seed)
    sym = rng.integers(1, C - 1, (B, S)).astype(np.int32)
    sym[:, 0] = min(3, C - 2)
    return sym, (C - 1 if blank_last else 0)


def logits_pair(W, N, blank_last, collapsed, seed=None):
    """(student, teacher float32 [B,T,r,W], symbols, blank), W = C + N: standard normal x 3.  For the collapsed mode ln C is
    added to the blank and the correct-symbol columns of both tensors, so that each of the three classes carries mass (as
    tests/kd_cases.py does)."""
    C = W - N
    seed = 5000 + 7 * W + N if seed is None else seed
    sym, blank = symbols_for(C, blank_last, seed)
    rng = np.random.default_rng(seed + 1)
    x = (3.0 * rng.standard_normal((B, T, R, W))).astype(np.float32)
    y = (3.0 * rng.standard_normal((B, T, R, W))).astype(np.float32)
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


def node_weights(seed=77, zeros=0.0):
    """float32 [B,T,r] in (0.25, 1.75); a share `zeros` of them exactly 0"""
    rng = np.random.default_rng(seed)
    w = (0.25 + 1.5 * rng.random((B, T, R))).astype(np.float32)
    if zeros:
        w[rng.random((B, T, R)) < zeros] = 0.0
    return w


def kd_fact_loss_torch(x, y, symbols, ranges, blank, boundary, factorization, num_durations, mode, tau, duration_weight=1.0,
                       node_weights=None):
    """The same loss composed from torch ops (any device, any float dtype of x; differentiable in x): per-utterance loss [B].
    Every factorization is turned into ONE normalised log-distribution per row and the KL is taken over that --
      hat   the joint row: log sigmoid(a_Bk) at the blank, log sigmoid(-a_Bk) + log_softmax over c != Bk elsewhere
      tdt   the token head; the duration head's full KL is added with its weight (and, for duration_weight = 1 and the full
            mode, checked by the caller against the KL of the outer-product distribution, joint_tdt_kl_torch below)
    -- so it shares no formula with the restatement beyond the definition of a KL."""
    import torch
    import torch.nn.functional as F
    Bn, Tn, r, W = x.shape
    N = int(num_durations)
    C = W - N
    Sn = symbols.shape[1]
    symbols, ranges = symbols.long(), ranges.long()
    if boundary is None:
        boundary = torch.tensor([[0, 0, Sn, Tn]] * Bn, device=x.device)
    bd = boundary.long()
    t = torch.arange(Tn, device=x.device)[None, :, None]
    sb, tb, se, te = (bd[:, i][:, None, None] for i in range(4))
    valid = (t >= tb) & (t < te) & (ranges >= sb) & (ranges <= se)
    if node_weights is not None:
        valid = valid & (node_weights != 0)
    zero = torch.zeros((), dtype=x.dtype, device=x.device)
    ninf = torch.full((), float("-inf"), dtype=x.dtype, device=x.device)
    # invalid rows may hold anything: they are replaced before the softmax, not multiplied by 0 after it
    xs = torch.where(valid[..., None], x, zero) / tau
    ys = torch.where(valid[..., None], y.to(x.dtype), zero) / tau
    cols = torch.arange(C, device=x.device)

    def row_logprobs(a):
        if factorization != "hat":
            return F.log_softmax(a[..., :C], dim=-1)
        nb = cols != blank
        inner = F.log_softmax(torch.where(nb, a, ninf), dim=-1)
        return torch.where(nb, F.logsigmoid(-a[..., blank])[..., None] + inner, F.logsigmoid(a[..., blank])[..., None])

    logq, logp = row_logprobs(xs), row_logprobs(ys)
    if mode == "full":
        node = F.kl_div(logq, logp, reduction="none", log_target=True).sum(-1)
    else:
        sym_at = torch.gather(F.pad(symbols, (0, 1), value=blank), 1, ranges.clamp(0, Sn).reshape(Bn, Tn * r)).reshape(Bn, Tn, r)
        has_sym = (ranges < se) & (sym_at != blank) & valid
        sym_at = torch.where(has_sym, sym_at, torch.full_like(sym_at, blank))
        rest = (cols != blank) & (cols[None, None, None, :] != sym_at[..., None])

        def classes(lp):
            lb = lp[..., blank]
            ls = torch.where(has_sym, torch.gather(lp, 3, sym_at[..., None])[..., 0], ninf)
            lr = torch.logsumexp(torch.where(rest, lp, ninf), dim=-1)
            return torch.stack([lb, ls, lr], -1)
        cq, cp = classes(logq), classes(logp)
        p = cp.exp()
        node = torch.where(p == 0, torch.zeros_like(p), p * (cp - cq)).sum(-1)
    if N and duration_weight != 0:
        dq, dp = F.log_softmax(xs[..., C:], dim=-1), F.log_softmax(ys[..., C:], dim=-1)
        node = node + duration_weight * F.kl_div(dq, dp, reduction="none", log_target=True).sum(-1)
    if node_weights is not None:
        node = node * torch.where(valid, node_weights.to(node.dtype), torch.zeros_like(node))
    return torch.where(valid, node, torch.zeros_like(node)).sum((1, 2))


def joint_tdt_kl_torch(x, y, N, tau, valid):
    """KL of the joint token x duration distributions p(c, n) = p_tok(c) p_dur(n) over all C * N pairs, per utterance"""
    import torch
    import torch.nn.functional as F
    C = x.shape[-1] - N

    def joint(a):
        a = torch.where(valid[..., None], a, torch.zeros((), dtype=a.dtype)) / tau
        return (F.log_softmax(a[..., :C], -1)[..., :, None] + F.log_softmax(a[..., C:], -1)[..., None, :]).flatten(-2)
    node = F.kl_div(joint(x), joint(y), reduction="none", log_target=True).sum(-1)
    return torch.where(valid, node, torch.zeros_like(node)).sum((1, 2))
