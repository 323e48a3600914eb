"""Float64 restatement of the multi-blank transducer lattice (big blanks that advance several frames; Xu et al.,
"Multi-blank Transducers for Speech Recognition", ICASSP 2023).  TEST INFRASTRUCTURE ONLY: nothing in the product package
imports this file, and it has no counterpart in the reference.

Definition.  blank 0 is the termination symbol with duration 1; big blank k is the vocabulary entry id_k with duration
d_k, 2 <= d_1 < ... <= 32; durations = (1, d_1, ..., d_K), D = K + 1.  Every joiner row is normalised by the ordinary
softmax over all C columns and sigma >= 0 is subtracted from every log-probability.

    px[b,s,t]   = log P(symbols[b,s]) - sigma at (s,t)           [B,S,T+1]
    py[b,j,s,t] = log P(blank_j) - sigma, the move (s,t)->(s,t+d_j)  [B,D,S+1,T], -inf where t + d_j > t_end
    both -inf outside the band, px also at column t_end; a symbol equal to a big-blank id gets px = -inf

    p[s_begin,t_begin] = 0
    p[s,t] = logadd(p[s-1,t] + px[s-1,t], logadd_j p[s,t-d_j] + py[j,s,t-d_j]),   ans = p[s_end,t_end]

with terms that would start outside the boundary rectangle absent.  The DP below is a plain torch program, so
autograd gives the occupancies and d loss / d logits; ``enumerate_paths`` sums exp over every path explicitly."""
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

_NEG_INF = float("-inf")


def _bounds(boundary, b, S, T):
    if boundary is None:
        return 0, 0, S, T
    return tuple(int(v) for v in boundary[b])


def _logsumexp0(stack: torch.Tensor) -> torch.Tensor:
    """logsumexp over dim 0 whose value AND gradient are right where every entry is -inf (-inf, zero gradient)."""
    m = stack.detach().max(dim=0).values
    m = torch.where(torch.isinf(m) & (m < 0), torch.zeros_like(m), m)
    tot = torch.exp(stack - m).sum(dim=0)
    some = ~(tot == 0)                                   # NaN counts as "some": it propagates
    return torch.where(some, m + torch.log(torch.where(some, tot, torch.ones_like(tot))), torch.full_like(tot, _NEG_INF))


def multiblank_dp(px: torch.Tensor, py: torch.Tensor, durations: Sequence[int], boundary=None) -> torch.Tensor:
    """px [B,S,T+1], py [B,D,S+1,T] (float64, may require grad) -> ans [B].  -inf where no path exists; 0 for an
    inverted rectangle (as mutual_information_recursion).

    The recursion cell by cell, evaluated one anti-diagonal k = (s - s_begin) + (t - t_begin) at a time as a vector over
    the rows: both predecessors of a cell lie on earlier diagonals (k - 1 for the symbol, k - d_j for blank j)."""
    B, S, _ = px.shape
    T = py.shape[3]
    durations = [int(d) for d in durations]
    assert py.shape[1] == len(durations)
    out = []
    for b in range(B):
        sb, tb, se, te = _bounds(boundary, b, S, T)
        if se < sb or te < tb:
            out.append(px.new_zeros(()))
            continue
        Sn, Tn = se - sb + 1, te - tb + 1
        neg = lambda *shape: px.new_full(shape, _NEG_INF)
        # X[r,t] = px[s_begin + r - 1, t_begin + t] (the symbol move INTO row r); Y[j][r,t] = py[j, row r, t - d_j]
        X = torch.cat((neg(1, Tn), px[b, sb:se, tb:te + 1]), dim=0)
        Y = [torch.cat((neg(Sn, min(d, Tn)), py[b, j, sb:se + 1, tb:tb + max(Tn - d, 0)]), dim=1) for j, d in enumerate(durations)]
        rows = torch.arange(Sn)
        diag = []
        for k in range(Sn + Tn - 1):
            t = k - rows
            valid = (t >= 0) & (t < Tn)
            tc = t.clamp(0, Tn - 1)
            if k == 0:
                diag.append(torch.where(rows == 0, px.new_zeros(Sn), neg(Sn)))
                continue
            terms = [torch.cat((neg(1), diag[k - 1][:-1])) + X[rows, tc]]
            for j, d in enumerate(durations):
                if k - d >= 0:
                    terms.append(diag[k - d] + Y[j][rows, tc])
            diag.append(torch.where(valid, _logsumexp0(torch.stack(terms)), neg(Sn)))
        out.append(diag[-1][Sn - 1])
    return torch.stack(out)


def multiblank_dp_with_grads(px, py, durations, boundary=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """numpy float32/float64 px, py -> (ans, px_grad, py_grad) as float64 numpy: the occupancies by autograd of ans.sum()."""
    x = torch.tensor(np.asarray(px), dtype=torch.float64, requires_grad=True)
    y = torch.tensor(np.asarray(py), dtype=torch.float64, requires_grad=True)
    ans = multiblank_dp(x, y, durations, boundary)
    if ans.requires_grad:
        ans.sum().backward()
    gx = x.grad.numpy() if x.grad is not None else np.zeros(x.shape)
    gy = y.grad.numpy() if y.grad is not None else np.zeros(y.shape)
    return ans.detach().numpy(), gx, gy


def enumerate_paths(px: np.ndarray, py: np.ndarray, durations: Sequence[int], bounds=None) -> float:
    """One utterance: px [S,T+1], py [D,S+1,T].  log of the sum over every path of exp(sum of its weights), each path
    walked explicitly (exponential; small lattices only)."""
    S = px.shape[0]
    T = py.shape[2]
    sb, tb, se, te = bounds if bounds is not None else (0, 0, S, T)
    totals = []

    def walk(s, t, w):
        if s == se and t == te:
            totals.append(w)
            return
        if s < se:
            walk(s + 1, t, w + float(px[s, t]))
        for j, d in enumerate(durations):
            if t + d <= te:
                walk(s, t + d, w + float(py[j, s, t]))

    walk(sb, tb, 0.0)
    totals = np.array([w for w in totals if w > _NEG_INF])
    if totals.size == 0:
        return _NEG_INF
    m = totals.max()
    return float(m + np.log(np.exp(totals - m).sum()))


def _roll_by_shifts(src: torch.Tensor, shifts: torch.Tensor) -> torch.Tensor:
    """out[b,t,s] = src[b,t,(s - shifts[b,t]) mod N]."""
    B, T, N = src.shape
    idx = (torch.arange(N).view(1, 1, N) - shifts.view(B, T, 1)) % N
    return torch.gather(src, 2, idx)


def multiblank_logprobs(logits: torch.Tensor, symbols, ranges, termination_symbol: int, big_blanks, boundary=None,
                        sigma: float = 0.0, delay_penalty: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """logits [B,T,r,C] (float64, may require grad) -> px [B,S,T+1], py [B,D,S+1,T]."""
    B, T, r, C = logits.shape
    sym = torch.as_tensor(np.asarray(symbols)).to(torch.int64)
    rg = torch.as_tensor(np.asarray(ranges)).to(torch.int64)
    S = sym.shape[1]
    ids = [int(termination_symbol)] + [int(i) for i, _ in big_blanks]
    durs = [1] + [int(d) for _, d in big_blanks]
    t_end = torch.full((B,), T, dtype=torch.int64) if boundary is None else torch.as_tensor(np.asarray(boundary))[:, 3].to(torch.int64)
    logp = torch.log_softmax(logits, dim=-1) - sigma
    neg = lambda *shape: torch.full(shape, _NEG_INF, dtype=logits.dtype)
    sym_ext = torch.cat((sym, torch.full((B, 1), int(termination_symbol), dtype=torch.int64)), dim=1)
    pruned_sym = torch.gather(sym_ext.unsqueeze(1).expand(B, T, S + 1), 2, rg)              # [B,T,r]
    px = torch.gather(logp, 3, pruned_sym.unsqueeze(-1)).squeeze(-1)
    for i in ids[1:]:
        px = px.masked_fill(pruned_sym == i, _NEG_INF)                                       # a big blank is not a symbol
    px = _roll_by_shifts(torch.cat((px, neg(B, T, S + 1 - r)), dim=2), rg[:, :, 0])[:, :, :S].permute(0, 2, 1)
    px = torch.cat((px, neg(B, S, 1)), dim=2)                                                # [B,S,T+1]
    tt = torch.arange(T + 1).view(1, 1, T + 1)
    px = px.masked_fill(tt == t_end.view(B, 1, 1), _NEG_INF)
    if delay_penalty > 0.0:
        offset = (t_end.to(logits.dtype).view(B, 1, 1) - 1.0) / 2.0
        px = px + (offset - tt.to(logits.dtype)) * delay_penalty
    planes = []
    for i, d in zip(ids, durs):
        y = _roll_by_shifts(torch.cat((logp[..., i], neg(B, T, S + 1 - r)), dim=2), rg[:, :, 0]).permute(0, 2, 1)
        planes.append(y.masked_fill(tt[:, :, :T] + d > t_end.view(B, 1, 1), _NEG_INF))      # may not overshoot t_end
    return px.contiguous(), torch.stack(planes, dim=1).contiguous()


def multiblank_loss(logits: torch.Tensor, symbols, ranges, termination_symbol, big_blanks, boundary=None, sigma=0.0,
                    delay_penalty=0.0) -> torch.Tensor:
    """Per-utterance loss [B] = -ans (reduction "none"), differentiable w.r.t. logits."""
    px, py = multiblank_logprobs(logits, symbols, ranges, termination_symbol, big_blanks, boundary, sigma, delay_penalty)
    durs = [1] + [int(d) for _, d in big_blanks]
    return -multiblank_dp(px, py, durs, boundary)
