"""Float64 restatement of the token-and-duration transducer lattice (TDT; Xu et al., "Efficient Sequence Transduction by
Jointly Predicting Tokens and Durations", ICML 2023).  TEST INFRASTRUCTURE ONLY: nothing in the product package imports
this file, and it has no counterpart in the reference.

Definition.  durations = (e_0 < ... < e_{N-1}) are integers in 0..16, 1 <= N <= 5, at least one positive.  Token moves use
all N durations, blank moves only the positive ones (blank_durations, Ny = N or N - 1 entries).  A joiner row has C + N
columns, the first C token logits (termination_symbol among them), the last N duration logits, normalised independently:

    tok = log_softmax(row[:C]) - sigma   (sigma >= 0, token head only),     dur = log_softmax(row[C:])

    px[b,i,s,t] = tok[symbols[b,s]] + dur[i] at (s,t), the move (s,t) -> (s+1, t+e_i)            [B,N,S,T+1]
                  -inf where t + e_i > t_end, at column t_end and outside the band; the delay penalty
                  (offset - t) * delay_penalty, offset = (t_end - 1) / 2, is added by source frame t
    py[b,j,s,t] = tok[termination_symbol] + dur[index of d_j], the move (s,t) -> (s, t+d_j)       [B,Ny,S+1,T]
                  -inf where t + d_j > t_end and outside the band

    p[s_begin,t_begin] = 0
    p[s,t] = logadd( (+)_i p[s-1,t-e_i] + px[i,s-1,t-e_i],  (+)_j p[s,t-d_j] + py[j,s,t-d_j] ),   ans = p[s_end,t_end]

with a term whose source lies outside the boundary rectangle absent, whatever it carries; no path gives -inf, an inverted
rectangle 0.  The recursion takes the two duration lists separately (token_durations: Dx >= 1 values in 0..16,
blank_durations: Dy >= 1 values in 1..16).  The DP below is a plain torch program, so autograd gives the occupancies
and d loss / d logits; ``enumerate_paths`` sums exp over every path explicitly."""
from typing import Sequence, Tuple

import numpy as np
import torch

from multiblank_restatement import _bounds, _logsumexp0, _roll_by_shifts

_NEG_INF = float("-inf")


def tdt_dp(px: torch.Tensor, py: torch.Tensor, token_durations: Sequence[int], blank_durations: Sequence[int],
           boundary=None) -> torch.Tensor:
    """px [B,Dx,S,T+1], py [B,Dy,S+1,T] (float64, may require grad) -> ans [B].

    Cell by cell, one anti-diagonal k = (s - s_begin) + (t - t_begin) at a time as a vector over the rows: the symbol
    predecessor (s-1, t-e) lies on diagonal k - 1 - e, one row down; the blank predecessor (s, t-d) on diagonal k - d."""
    B, _, S, _ = px.shape
    T = py.shape[3]
    tok = [int(e) for e in token_durations]
    blk = [int(d) for d in blank_durations]
    assert px.shape[1] == len(tok) and py.shape[1] == len(blk)
    out = []
    for b in range(B):
        sb, tb, se, te = _bounds(boundary, b, S, T)
        if se < sb or te < tb:
            out.append(px.new_zeros(()))
            continue
        Sn, Tn = se - sb + 1, te - tb + 1
        neg = lambda *shape: px.new_full(shape, _NEG_INF)
        # X[i][r,t] = px[i, s_begin + r - 1, t_begin + t - e_i] (symbol move i INTO (r,t)); Y[j][r,t] = py[j, row r, t - d_j]
        X = [torch.cat((neg(1, Tn), torch.cat((neg(Sn - 1, min(e, Tn)), px[b, i, sb:se, tb:tb + max(Tn - e, 0)]), dim=1)), dim=0)
             for i, e in enumerate(tok)]
        Y = [torch.cat((neg(Sn, min(d, Tn)), py[b, j, sb:se + 1, tb:tb + max(Tn - d, 0)]), dim=1) for j, d in enumerate(blk)]
        rows = torch.arange(Sn)
        diag = []
        for k in range(Sn + Tn - 1):
            t = k - rows
            valid = (t >= 0) & (t < Tn)
            tc = t.clamp(0, Tn - 1)
            if k == 0:
                diag.append(torch.where(rows == 0, px.new_zeros(Sn), neg(Sn)))
                continue
            terms = []
            for i, e in enumerate(tok):
                if k - 1 - e >= 0:
                    terms.append(torch.cat((neg(1), diag[k - 1 - e][:-1])) + X[i][rows, tc])
            for j, d in enumerate(blk):
                if k - d >= 0:
                    terms.append(diag[k - d] + Y[j][rows, tc])
            diag.append(torch.where(valid, _logsumexp0(torch.stack(terms)), neg(Sn)) if terms else neg(Sn))
        out.append(diag[-1][Sn - 1])
    return torch.stack(out)


def tdt_dp_with_grads(px, py, token_durations, blank_durations, boundary=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """numpy px, py -> (ans, px_grad, py_grad) as float64 numpy: the occupancies by autograd of ans.sum()."""
    x = torch.tensor(np.asarray(px), dtype=torch.float64, requires_grad=True)
    y = torch.tensor(np.asarray(py), dtype=torch.float64, requires_grad=True)
    ans = tdt_dp(x, y, token_durations, blank_durations, boundary)
    if ans.requires_grad:
        ans.sum().backward()
    gx = x.grad.numpy() if x.grad is not None else np.zeros(x.shape)
    gy = y.grad.numpy() if y.grad is not None else np.zeros(y.shape)
    return ans.detach().numpy(), gx, gy


def enumerate_paths(px: np.ndarray, py: np.ndarray, token_durations: Sequence[int], blank_durations: Sequence[int],
                    bounds=None) -> float:
    """One utterance: px [Dx,S,T+1], py [Dy,S+1,T].  log of the sum over every path of exp(sum of its weights), each path
    walked explicitly (exponential; small lattices only)."""
    S = px.shape[1]
    T = py.shape[2]
    sb, tb, se, te = bounds if bounds is not None else (0, 0, S, T)
    totals = []

    def walk(s, t, w):
        if s == se and t == te:
            totals.append(w)           # the end has no outgoing move inside the rectangle
            return
        if s < se:
            for i, e in enumerate(token_durations):
                if t + e <= te:
                    walk(s + 1, t + e, w + float(px[i, s, t]))
        for j, d in enumerate(blank_durations):
            if t + d <= te:
                walk(s, t + d, w + float(py[j, s, t]))

    if se >= sb and te >= tb:
        walk(sb, tb, 0.0)
    else:
        return 0.0
    totals = np.array([w for w in totals if w > _NEG_INF])
    if totals.size == 0:
        return _NEG_INF
    m = totals.max()
    return float(m + np.log(np.exp(totals - m).sum()))


def blank_durations_of(durations: Sequence[int]) -> Tuple[int, ...]:
    return tuple(int(d) for d in durations if int(d) > 0)


def tdt_logprobs(logits: torch.Tensor, symbols, ranges, termination_symbol: int, durations, boundary=None,
                 sigma: float = 0.0, delay_penalty: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """logits [B,T,r,C+N] (float64, may require grad) -> px [B,N,S,T+1], py [B,Ny,S+1,T]."""
    durs = [int(d) for d in durations]
    N = len(durs)
    B, T, r, W = logits.shape
    C = W - N
    sym = torch.tensor(np.array(symbols), dtype=torch.int64)
    rg = torch.tensor(np.array(ranges), dtype=torch.int64)
    S = sym.shape[1]
    t_end = torch.full((B,), T, dtype=torch.int64) if boundary is None else torch.as_tensor(np.asarray(boundary))[:, 3].to(torch.int64)
    tok = torch.log_softmax(logits[..., :C], dim=-1) - sigma
    dur = torch.log_softmax(logits[..., C:], dim=-1)
    neg = lambda *shape: torch.full(shape, _NEG_INF, dtype=logits.dtype)
    sym_ext = torch.cat((sym, torch.full((B, 1), int(termination_symbol), dtype=torch.int64)), dim=1)
    pruned_sym = torch.gather(sym_ext.unsqueeze(1).expand(B, T, S + 1), 2, rg)              # [B,T,r]
    tokx = torch.gather(tok, 3, pruned_sym.unsqueeze(-1)).squeeze(-1)
    toky = tok[..., int(termination_symbol)]
    tt = torch.arange(T + 1).view(1, 1, T + 1)
    te = t_end.view(B, 1, 1)
    to_lattice = lambda v: _roll_by_shifts(torch.cat((v, neg(B, T, S + 1 - r)), dim=2), rg[:, :, 0]).permute(0, 2, 1)   # [B,S+1,T]
    xs, ys = [], []
    for i, e in enumerate(durs):
        x = torch.cat((to_lattice(tokx + dur[..., i])[:, :S], neg(B, S, 1)), dim=2)        # [B,S,T+1]
        x = x.masked_fill((tt + e > te) | (tt == te), _NEG_INF)
        if delay_penalty > 0.0:
            offset = (t_end.to(logits.dtype).view(B, 1, 1) - 1.0) / 2.0
            x = x + (offset - tt.to(logits.dtype)) * delay_penalty
        xs.append(x)
        if e > 0:
            ys.append(to_lattice(toky + dur[..., i]).masked_fill(tt[:, :, :T] + e > te, _NEG_INF))
    return torch.stack(xs, dim=1).contiguous(), torch.stack(ys, dim=1).contiguous()


def tdt_loss(logits: torch.Tensor, symbols, ranges, termination_symbol, durations, boundary=None, sigma=0.0,
             delay_penalty=0.0) -> torch.Tensor:
    """Per-utterance loss [B] = -ans (reduction "none"), differentiable w.r.t. logits."""
    px, py = tdt_logprobs(logits, symbols, ranges, termination_symbol, durations, boundary, sigma, delay_penalty)
    return -tdt_dp(px, py, durations, blank_durations_of(durations), boundary)
