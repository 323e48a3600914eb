"""Knowledge distillation on the pruned band, restated in numpy float64 straight from its definition (no torch): the loss
per utterance and its gradient with respect to the student logits.

Node (b,t,k) with s = ranges[b,t,k] is valid iff t_begin <= t < t_end and s_begin <= s <= s_end, boundary[b] = (s_begin,
t_begin, s_end, t_end) (None: (0, 0, S, T)); an invalid node adds 0 and has a zero gradient row, and its rows are not read.
  full:      KL(p || q) = sum_c p_c (log p_c - log q_c), p = softmax(teacher row / tau), q = softmax(student row / tau)
  collapsed: the same over the classes {blank}, {symbols[b,s]} (only when s < s_end and it is not the blank), {the rest};
             the rest's mass is a logsumexp over the other columns
Terms with p = 0 are 0.  No tau^2 factor.  The loss of an utterance is the sum over its valid nodes."""
import numpy as np


def _lse(v):
    """logsumexp of a 1-d array; -inf for an empty or all -inf one"""
    if v.size == 0:
        return -np.inf
    m = np.max(v)
    if not np.isfinite(m):
        return m
    return m + np.log(np.sum(np.exp(v - m)))


def _xlogy_terms(logp, logq):
    p = np.exp(logp)
    with np.errstate(invalid="ignore"):
        return np.where(p == 0, 0.0, p * (logp - logq))


def valid_nodes(ranges, boundary, S):
    """bool [B,T,r]"""
    ranges = np.asarray(ranges)
    B, T, r = ranges.shape
    bd = np.tile(np.array([0, 0, S, T]), (B, 1)) if boundary is None else np.asarray(boundary)
    t = np.arange(T)[None, :, None]
    sb, tb, se, te = (bd[:, i][:, None, None] for i in range(4))
    return (t >= tb) & (t < te) & (ranges >= sb) & (ranges <= se)


def kd_loss_and_grad(logits, teacher_logits, symbols, ranges, termination_symbol, boundary=None, mode="full",
                     temperature=1.0):
    """(loss [B], d sum(loss) / d logits [B,T,r,C]) in float64"""
    x = np.asarray(logits, np.float64)
    y = np.asarray(teacher_logits, np.float64)
    symbols, ranges = np.asarray(symbols), np.asarray(ranges)
    B, T, r, C = x.shape
    S = symbols.shape[1]
    assert y.shape == x.shape and ranges.shape == (B, T, r) and mode in ("full", "collapsed") and temperature > 0
    bd = np.tile(np.array([0, 0, S, T]), (B, 1)) if boundary is None else np.asarray(boundary)
    valid = valid_nodes(ranges, boundary, S)
    loss = np.zeros(B)
    grad = np.zeros_like(x)
    blank = int(termination_symbol)
    for b in range(B):
        for t in range(T):
            for k in range(r):
                if not valid[b, t, k]:
                    continue
                a, c = x[b, t, k] / temperature, y[b, t, k] / temperature
                logq, logp = a - _lse(a), c - _lse(c)
                if mode == "full":
                    loss[b] += _xlogy_terms(logp, logq).sum()
                    grad[b, t, k] = (np.exp(logq) - np.exp(logp)) / temperature
                    continue
                s = int(ranges[b, t, k])
                classes = [np.array([blank])]
                if s < bd[b, 2] and int(symbols[b, s]) != blank:
                    classes.append(np.array([int(symbols[b, s])]))
                taken = np.concatenate(classes)
                classes.append(np.setdiff1d(np.arange(C), taken))
                for cols in classes:
                    if cols.size == 0:
                        continue
                    lq, lp = _lse(logq[cols]), _lse(logp[cols])
                    loss[b] += float(_xlogy_terms(np.array(lp), np.array(lq)))
                    # d/d a_c of -P (log Q): -P (1[c in class] exp(logq_c - lq) - q_c); the -q_c parts sum to +q_c
                    if np.isfinite(lq):
                        grad[b, t, k, cols] -= np.exp(lp) * np.exp(logq[cols] - lq)
                grad[b, t, k] += np.exp(logq)
                grad[b, t, k] /= temperature
    return loss, grad
