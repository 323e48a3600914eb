"""Factored knowledge distillation on the pruned band (rnnt_kd_loss_pruned_factored), restated in numpy float64 straight from
its definition (no torch): the loss per utterance and its gradient with respect to the student logits.

A node is valid as in tests/kd_restatement.py, and additionally only if its weight (node_weights[b,t,k], 1 without weights)
is not exactly 0; an invalid node adds 0, has a zero gradient row, and its rows are not read.  With a = student row / tau,
b = teacher row / tau, Bk the blank column and sym the symbol column (symbols[b,s], absent when s >= s_end or it is Bk):
  softmax  the loss of tests/kd_restatement.py
  hat      qb = sigmoid(a_Bk), u = softmax(a) over c != Bk; pb, v from b.
           full:      KL(Bern(pb) || Bern(qb)) + (1 - pb) sum_{c != Bk} v_c (log v_c - log u_c)
           collapsed: KL over the classes {Bk}: pb, {sym}: (1 - pb) v_sym, {rest}: (1 - pb) sum over the rest of v
  tdt      rows of width C + N: KL_tok + duration_weight KL_dur; KL_tok is the softmax loss (either mode) over the first C
           columns, KL_dur the full KL over the last N.  duration_weight == 0: the duration columns are ignored.
The node loss and its gradient row are multiplied by the weight.  Terms of teacher mass 0 are 0.  No tau^2 factor."""
import numpy as np

from kd_restatement import _lse, _xlogy_terms, valid_nodes


def _class_kl(a, c, classes):
    """KL between softmax(c) and softmax(a) collapsed to `classes` (index arrays that partition the vector; empty ones are
    skipped): (loss, d loss / d a)"""
    logq, logp = a - _lse(a), c - _lse(c)
    loss, grad = 0.0, np.exp(logq)
    for cols in classes:
        if cols.size == 0:
            continue
        lq, lp = _lse(logq[cols]), _lse(logp[cols])
        loss += float(_xlogy_terms(np.array(lp), np.array(lq)))
        if np.isfinite(lq):
            grad[cols] -= np.exp(lp) * np.exp(logq[cols] - lq)     # -P (1[c in class] q_c / Q); the -(-q_c) parts are grad's start
    return loss, grad


def _softmax_kl(a, c, mode, blank, sym):
    """the loss of kd_restatement on one row; sym: the symbol column or None"""
    n = a.size
    if mode == "full":      # every column a class of its own, written out
        logq, logp = a - _lse(a), c - _lse(c)
        return float(_xlogy_terms(logp, logq).sum()), np.exp(logq) - np.exp(logp)
    taken = [blank] + ([sym] if sym is not None else [])
    classes = [np.array([i]) for i in taken] + [np.setdiff1d(np.arange(n), np.array(taken))]
    return _class_kl(a, c, classes)


def _log_sigmoid(z):
    return -np.logaddexp(0.0, -z)


def _hat_kl(a, c, mode, blank, sym):
    n = a.size
    nb = np.setdiff1d(np.arange(n), np.array([blank]))
    lqb, lqn, lpb, lpn = _log_sigmoid(a[blank]), _log_sigmoid(-a[blank]), _log_sigmoid(c[blank]), _log_sigmoid(-c[blank])
    pb, pn, qb = np.exp(lpb), np.exp(lpn), np.exp(lqb)
    bern = float(_xlogy_terms(np.array(lpb), np.array(lqb))) + float(_xlogy_terms(np.array(lpn), np.array(lqn)))
    if mode == "full":
        inner, ginner = _softmax_kl(a[nb], c[nb], "full", 0, None)
    else:
        pos = {int(col): i for i, col in enumerate(nb)}
        taken = [pos[sym]] if sym is not None else []
        inner, ginner = _class_kl(a[nb], c[nb], [np.array(taken, int), np.setdiff1d(np.arange(nb.size), np.array(taken, int))])
    grad = np.zeros(n)
    grad[blank] = qb - pb
    grad[nb] = pn * ginner
    with np.errstate(invalid="ignore"):
        rest = 0.0 if (pn == 0 and not np.isnan(inner)) else pn * inner
    return bern + rest, grad


def kd_fact_loss_and_grad(logits, teacher_logits, symbols, ranges, termination_symbol, boundary=None, factorization="softmax",
                          num_durations=0, mode="full", temperature=1.0, duration_weight=1.0, node_weights=None):
    """(loss [B], d sum(loss) / d logits [B,T,r,W]) in float64"""
    x = np.asarray(logits, np.float64)
    y = np.asarray(teacher_logits, np.float64)
    symbols, ranges = np.asarray(symbols), np.asarray(ranges)
    B, T, r, W = x.shape
    S = symbols.shape[1]
    N = int(num_durations)
    C = W - N
    assert y.shape == x.shape and ranges.shape == (B, T, r) and mode in ("full", "collapsed") and temperature > 0
    assert factorization in ("softmax", "hat", "tdt") and (1 <= N <= 5 if factorization == "tdt" else N == 0) and C >= 1
    blank = int(termination_symbol)
    assert 0 <= blank < C
    bd = np.tile(np.array([0, 0, S, T]), (B, 1)) if boundary is None else np.asarray(boundary)
    w = np.ones((B, T, r)) if node_weights is None else np.asarray(node_weights, np.float64)
    valid = valid_nodes(ranges, boundary, S) & (w != 0)
    loss = np.zeros(B)
    grad = np.zeros_like(x)
    for b in range(B):
        for t in range(T):
            for k in range(r):
                if not valid[b, t, k]:
                    continue
                a, c = x[b, t, k] / temperature, y[b, t, k] / temperature
                s = int(ranges[b, t, k])
                sym = None
                if mode == "collapsed" and s < bd[b, 2] and int(symbols[b, s]) != blank:
                    sym = int(symbols[b, s])
                g = np.zeros(W)
                if factorization == "hat":
                    node, g[:] = _hat_kl(a, c, mode, blank, sym)
                else:
                    node, g[:C] = _softmax_kl(a[:C], c[:C], mode, blank, sym)
                    if N and duration_weight != 0:
                        dur, gd = _softmax_kl(a[C:], c[C:], "full", 0, None)
                        node += duration_weight * dur
                        g[C:] = duration_weight * gd
                loss[b] += w[b, t, k] * node
                grad[b, t, k] = w[b, t, k] * g / temperature
    return loss, grad
