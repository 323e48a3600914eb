"""Distillation on the pruned band from a stored top-K teacher, restated in numpy float64 straight from its definition (no
torch): the loss per utterance, its gradient with respect to the student logits, and which nodes are distilled.

The student x [B,T,r,C] lies on `ranges`; the teacher cache lies on the teacher's own band of r_t rows per frame: K raw
logits per row (`values`), their columns (`indices`, clamped into [0,C); I = the set of a row's columns) and optionally
`rest` = logsumexp over c not in I of teacher_row[c] / tau (None = -inf: the renormalised form).  Node (b,t,k) with
s = ranges[b,t,k] is distilled iff it is valid (kd_restatement.valid_nodes), its weight is not 0, and
k' = s - teacher_ranges[b,t,0] lies in [0, r_t); its teacher row is (b,t,k').  For such a node, a = x / tau, v = values / tau:
  L = logaddexp(logsumexp_k v_k, R), p_k = exp(v_k - L), p_R = exp(R - L)
  q_k = softmax(a)[idx_k], log q_R = logsumexp_{c not in I} a_c - logsumexp_c a_c
  loss = w (sum_k xlogy(p_k, p_k / q_k) + xlogy(p_R, p_R / q_R))
  d loss / d x_c = (w / tau) (softmax(a)_c - pt_c), pt_c = p_k at c = idx_k, p_R exp(a_c - logsumexp_{c' not in I} a_c') elsewhere
Terms of teacher mass 0 are 0.  No tau^2 factor.  The loss of an utterance is the sum over its distilled nodes."""
import numpy as np

from kd_restatement import _lse, valid_nodes


def distilled_nodes(ranges, boundary, S, teacher_ranges=None, r_t=None, node_weights=None):
    """(bool [B,T,r], k' [B,T,r]); teacher_ranges None = the student's ranges"""
    ranges = np.asarray(ranges).astype(np.int64)
    tr = ranges if teacher_ranges is None else np.asarray(teacher_ranges).astype(np.int64)
    r_t = tr.shape[2] if r_t is None else r_t
    kp = ranges - tr[:, :, :1]
    on = valid_nodes(ranges, boundary, S) & (kp >= 0) & (kp < r_t)
    if node_weights is not None:
        on &= np.asarray(node_weights) != 0
    return on, kp


def topk_loss_and_grad(logits, values, indices, ranges, S, boundary=None, teacher_ranges=None, teacher_rest=None,
                       temperature=1.0, node_weights=None):
    """(loss [B], d sum(loss) / d logits [B,T,r,C], distilled [B,T,r]) in float64"""
    x = np.asarray(logits, np.float64)
    vals = np.asarray(values, np.float64)
    B, T, r, C = x.shape
    r_t, K = vals.shape[2:]
    idx = np.clip(np.asarray(indices).astype(np.int64), 0, C - 1)
    assert vals.shape == (B, T, r_t, K) == idx.shape and temperature > 0
    assert teacher_ranges is not None or r_t == r
    on, kp = distilled_nodes(ranges, boundary, S, teacher_ranges, r_t, node_weights)
    loss, grad = np.zeros(B), np.zeros_like(x)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for b, t, k in zip(*np.nonzero(on)):
            w = 1.0 if node_weights is None else float(node_weights[b, t, k])
            kt = kp[b, t, k]
            a, v, cols = x[b, t, k] / temperature, vals[b, t, kt] / temperature, idx[b, t, kt]
            R = -np.inf if teacher_rest is None else float(teacher_rest[b, t, kt])
            L = np.logaddexp(_lse(v), R)
            stored = np.zeros(C, bool)
            stored[cols] = True
            Ls, Rs = _lse(a), _lse(a[~stored])
            lp, lq = v - L, a[cols] - Ls
            p = np.exp(lp)
            node = np.where(p == 0, 0.0, p * (lp - lq)).sum()
            pR = np.exp(R - L)
            if pR != 0:
                node += pR * ((R - L) - (Rs - Ls))
            loss[b] += w * node
            pt = np.zeros(C)
            np.add.at(pt, cols, p)
            if pR != 0 and np.isfinite(Rs):
                pt[~stored] = pR * np.exp(a[~stored] - Rs)
            grad[b, t, k] = (w / temperature) * (np.exp(a - Ls) - pt)
    return loss, grad, on
