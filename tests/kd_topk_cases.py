"""Geometry and inputs shared by tests/test_kd_topk.py and tests/test_gpu_kd_topk.py (distillation from a stored top-K
teacher on the teacher's own band).  numpy only.

Student: the geometry and inputs of tests/kd_cases.py -- B=2 T=12 S=5 r=3, its BOUNDARY and band_ranges(), standard normal
x 3 logits.  Teacher band: r_t rows per frame, teacher_ranges[b,t,0] = clip(ranges[b,t,0] + (-1,0,1,2)[t % 4], 0,
max(S + 1 - r_t, 0)), rows consecutive; with r_t = 2 the valid-and-matched nodes are 20 of 36 and 12 of 23 in the two
utterances, with r_t = 4 they are 34 of 36 and 21 of 23 (asserted below, with at least 2 distilled and 2
valid-but-unmatched nodes in every utterance).  r_t = None is a cache on the student's own ranges.  The cache comes from a
dense random teacher (standard normal x 2) through a numpy top-K; where a rest is given its share p_R of the teacher's mass
is at least 1e-3 in every row (asserted), about 0.3 at C=37 K=5 and 0.6 - 0.7 at C=500 K=8."""
import numpy as np

import kd_cases as K
from kd_restatement import _lse, valid_nodes

B, T, S, R, BOUNDARY = K.B, K.T, K.S, K.R, K.BOUNDARY
SHIFTS = (-1, 0, 1, 2)
MATCHED = {2: ((20, 36), (12, 23)), 4: ((34, 36), (21, 23))}   # r_t -> per utterance (valid and matched, valid)


def teacher_ranges(r_t):
    """int32 [B,T,r_t], or None for r_t None"""
    if r_t is None:
        return None
    rg = K.band_ranges()
    s0 = np.clip(rg[:, :, 0] + np.array(SHIFTS)[np.arange(T) % 4][None, :], 0, max(S + 1 - r_t, 0))
    return (s0[:, :, None] + np.arange(r_t)[None, None, :]).astype(np.int32)


def matched(r_t):
    """bool [B,T,r]: valid and inside the teacher's band"""
    rg = K.band_ranges().astype(np.int64)
    tr = teacher_ranges(r_t)
    kp = rg - (rg if tr is None else tr.astype(np.int64))[:, :, :1]
    return valid_nodes(rg, BOUNDARY, S) & (kp >= 0) & (kp < (R if r_t is None else r_t))


def _check_geometry():
    valid = valid_nodes(K.band_ranges(), BOUNDARY, S)
    for r_t, want in MATCHED.items():
        m = matched(r_t)
        for b in range(B):
            got = (int(m[b].sum()), int(valid[b].sum()))
            assert got == want[b], (r_t, b, got)
            assert got[0] >= 2 and got[1] - got[0] >= 2, (r_t, b, got)


_check_geometry()


def student(C):
    """float32 [B,T,r,C], standard normal x 3 (the student of kd_cases.logits_pair)"""
    return K.logits_pair(C, True, False)[0]


def dense_teacher(C, r_t, seed=None):
    """float32 [B,T,r_t,C] (r_t None: on the student's ranges, r rows), standard normal x 2"""
    rng = np.random.default_rng((7000 + C if seed is None else seed) + 10 * (0 if r_t is None else r_t))
    return (2.0 * rng.standard_normal((B, T, R if r_t is None else r_t, C))).astype(np.float32)


def topk_cache(dense, k, tau, with_rest):
    """(values float32 [..., k], indices int32 [..., k], rest float32 [...] | None) of a dense teacher, by numpy: the k largest
    logits of every row (ties: the lower column), rest = logsumexp of the other columns / tau in float64, rounded to float32"""
    y = np.asarray(dense, np.float32)
    idx = np.argsort(-y, axis=-1, kind="stable")[..., :k]
    vals = np.take_along_axis(y, idx, axis=-1)
    rest = None
    if with_rest:
        rest = np.empty(y.shape[:-1], np.float32)
        for pos in np.ndindex(*y.shape[:-1]):
            others = np.delete(y[pos].astype(np.float64), idx[pos]) / tau
            rest[pos] = _lse(others)
            L = np.logaddexp(_lse(vals[pos].astype(np.float64) / tau), float(rest[pos]))
            assert np.exp(float(rest[pos]) - L) >= 1e-3, (pos, k)          # the rest class carries mass
    return vals, idx.astype(np.int32), rest


def dense_from_cache(vals, idx, C):
    """float32 [..., C]: -inf outside the stored columns"""
    out = np.full(vals.shape[:-1] + (C,), -np.inf, np.float32)
    np.put_along_axis(out, idx.astype(np.int64), vals.astype(np.float32), axis=-1)
    return out
