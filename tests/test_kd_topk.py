"""The float64 restatement of the top-K distillation loss (tests/kd_topk_restatement.py), checked without a device: its
gradient against central differences, its renormalised form against the dense restatement (tests/kd_restatement.py) with a
teacher that is -inf outside the stored columns, and its rest form against the dense full KL, which it must not exceed."""
import numpy as np
import pytest

import kd_cases as K
import kd_restatement as R
import kd_topk_cases as TC
import kd_topk_restatement as TR

SHAPES = [(37, 5), (8, 8), (500, 8)]


def _node_problem(C, k, tau, with_rest, seed):
    """one node as a B = T = r = 1 problem: (x [1,1,1,C], values, indices, rest)"""
    rng = np.random.default_rng(seed)
    x = 3.0 * rng.standard_normal((1, 1, 1, C))
    y = (3.0 * rng.standard_normal((1, 1, 1, C))).astype(np.float32)
    with_rest = with_rest and k < C
    vals, idx, rest = TC.topk_cache(y, k, tau, with_rest)
    return x, vals, idx, rest


@pytest.mark.parametrize("with_rest", [True, False])
@pytest.mark.parametrize("tau", [1.0, 2.0])
@pytest.mark.parametrize("C,k", SHAPES)
def test_gradient_against_central_differences(C, k, tau, with_rest):
    """h = 3e-5 in float64.  The third derivative of the loss along one logit is at most ~0.2 / tau^3 (third cumulants of
    Bernoulli variables, 0.1 each for the full and the masked logsumexp), so the truncation error h^2 / 6 |f'''| is below
    4e-11; the loss of one node is below ~50, so the rounding error 2^-52 |f| / h is below 4e-10.  Bound: 1e-9."""
    rg = np.zeros((1, 1, 1), np.int32)
    worst = 0.0
    for seed in (1, 2, 3):
        x, vals, idx, rest = _node_problem(C, k, tau, with_rest, 100 * C + seed)
        f = lambda z: TR.topk_loss_and_grad(z, vals, idx, rg, 0, None, None, rest, tau)[0][0]
        loss, g, on = TR.topk_loss_and_grad(x, vals, idx, rg, 0, None, None, rest, tau)
        assert on.all() and np.isfinite(loss).all() and loss[0] > 0 and abs(loss[0]) < 50
        cols = np.arange(C) if C <= 64 else np.unique(np.concatenate([idx.ravel(), np.random.default_rng(seed).integers(0, C, 40)]))
        h = 3e-5
        for c in cols:
            xp, xm = x.copy(), x.copy()
            xp[0, 0, 0, c] += h
            xm[0, 0, 0, c] -= h
            worst = max(worst, abs((f(xp) - f(xm)) / (2 * h) - g[0, 0, 0, c]))
        assert abs(g.sum()) < 1e-12            # both distributions sum to one
    print(f"C={C} K={k} tau={tau} rest={with_rest}: max |g - fd| = {worst:.3g}")
    assert worst < 1e-9


@pytest.mark.parametrize("tau", [1.0, 2.0])
@pytest.mark.parametrize("C,k", SHAPES + [(8, 1)])
def test_renormalised_form_is_the_dense_loss_on_a_minus_inf_filled_teacher(C, k, tau):
    """teacher_ranges = None, no rest: the loss of kd_restatement.kd_loss_and_grad (full mode) against a teacher that is -inf
    outside the stored columns -- the same sums in another order, so equal to a few ulp of float64."""
    x = TC.student(C)
    vals, idx, _ = TC.topk_cache(TC.dense_teacher(C, None), k, tau, False)
    rg = K.band_ranges()
    loss, g, on = TR.topk_loss_and_grad(x, vals, idx, rg, K.S, K.BOUNDARY, None, None, tau)
    dense = TC.dense_from_cache(vals, idx, C)
    ref, gref = R.kd_loss_and_grad(x, dense, np.zeros((K.B, K.S), np.int32), rg, 0, K.BOUNDARY, "full", tau)
    assert np.array_equal(on, R.valid_nodes(rg, K.BOUNDARY, K.S))
    assert np.abs(loss - ref).max() <= 1e-13 * np.abs(ref).max()
    assert np.abs(g - gref).max() <= 1e-14
    assert (g[~on] == 0).all()


@pytest.mark.parametrize("r_t", [2, 4, None])
@pytest.mark.parametrize("C,k", [(37, 5), (500, 8)])
def test_rest_form_is_a_coarsening_of_the_dense_kl(C, k, r_t):
    """With the rest given, the loss is the KL between the two distributions coarsened to K columns + one class: never more
    than the full KL against the dense teacher on the same nodes, and more than the renormalised form's nothing-outside-I."""
    x = TC.student(C)
    y = TC.dense_teacher(C, r_t)
    vals, idx, rest = TC.topk_cache(y, k, 1.0, True)
    rg, tr = K.band_ranges(), TC.teacher_ranges(r_t)
    loss, g, on = TR.topk_loss_and_grad(x, vals, idx, rg, K.S, K.BOUNDARY, tr, rest, 1.0)
    assert np.array_equal(on, TC.matched(r_t))
    # the dense teacher moved onto the student's nodes
    kp = np.clip(rg.astype(np.int64) - (rg if tr is None else tr)[:, :, :1], 0, y.shape[2] - 1)
    y_on = np.take_along_axis(y, kp[..., None], axis=2)
    full = np.zeros(K.B)
    for b, t, k_ in zip(*np.nonzero(on)):
        a, c = x[b, t, k_].astype(np.float64), y_on[b, t, k_].astype(np.float64)
        logq, logp = a - R._lse(a), c - R._lse(c)
        full[b] += (np.exp(logp) * (logp - logq)).sum()
    assert (loss > 0).all() and (loss <= full * (1 + 1e-6)).all(), (loss, full)   # rest is stored in float32
    assert (g[~on] == 0).all() and np.abs(g[on]).max() > 0
