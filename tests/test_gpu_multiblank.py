"""Multi-blank transducer on the GPU: the recursion with big blanks (csrc/mi_multiblank.hip), the builder and gradient
twins (the mb_* kernels of csrc/pruned_logprobs.hip) and the losses, every one against the float64 restatement of
tests/multiblank_restatement.py under the project's rule: normwise max|d| / max|ref| <= 1e-4 (TOL_F64 of
tests/test_gpu_config_parity.py).  No utterance is skipped in a parity test; the no-path case has a test of its own.

One deviation from the listed builder cases: s_range = 16 cannot be a band of a lattice with S = 9 (the entry points
require s_range <= S + 1, as the ordinary builder does), so the r = 16 cases run at S = 17; r = 1 and r = 5 run at S = 9."""
import functools

import numpy as np
import pytest
import torch

from helpers import max_rel, synthetic
from multiblank_restatement import multiblank_dp_with_grads, multiblank_logprobs, multiblank_loss
from test_gpu_graph import _capture

pytestmark = pytest.mark.gpu

TOL_F64 = 1e-4
NEG = float("-inf")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _n(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------- recursion alone
SHAPES = [(2, 0, 9), (2, 5, 1), (3, 12, 40), (2, 70, 33), (1, 1100, 6), (2, 50, 200)]
DURATIONS = [(1,), (1, 2, 4, 8), (1, 7, 8, 9), (1, 32), (2, 3)]


def _fit(durations, T):
    """T = 6: the durations of the set that fit."""
    return tuple(d for d in durations if d <= T) if T == 6 else durations


def _lattice(B, S, T, D, seed, with_boundary):
    rng = np.random.default_rng(seed)
    px = rng.standard_normal((B, S, T + 1)).astype(np.float32)
    py = rng.standard_normal((B, D, S + 1, T)).astype(np.float32)
    if S > 4 * T:   # a tall lattice has only T blank moves to dodge -inf symbol cells with: a handful of them, not 2 %
        px.reshape(-1)[rng.integers(0, px.size, 3 if px.size > 100 else 1)] = NEG
        py[rng.random(py.shape) < 0.02] = NEG if T > 1 else 0.0
    else:
        px[rng.random(px.shape) < 0.02] = NEG
        py[rng.random(py.shape) < 0.02] = NEG
    bd = None
    if with_boundary:   # t_begin > 0, t_end < T, s_begin > 0 wherever the lattice has room for them
        bd = np.zeros((B, 4), np.int32)
        for b in range(B):
            bd[b] = [1 if S >= 1 else 0, 1 if T >= 3 else 0, S - (b % 2 if S >= 2 else 0), T - 1 - b % 2 if T >= 3 else T]
    return px, py, bd


@functools.lru_cache(maxsize=None)
def _recursion_case(shape, durations, with_boundary):
    B, S, T = shape
    px, py, bd = _lattice(B, S, T, len(durations), 17 * S + T + len(durations), with_boundary)
    return px, py, bd, multiblank_dp_with_grads(px, py, durations, bd)


@pytest.mark.parametrize("with_boundary", [False, True], ids=["full", "subrect"])
@pytest.mark.parametrize("durations", DURATIONS, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_recursion_matches_restatement(ft, dev, shape, durations, with_boundary):
    durations = _fit(durations, shape[2])
    px, py, bd, (w_ans, w_gx, w_gy) = _recursion_case(shape, durations, with_boundary)
    if 1 in durations:
        assert np.isfinite(w_ans).all(), "the inputs of a parity case must leave every utterance a path"
    bdt = None if bd is None else _t(bd, dev)
    ans, (gx, gy) = ft.mutual_information_recursion_multiblank(_t(px, dev), _t(py, dev), durations, bdt, calc_gradients=True)
    e = (max_rel(_n(ans), w_ans), max_rel(_n(gx), w_gx), max_rel(_n(gy), w_gy))
    print(f"multiblank recursion {shape} {durations} boundary={with_boundary}: ans {e[0]:.3g} px_grad {e[1]:.3g} py_grad {e[2]:.3g}")
    assert max(e) <= TOL_F64, e
    if durations == (1,):
        o_ans, (o_gx, o_gy) = ft.mutual_information_recursion(_t(px, dev), _t(py[:, 0], dev), bdt, calc_gradients=True)
        assert max_rel(_n(ans), _n(o_ans)) <= TOL_F64
        assert max_rel(_n(gx), _n(o_gx)) <= TOL_F64 and max_rel(_n(gy[:, 0]), _n(o_gy)) <= TOL_F64


def test_recursion_autograd_scales_by_upstream(ft, dev):
    px, py, bd, (w_ans, w_gx, w_gy) = _recursion_case((3, 12, 40), (1, 2, 4, 8), True)
    x, y = _t(px, dev).requires_grad_(True), _t(py, dev).requires_grad_(True)
    ans = ft.mutual_information_recursion_multiblank(x, y, (1, 2, 4, 8), _t(bd, dev))
    w = torch.tensor([0.5, -2.0, 3.0], device=dev)
    (ans * w).sum().backward()
    assert max_rel(_n(x.grad), w_gx * _n(w)[:, None, None]) <= TOL_F64
    assert max_rel(_n(y.grad), w_gy * _n(w)[:, None, None, None]) <= TOL_F64


def test_no_path_utterance_is_minus_inf_with_finite_gradients(ft, dev):
    """Utterance 1 has every duration-1 blank at -inf and T = 7 is not a sum of 2s and 4s: ans = -inf, every gradient
    finite (zero); its batch neighbours are what they are without it, bit for bit."""
    B, S, T, durations = 3, 4, 7, (1, 2, 4)
    px, py, _ = _lattice(B, S, T, 3, 5, False)
    py2 = py.copy()
    py2[1, 0] = NEG
    run = lambda y: ft.mutual_information_recursion_multiblank(_t(px, dev), _t(y, dev), durations, None, calc_gradients=True)
    ans0, (gx0, gy0) = run(py)
    ans, (gx, gy) = run(py2)
    assert _n(ans)[1] == NEG
    assert np.isfinite(_n(gx)).all() and np.isfinite(_n(gy)).all()
    assert not _n(gx)[1].any() and not _n(gy)[1].any()
    for b in (0, 2):
        assert _n(ans)[b].tobytes() == _n(ans0)[b].tobytes()
        assert _n(gx)[b].tobytes() == _n(gx0)[b].tobytes() and _n(gy)[b].tobytes() == _n(gy0)[b].tobytes()
    w_ans, w_gx, w_gy = multiblank_dp_with_grads(px, py2, durations, None)
    assert max_rel(_n(ans), w_ans) <= TOL_F64 and max_rel(_n(gx), w_gx) <= TOL_F64 and max_rel(_n(gy), w_gy) <= TOL_F64


def test_nan_stays_in_its_utterance(ft, dev):
    B, S, T, durations = 3, 70, 33, (1, 7, 8, 9)
    px, py, _ = _lattice(B, S, T, 4, 6, False)
    px2 = px.copy()
    px2[1, 3, 2] = np.nan
    run = lambda x: ft.mutual_information_recursion_multiblank(_t(x, dev), _t(py, dev), durations, None, calc_gradients=True)
    ans0, (gx0, gy0) = run(px)
    ans, (gx, gy) = run(px2)
    assert np.isnan(_n(ans)[1])
    for b in (0, 2):
        assert _n(ans)[b].tobytes() == _n(ans0)[b].tobytes()
        assert _n(gx)[b].tobytes() == _n(gx0)[b].tobytes() and _n(gy)[b].tobytes() == _n(gy0)[b].tobytes()


# ------------------------------------------------------------------------------------------------------------ builder
def _band_case(seed, B, T, S, C, r, blank, big_ids):
    """Random logits, symbols that avoid the blanks except one that IS a big blank, monotone band ranges, ragged boundary."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((B, T, r, C)) * 2).astype(np.float32)
    others = np.array([c for c in range(C) if c != blank and c not in big_ids])
    sym = others[rng.integers(0, len(others), (B, S))].astype(np.int32)
    if big_ids:
        sym[0, 2] = big_ids[len(big_ids) // 2]
    sym[1, 0] = blank                          # gathered as in the ordinary builder
    s0 = np.sort(rng.integers(0, S - r + 2, (B, T)), axis=1)
    ranges = (s0[..., None] + np.arange(r)).astype(np.int32)
    bd = np.zeros((B, 4), np.int32)
    bd[:, 2] = S - np.arange(B) % 3
    bd[:, 3] = T - 3 * (np.arange(B) % 3)
    return logits, sym, ranges, bd


@pytest.mark.parametrize("sigma", [0.0, 0.05])
@pytest.mark.parametrize("r", [1, 5, 16])
@pytest.mark.parametrize("C", [5, 500, 501, 2048])
def test_builder_matches_restatement(ft, dev, C, r, sigma):
    """px, py and d logits (random upstream gpx / gpy) against the restatement; big-blank ids in the first, a middle and
    the last column; C = 501 takes the scalar row path; a symbol equal to a big-blank id gets px = -inf; the rows of
    d logits sum to zero for gpx = gpy = 1."""
    B, T, S = 2, 24, (17 if r == 16 else 9)
    blank = 1
    big = ((0, 2), (C // 2, 4), (C - 1, 8))
    logits_np, sym, ranges, bd = _band_case(C + 31 * r, B, T, S, C, r, blank, [i for i, _ in big])
    symt, rgt, bdt = _t(sym, dev), _t(ranges, dev), _t(bd, dev)
    logits = _t(logits_np, dev).requires_grad_(True)
    px, py = ft.get_rnnt_logprobs_multiblank_pruned(logits, symt, rgt, blank, big, bdt, sigma=sigma)
    l64 = torch.from_numpy(logits_np).double().requires_grad_(True)
    px64, py64 = multiblank_logprobs(l64, sym, ranges, blank, big, bd, sigma=sigma)
    assert tuple(px.shape) == (B, S, T + 1) and tuple(py.shape) == (B, 4, S + 1, T)
    ex, ey = max_rel(_n(px), _n(px64)), max_rel(_n(py), _n(py64))      # max_rel also asserts the same -inf pattern
    assert torch.isneginf(px[0, 2]).all()
    g = torch.Generator(device="cpu").manual_seed(C + r)
    wx = torch.rand(px.shape, generator=g, dtype=torch.float64) + 0.5
    wy = torch.rand(py.shape, generator=g, dtype=torch.float64) + 0.5
    (got,) = torch.autograd.grad((px, py), (logits,), (wx.float().to(dev), wy.float().to(dev)), retain_graph=True)
    fx, fy = torch.isfinite(px64), torch.isfinite(py64)
    obj = (torch.where(fx, px64, torch.zeros_like(px64)) * wx).sum() + (torch.where(fy, py64, torch.zeros_like(py64)) * wy).sum()
    (want,) = torch.autograd.grad(obj, (l64,))
    eg = max_rel(_n(got), _n(want))
    print(f"multiblank builder C={C} r={r} sigma={sigma}: px {ex:.3g} py {ey:.3g} dlogits {eg:.3g}")
    assert max(ex, ey, eg) <= TOL_F64, (ex, ey, eg)
    # rows sum to zero: -softmax * (gx + sum gy) + gx + sum gy.  Each of the C float32 terms is off by a few ulp and the
    # float32 lse by ulp(|lse|) (|lse| <= log C + max|x| < 16), so |row sum| <= tot (2 C + 32) 2^-24 with tot <= 1 + D
    (ones,) = torch.autograd.grad((px, py), (logits,), (torch.ones_like(px), torch.ones_like(py)))
    assert _n(ones.sum(-1).abs().max()) <= 5 * (2 * C + 32) * 2.0 ** -24


def test_joint_builder_is_the_pruned_builder_on_identity_ranges(ft, dev):
    B, T, S, C = 2, 9, 4, 12
    rng = np.random.default_rng(2)
    logits = _t(rng.standard_normal((B, T, S + 1, C)).astype(np.float32), dev)
    sym = _t(rng.integers(4, C, (B, S)).astype(np.int32), dev)
    big = ((1, 2), (2, 3))
    px, py = ft.get_rnnt_logprobs_multiblank_joint(logits, sym, 0, big, None, sigma=0.05)
    px64, py64 = multiblank_logprobs(logits.cpu().double(), _n(sym), np.broadcast_to(np.arange(S + 1), (B, T, S + 1)), 0, big,
                                     None, sigma=0.05)
    assert max_rel(_n(px), _n(px64)) <= TOL_F64 and max_rel(_n(py), _n(py64)) <= TOL_F64


# --------------------------------------------------------------------------------------------------------------- loss
LOSS_SHAPES = [(3, 40, 12, 20, 4), (2, 90, 33, 12, 5), (2, 200, 50, 50, 5)]
BIG_BLANKS = ["none", "last", "three"]


def _big(name, C):
    return {"none": (), "last": ((C - 1, 2),), "three": ((1, 2), (2, 4), (3, 8))}[name]


@functools.lru_cache(maxsize=None)
def _loss_inputs(shape):
    """Prune ranges from the ordinary simple loss (get_rnnt_prune_ranges): a duration-1 path always exists."""
    import tf_fast_rnnt as ft
    B, T, S, C, r = shape
    dev = torch.device("cuda:0")
    d = synthetic(900 + T, B, T, S, C, ragged=True)
    blank = 0
    sym = (4 + d["symbols"] % (C - 5)).astype(np.int32)            # in [4, C-2]: no symbol is a blank of any of the sets
    bdt = _t(d["boundary"], dev)
    _, (gx, gy) = ft.rnnt_loss_simple(_t(d["lm"], dev), _t(d["am"], dev), _t(sym, dev), blank, bdt, calc_gradients=True)
    ranges = _n(ft.get_rnnt_prune_ranges(gx, gy, bdt, r))
    logits = (np.random.default_rng(T).standard_normal((B, T, r, C)) * 2).astype(np.float32)
    return logits, sym, ranges, d["boundary"], blank


@functools.lru_cache(maxsize=None)
def _loss_reference(shape, bb, delay_penalty):
    """Per-utterance float64 losses and d (sum of losses) / d logits: every reduction follows from them."""
    logits, sym, ranges, bd, blank = _loss_inputs(shape)
    l64 = torch.from_numpy(logits).double().requires_grad_(True)
    per = multiblank_loss(l64, sym, ranges, blank, _big(bb, shape[3]), bd, 0.05, delay_penalty)
    per.sum().backward()
    return per.detach().numpy(), l64.grad.numpy()


@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
@pytest.mark.parametrize("delay_penalty", [0.0, 0.1])
@pytest.mark.parametrize("bb", BIG_BLANKS)
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=str)
def test_loss_matches_restatement(ft, dev, shape, bb, delay_penalty, reduction):
    B, T, S, C, r = shape
    logits_np, sym, ranges, bd, blank = _loss_inputs(shape)
    per, grad = _loss_reference(shape, bb, delay_penalty)
    assert np.isfinite(per).all()                                  # no utterance drops out
    logits = _t(logits_np, dev).requires_grad_(True)
    loss = ft.rnnt_loss_multiblank_pruned(logits, _t(sym, dev), _t(ranges, dev), blank, _big(bb, C), _t(bd, dev), sigma=0.05,
                                          delay_penalty=delay_penalty, reduction=reduction)
    w = np.array([0.7, 1.3, 0.9])[:B]
    if reduction == "none":
        (loss * _t(w.astype(np.float32), dev)).sum().backward()
        want, want_g = per, grad * w[:, None, None, None]
    else:
        loss.backward()
        want = per.mean() if reduction == "mean" else per.sum()
        want_g = grad / B if reduction == "mean" else grad
    el, eg = max_rel(_n(loss), want), max_rel(_n(logits.grad), want_g)
    print(f"multiblank loss {shape} {bb} dp={delay_penalty} {reduction}: loss {el:.3g} dlogits {eg:.3g}")
    assert el <= TOL_F64 and eg <= TOL_F64, (el, eg)


@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=str)
def test_loss_without_big_blanks_is_the_ordinary_pruned_loss(ft, dev, shape, monkeypatch):
    monkeypatch.setenv("FTR_PRUNED_ROUTE", "lattice")
    B, T, S, C, r = shape
    logits_np, sym, ranges, bd, blank = _loss_inputs(shape)
    out = []
    for f in (lambda x: ft.rnnt_loss_multiblank_pruned(x, _t(sym, dev), _t(ranges, dev), blank, (), _t(bd, dev), reduction="sum"),
              lambda x: ft.rnnt_loss_pruned(x, _t(sym, dev), _t(ranges, dev), blank, _t(bd, dev), reduction="sum")):
        x = _t(logits_np, dev).requires_grad_(True)
        loss = f(x)
        loss.backward()
        out.append((_n(loss), _n(x.grad)))
    assert max_rel(out[0][0], out[1][0]) <= TOL_F64 and max_rel(out[0][1], out[1][1]) <= TOL_F64


def test_unpruned_loss_is_the_pruned_loss_on_identity_ranges(ft, dev):
    B, T, S1, C = 2, 20, 7, 12
    rng = np.random.default_rng(8)
    joint = rng.standard_normal((B, T, S1, C)).astype(np.float32)
    sym = _t(rng.integers(4, C, (B, S1 - 1)).astype(np.int32), dev)
    bd = _t(np.array([[0, 0, S1 - 1, T], [0, 0, S1 - 2, T - 3]], np.int32), dev)
    big = ((1, 2), (2, 4))
    ident = torch.arange(S1, dtype=torch.int32, device=dev).expand(B, T, S1).contiguous()
    out = []
    for f in (lambda x: ft.rnnt_loss_multiblank(x, sym, 0, big, bd, sigma=0.05, delay_penalty=0.1),
              lambda x: ft.rnnt_loss_multiblank_pruned(x, sym, ident, 0, big, bd, sigma=0.05, delay_penalty=0.1)):
        x = _t(joint, dev).requires_grad_(True)
        loss = f(x)
        loss.backward()
        out.append((_n(loss), _n(x.grad)))
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()


def test_only_the_regular_type_exists(ft, dev):
    B, T, S1, C = 1, 4, 3, 6
    joint = torch.zeros(B, T, S1, C, device=dev)
    sym = torch.full((B, S1 - 1), 3, dtype=torch.int32, device=dev)
    ident = torch.arange(S1, dtype=torch.int32, device=dev).expand(B, T, S1).contiguous()
    for rt in ("modified", "constrained", "nonsense"):
        with pytest.raises(ValueError):
            ft.rnnt_loss_multiblank(joint, sym, 0, ((1, 2),), rnnt_type=rt)
        with pytest.raises(ValueError):
            ft.rnnt_loss_multiblank_pruned(joint, sym, ident, 0, ((1, 2),), rnnt_type=rt)
    for bad in (((0, 2),), ((1, 2), (1, 3)), ((6, 2),), ((1, 1),), ((1, 3), (2, 2)), ((1, 33),)):
        with pytest.raises(ValueError):
            ft.rnnt_loss_multiblank(joint, sym, 0, bad)
    with pytest.raises(ValueError):
        ft.rnnt_loss_multiblank(joint, sym, 0, ((1, 2),), sigma=-0.1)


# ------------------------------------------------------------------------------------------- determinism and capture
def _step_fn(ft, dev, shape, bb):
    B, T, S, C, r = shape
    logits_np, sym, ranges, bd, blank = _loss_inputs(shape)
    buf = _t(logits_np, dev)
    symt, rgt, bdt = _t(sym, dev), _t(ranges, dev), _t(bd, dev)

    def step():
        x = buf.clone().requires_grad_(True)          # the leaf is created inside the step
        loss = ft.rnnt_loss_multiblank_pruned(x, symt, rgt, blank, _big(bb, C), bdt, sigma=0.05, delay_penalty=0.1,
                                              reduction="none")
        (g,) = torch.autograd.grad(loss.sum(), (x,))
        return loss.detach(), g.detach()              # only detached results leave it
    return buf, step


def test_forward_and_backward_are_bit_reproducible(ft, dev):
    _, step = _step_fn(ft, dev, LOSS_SHAPES[1], "three")
    step()
    a = [_n(v).copy() for v in step()]
    b = [_n(v).copy() for v in step()]
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()


def test_step_replays_from_a_graph_with_new_values(ft, dev):
    buf, step = _step_fn(ft, dev, LOSS_SHAPES[0], "three")
    g, out = _capture(step)
    for seed in (21, 22):
        buf.copy_(torch.randn(buf.shape, generator=torch.Generator().manual_seed(seed)).to(dev) * 2)
        g.replay()
        torch.cuda.synchronize()
        got = [_n(v).copy() for v in out]
        ref = [_n(v).copy() for v in step()]
        for u, v in zip(got, ref):
            assert u.tobytes() == v.tobytes()
