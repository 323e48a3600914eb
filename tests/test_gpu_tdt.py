"""TDT (token-and-duration transducer) on the GPU: the recursion whose symbol moves also skip frames (csrc/mi_tdt.hip), the
two-headed builder and its gradient twin (csrc/tdt_logprobs.hip) and the losses, every one against the float64 restatement
of tests/tdt_restatement.py under the project's rule: normwise max|d| / max|ref| <= 1e-4 (TOL_F64 of
tests/test_gpu_config_parity.py), with the same -inf pattern (helpers.max_rel asserts it).  No utterance is skipped in a
parity test; the no-path case has a test of its own.

As in tests/test_gpu_multiblank.py, s_range = 16 cannot be a band of a lattice with S = 9 (the entry points require
s_range <= S + 1), so the r = 16 builder cases run at S = 17; r = 1 and r = 5 run at S = 9."""
import functools

import numpy as np
import pytest
import torch

from helpers import max_rel, synthetic
from tdt_restatement import blank_durations_of, tdt_dp_with_grads, tdt_logprobs, tdt_loss
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
MOVES = [((0,), (1,)), ((0,), (1, 2, 4, 8)), ((0, 1, 2, 3, 4), (1, 2, 3, 4)), ((1, 2), (1,)), ((0, 16), (3, 16)),
         ((0, 5, 6, 7), (1, 9))]


def _fit(moves, T):
    """T = 6: the durations of each list that fit."""
    if T != 6:
        return moves
    return tuple(tuple(d for d in m if d <= T) for m in moves)


def _lattice(B, S, T, Dx, Dy, seed, with_boundary):
    rng = np.random.default_rng(seed)
    px = rng.standard_normal((B, Dx, S, T + 1)).astype(np.float32)
    py = rng.standard_normal((B, Dy, S + 1, T)).astype(np.float32)
    if S > 4 * T:   # a tall lattice has only T frames to dodge -inf symbol cells with: a handful of them, not 2 %
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
def _recursion_case(shape, moves, with_boundary):
    B, S, T = shape
    tok, blk = moves
    px, py, bd = _lattice(B, S, T, len(tok), len(blk), 17 * S + T + len(tok) + 3 * len(blk), with_boundary)
    return px, py, bd, tdt_dp_with_grads(px, py, tok, blk, bd)


@pytest.mark.parametrize("with_boundary", [False, True], ids=["full", "subrect"])
@pytest.mark.parametrize("moves", MOVES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_recursion_matches_restatement(ft, dev, shape, moves, with_boundary):
    moves = _fit(moves, shape[2])
    tok, blk = moves
    px, py, bd, (w_ans, w_gx, w_gy) = _recursion_case(shape, moves, with_boundary)
    if 0 in tok and 1 in blk:
        assert np.isfinite(w_ans).all(), "the inputs of a parity case must leave every utterance a path"
    bdt = None if bd is None else _t(bd, dev)
    ans, (gx, gy) = ft.mutual_information_recursion_tdt(_t(px, dev), _t(py, dev), tok, blk, bdt, calc_gradients=True)
    assert tuple(gx.shape) == px.shape and tuple(gy.shape) == py.shape
    e = (max_rel(_n(ans), w_ans), max_rel(_n(gx), w_gx), max_rel(_n(gy), w_gy))
    print(f"tdt recursion {shape} {tok}/{blk} boundary={with_boundary}: ans {e[0]:.3g} px_grad {e[1]:.3g} py_grad {e[2]:.3g}")
    assert max(e) <= TOL_F64, e
    if tok == (0,):     # the multi-blank recursion, and with blank durations (1,) the ordinary one, on the GPU
        m_ans, (m_gx, m_gy) = ft.mutual_information_recursion_multiblank(_t(px[:, 0], dev), _t(py, dev), blk, bdt, calc_gradients=True)
        assert max_rel(_n(ans), _n(m_ans)) <= TOL_F64
        assert max_rel(_n(gx[:, 0]), _n(m_gx)) <= TOL_F64 and max_rel(_n(gy), _n(m_gy)) <= TOL_F64
    if tok == (0,) and blk == (1,):
        o_ans, (o_gx, o_gy) = ft.mutual_information_recursion(_t(px[:, 0], dev), _t(py[:, 0], dev), bdt, calc_gradients=True)
        assert max_rel(_n(ans), _n(o_ans)) <= TOL_F64
        assert max_rel(_n(gx[:, 0]), _n(o_gx)) <= TOL_F64 and max_rel(_n(gy[:, 0]), _n(o_gy)) <= TOL_F64


def test_recursion_autograd_scales_by_upstream(ft, dev):
    moves = ((0, 1, 2, 3, 4), (1, 2, 3, 4))
    px, py, bd, (w_ans, w_gx, w_gy) = _recursion_case((3, 12, 40), moves, True)
    x, y = _t(px, dev).requires_grad_(True), _t(py, dev).requires_grad_(True)
    ans = ft.mutual_information_recursion_tdt(x, y, *moves, _t(bd, dev))
    w = torch.tensor([0.5, -2.0, 3.0], device=dev)
    (ans * w).sum().backward()
    assert max_rel(_n(x.grad), w_gx * _n(w)[:, None, None, None]) <= TOL_F64
    assert max_rel(_n(y.grad), w_gy * _n(w)[:, None, None, None]) <= TOL_F64


def test_no_path_utterance_is_minus_inf_with_finite_gradients(ft, dev):
    """Utterance 1 has every token move of duration 0 and 1 at -inf: its S = 4 symbols would have to advance 3 frames each
    and T = 7 has no room.  ans = -inf, every gradient finite (zero); its batch neighbours are what they are without it,
    bit for bit."""
    B, S, T, tok, blk = 3, 4, 7, (0, 1, 3), (1, 2)
    px, py, _ = _lattice(B, S, T, 3, 2, 5, False)
    px2 = px.copy()
    px2[1, :2] = NEG
    run = lambda x: ft.mutual_information_recursion_tdt(_t(x, dev), _t(py, dev), tok, blk, None, calc_gradients=True)
    ans0, (gx0, gy0) = run(px)
    ans, (gx, gy) = run(px2)
    assert _n(ans)[1] == NEG
    assert np.isfinite(_n(gx)).all() and np.isfinite(_n(gy)).all()
    assert not _n(gx)[1].any() and not _n(gy)[1].any()
    for b in (0, 2):
        assert _n(ans)[b].tobytes() == _n(ans0)[b].tobytes()
        assert _n(gx)[b].tobytes() == _n(gx0)[b].tobytes() and _n(gy)[b].tobytes() == _n(gy0)[b].tobytes()
    w_ans, w_gx, w_gy = tdt_dp_with_grads(px2, py, tok, blk, None)
    assert max_rel(_n(ans), w_ans) <= TOL_F64 and max_rel(_n(gx), w_gx) <= TOL_F64 and max_rel(_n(gy), w_gy) <= TOL_F64


def test_nan_stays_in_its_utterance(ft, dev):
    B, S, T, tok, blk = 3, 70, 33, (0, 5, 6, 7), (1, 9)
    px, py, _ = _lattice(B, S, T, 4, 2, 6, False)
    px2 = px.copy()
    px2[1, 0, 3, 2] = np.nan
    run = lambda x: ft.mutual_information_recursion_tdt(_t(x, dev), _t(py, dev), tok, blk, None, calc_gradients=True)
    ans0, (gx0, gy0) = run(px)
    ans, (gx, gy) = run(px2)
    assert np.isnan(_n(ans)[1])
    for b in (0, 2):
        assert _n(ans)[b].tobytes() == _n(ans0)[b].tobytes()
        assert _n(gx)[b].tobytes() == _n(gx0)[b].tobytes() and _n(gy)[b].tobytes() == _n(gy0)[b].tobytes()


# ------------------------------------------------------------------------------------------------------------ builder
DURATIONS_OF_N = {3: (1, 2, 4), 5: (0, 1, 2, 3, 4)}     # without a zero (Ny = N) and with one (Ny = N - 1)


def _band_case(seed, B, T, S, C, N, r, blank):
    """Random logits [B,T,r,C+N], one symbol that IS the blank, monotone band ranges, ragged boundary."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((B, T, r, C + N)) * 2).astype(np.float32)
    sym = rng.integers(0, C, (B, S)).astype(np.int32)
    sym[1, 0] = blank                          # gathered as in the ordinary builder
    s0 = np.sort(rng.integers(0, S - r + 2, (B, T)), axis=1)
    ranges = (s0[..., None] + np.arange(r)).astype(np.int32)
    bd = np.zeros((B, 4), np.int32)
    bd[:, 2] = S - np.arange(B) % 3
    bd[:, 3] = T - 3 * (np.arange(B) % 3)
    return logits, sym, ranges, bd


@pytest.mark.parametrize("sigma", [0.0, 0.05])
@pytest.mark.parametrize("r", [1, 5, 16])
@pytest.mark.parametrize("CN", [(5, 3), (500, 5), (507, 5), (2043, 5)], ids=str)
def test_builder_matches_restatement(ft, dev, CN, r, sigma):
    """px, py and d logits (random upstream gpx / gpy) against the restatement; C + N = 8, 512 and 2048 take the 16-byte
    row path (with C itself no multiple of 4 in two of them), 505 the scalar one; with all-ones upstream the token columns
    and the duration columns of d logits each sum to zero."""
    C, N = CN
    durs = DURATIONS_OF_N[N]
    Ny = len(blank_durations_of(durs))
    B, T, S = 2, 24, (17 if r == 16 else 9)
    blank = 1
    logits_np, sym, ranges, bd = _band_case(C + 31 * r, B, T, S, C, N, r, blank)
    symt, rgt, bdt = _t(sym, dev), _t(ranges, dev), _t(bd, dev)
    logits = _t(logits_np, dev).requires_grad_(True)
    px, py = ft.get_rnnt_logprobs_tdt_pruned(logits, symt, rgt, blank, durs, bdt, sigma=sigma, delay_penalty=0.1)
    l64 = torch.from_numpy(logits_np).double().requires_grad_(True)
    px64, py64 = tdt_logprobs(l64, sym, ranges, blank, durs, bd, sigma=sigma, delay_penalty=0.1)
    assert tuple(px.shape) == (B, N, S, T + 1) and tuple(py.shape) == (B, Ny, S + 1, T)
    ex, ey = max_rel(_n(px), _n(px64)), max_rel(_n(py), _n(py64))      # max_rel also asserts the same -inf pattern
    g = torch.Generator(device="cpu").manual_seed(C + r)
    wx = torch.rand(px.shape, generator=g, dtype=torch.float64) + 0.5
    wy = torch.rand(py.shape, generator=g, dtype=torch.float64) + 0.5
    (got,) = torch.autograd.grad((px, py), (logits,), (wx.float().to(dev), wy.float().to(dev)), retain_graph=True)
    fx, fy = torch.isfinite(px64), torch.isfinite(py64)
    obj = (torch.where(fx, px64, torch.zeros_like(px64)) * wx).sum() + (torch.where(fy, py64, torch.zeros_like(py64)) * wy).sum()
    (want,) = torch.autograd.grad(obj, (l64,))
    eg = max_rel(_n(got), _n(want))
    print(f"tdt builder C={C} N={N} r={r} sigma={sigma}: px {ex:.3g} py {ey:.3g} dlogits {eg:.3g}")
    assert max(ex, ey, eg) <= TOL_F64, (ex, ey, eg)
    # Each head sums to zero: -softmax * (GX + GY) + GX + GY with GX + GY = tot <= N + Ny for all-ones upstream.  Over a
    # head of K columns: every float32 term tot * exp(x - lse) is off by a few ulp of itself plus ulp(|x - lse|) <= 16 ulp
    # from the rounded argument (together < 20 tot 2^-24 over the head, the softmax summing to 1), the float32 lse by
    # ulp(|lse|) (|lse| <= log K + max|x| < 16: another 16 tot 2^-24), and the float32 sum over the K columns by
    # <= K tot 2^-24: |sum| <= tot (K + 36) 2^-24 < tot (2 K + 32) 2^-24, the bound of tests/test_gpu_multiblank.py.
    (ones,) = torch.autograd.grad((px, py), (logits,), (torch.ones_like(px), torch.ones_like(py)))
    assert _n(ones[..., :C].sum(-1).abs().max()) <= (N + Ny) * (2 * C + 32) * 2.0 ** -24
    assert _n(ones[..., C:].sum(-1).abs().max()) <= (N + Ny) * (2 * N + 32) * 2.0 ** -24


def test_joint_builder_is_the_pruned_builder_on_identity_ranges(ft, dev):
    B, T, S, C, durs = 2, 9, 4, 12, (0, 1, 3)
    rng = np.random.default_rng(2)
    logits = _t(rng.standard_normal((B, T, S + 1, C + 3)).astype(np.float32), dev)
    sym = _t(rng.integers(0, C, (B, S)).astype(np.int32), dev)
    ident = torch.arange(S + 1, dtype=torch.int32, device=dev).expand(B, T, S + 1).contiguous()
    px, py = ft.get_rnnt_logprobs_tdt_joint(logits, sym, 0, durs, None, sigma=0.05)
    qx, qy = ft.get_rnnt_logprobs_tdt_pruned(logits, sym, ident, 0, durs, None, sigma=0.05)
    assert _n(px).tobytes() == _n(qx).tobytes() and _n(py).tobytes() == _n(qy).tobytes()
    px64, py64 = tdt_logprobs(logits.cpu().double(), _n(sym), np.broadcast_to(np.arange(S + 1), (B, T, S + 1)), 0, durs, None,
                              sigma=0.05)
    assert max_rel(_n(px), _n(px64)) <= TOL_F64 and max_rel(_n(py), _n(py64)) <= TOL_F64


# --------------------------------------------------------------------------------------------------------------- loss
LOSS_SHAPES = [(3, 40, 12, 20, 4), (2, 90, 33, 12, 5), (2, 200, 50, 50, 5)]
LOSS_DURATIONS = [(0, 1), (0, 1, 2, 3, 4)]


@functools.lru_cache(maxsize=None)
def _loss_inputs(shape, N):
    """Prune ranges from the ordinary simple loss (get_rnnt_prune_ranges): with durations 0 and 1 a path always exists."""
    import tf_fast_rnnt as ft
    B, T, S, C, r = shape
    dev = torch.device("cuda:0")
    d = synthetic(900 + T, B, T, S, C, ragged=True)
    blank = 0
    sym = (1 + d["symbols"] % (C - 1)).astype(np.int32)
    bdt = _t(d["boundary"], dev)
    _, (gx, gy) = ft.rnnt_loss_simple(_t(d["lm"], dev), _t(d["am"], dev), _t(sym, dev), blank, bdt, calc_gradients=True)
    ranges = _n(ft.get_rnnt_prune_ranges(gx, gy, bdt, r))
    logits = (np.random.default_rng(T + N).standard_normal((B, T, r, C + N)) * 2).astype(np.float32)
    return logits, sym, ranges, d["boundary"], blank


@functools.lru_cache(maxsize=None)
def _loss_reference(shape, durs, delay_penalty):
    """Per-utterance float64 losses and d (sum of losses) / d logits: every reduction follows from them."""
    logits, sym, ranges, bd, blank = _loss_inputs(shape, len(durs))
    l64 = torch.from_numpy(logits).double().requires_grad_(True)
    per = tdt_loss(l64, sym, ranges, blank, durs, bd, 0.05, delay_penalty)
    per.sum().backward()
    return per.detach().numpy(), l64.grad.numpy()


@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
@pytest.mark.parametrize("delay_penalty", [0.0, 0.1])
@pytest.mark.parametrize("durs", LOSS_DURATIONS, ids=str)
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=str)
def test_loss_matches_restatement(ft, dev, shape, durs, delay_penalty, reduction):
    B, T, S, C, r = shape
    logits_np, sym, ranges, bd, blank = _loss_inputs(shape, len(durs))
    per, grad = _loss_reference(shape, durs, delay_penalty)
    assert np.isfinite(per).all()                                  # no utterance drops out
    logits = _t(logits_np, dev).requires_grad_(True)
    loss = ft.rnnt_loss_tdt_pruned(logits, _t(sym, dev), _t(ranges, dev), blank, durs, _t(bd, dev), sigma=0.05,
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
    print(f"tdt loss {shape} {durs} dp={delay_penalty} {reduction}: loss {el:.3g} dlogits {eg:.3g}")
    assert el <= TOL_F64 and eg <= TOL_F64, (el, eg)


def test_unpruned_loss_is_the_pruned_loss_on_identity_ranges(ft, dev):
    B, T, S1, C, durs = 2, 20, 7, 12, (0, 1, 2)
    rng = np.random.default_rng(8)
    joint = rng.standard_normal((B, T, S1, C + 3)).astype(np.float32)
    sym = _t(rng.integers(1, C, (B, S1 - 1)).astype(np.int32), dev)
    bd = _t(np.array([[0, 0, S1 - 1, T], [0, 0, S1 - 2, T - 3]], np.int32), dev)
    ident = torch.arange(S1, dtype=torch.int32, device=dev).expand(B, T, S1).contiguous()
    out = []
    for f in (lambda x: ft.rnnt_loss_tdt(x, sym, 0, durs, bd, sigma=0.05, delay_penalty=0.1),
              lambda x: ft.rnnt_loss_tdt_pruned(x, sym, ident, 0, durs, bd, sigma=0.05, delay_penalty=0.1)):
        x = _t(joint, dev).requires_grad_(True)
        loss = f(x)
        loss.backward()
        out.append((_n(loss), _n(x.grad)))
    assert np.isfinite(out[0][0]).all()
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()


def test_value_errors(ft, dev):
    B, T, S1, C = 1, 4, 3, 6
    joint = torch.zeros(B, T, S1, C + 2, device=dev)
    sym = torch.full((B, S1 - 1), 3, dtype=torch.int32, device=dev)
    ident = torch.arange(S1, dtype=torch.int32, device=dev).expand(B, T, S1).contiguous()
    for rt in ("modified", "constrained", "nonsense"):
        with pytest.raises(ValueError):
            ft.rnnt_loss_tdt(joint, sym, 0, (0, 1), rnnt_type=rt)
        with pytest.raises(ValueError):
            ft.rnnt_loss_tdt_pruned(joint, sym, ident, 0, (0, 1), rnnt_type=rt)
    for bad in ((), (0,), (1, 1), (2, 1), (-1, 1), (0, 17), (0, 1, 2, 3, 4, 5)):
        with pytest.raises(ValueError):
            ft.rnnt_loss_tdt(joint, sym, 0, bad)
        with pytest.raises(ValueError):
            ft.get_rnnt_logprobs_tdt_joint(joint, sym, 0, bad)
    with pytest.raises(ValueError):
        ft.rnnt_loss_tdt(joint, sym, 0, (0, 1), sigma=-0.1)
    with pytest.raises(ValueError):
        ft.rnnt_loss_tdt(joint, sym, C, (0, 1))                   # the termination symbol is a token column
    with pytest.raises(ValueError):
        ft.rnnt_loss_tdt(joint, sym, 0, (0, 1), reduction="nonsense")
    px, py = torch.zeros(B, 1, 2, T + 1, device=dev), torch.zeros(B, 1, 3, T, device=dev)
    for tok, blk in (((), (1,)), ((0,), ()), ((0,), (0,)), ((1, 0), (1,)), ((0,), (17,)), ((0, 1, 2, 3, 4), (1, 2, 3, 4, 5))):
        with pytest.raises(ValueError):
            ft.mutual_information_recursion_tdt(px, py, tok, blk)
    with pytest.raises(ValueError):
        ft.mutual_information_recursion_tdt(px, py, (0, 1), (1,))   # px holds one plane


# ------------------------------------------------------------------------------------------- determinism and capture
def _step_fn(ft, dev, shape, durs):
    B, T, S, C, r = shape
    logits_np, sym, ranges, bd, blank = _loss_inputs(shape, len(durs))
    buf = _t(logits_np, dev)
    symt, rgt, bdt = _t(sym, dev), _t(ranges, dev), _t(bd, dev)

    def step():
        x = buf.clone().requires_grad_(True)          # the leaf is created inside the step
        loss = ft.rnnt_loss_tdt_pruned(x, symt, rgt, blank, durs, bdt, sigma=0.05, delay_penalty=0.1, reduction="none")
        (g,) = torch.autograd.grad(loss.sum(), (x,))
        return loss.detach(), g.detach()              # only detached results leave it
    return buf, step


def test_forward_and_backward_are_bit_reproducible(ft, dev):
    _, step = _step_fn(ft, dev, LOSS_SHAPES[1], LOSS_DURATIONS[1])
    step()
    a = [_n(v).copy() for v in step()]
    b = [_n(v).copy() for v in step()]
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()


def test_step_replays_from_a_graph_with_new_values(ft, dev):
    buf, step = _step_fn(ft, dev, LOSS_SHAPES[0], LOSS_DURATIONS[1])
    g, out = _capture(step)
    for seed in (21, 22):
        buf.copy_(torch.randn(buf.shape, generator=torch.Generator().manual_seed(seed)).to(dev) * 2)
        g.replay()
        torch.cuda.synchronize()
        got = [_n(v).copy() for v in out]
        ref = [_n(v).copy() for v in step()]
        assert np.isfinite(got[0]).all()
        for u, v in zip(got, ref):
            assert u.tobytes() == v.tobytes()
