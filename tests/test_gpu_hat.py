"""HAT (hybrid autoregressive transducer) lattices and losses on the GPU: the ftr_hat_* kernels against the float64
restatement of tests/hat_restatement.py, the normalisation on its own, the losses against a float64 DP, the identity with
the shipped ordinary loss, the band route against the lattice route, extreme blank logits, out-of-range symbols, NaN
containment, determinism and graph replay."""
import numpy as np
import pytest
import torch

from hat_restatement import get_hat_logprobs_joint_torch, get_hat_logprobs_pruned_torch, lattice_loss_torch
from helpers import max_rel, synthetic
from test_gpu_graph import _capture, _same

pytestmark = pytest.mark.gpu

TYPES = ("regular", "modified", "constrained")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _case(seed, B, T, S, C, r, blank, blank_symbols=True, diagonal=False):
    """Random logits, symbols (some equal to blank when blank_symbols), monotone band ranges (random, or along the
    diagonal of each boundary rectangle so that every utterance has a path: diagonal), ragged boundaries."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((B, T, r, C)) * 2).astype(np.float32)
    if blank_symbols:
        sym = rng.integers(0, C, (B, S)).astype(np.int32)
        sym[0, 1] = blank
    else:
        others = np.array([c for c in range(C) if c != blank])
        sym = others[rng.integers(0, C - 1, (B, S))].astype(np.int32)
    bd = np.zeros((B, 4), np.int32)
    bd[:, 2] = S - np.arange(B) % 3
    bd[:, 3] = T - 2 * (np.arange(B) % 3)
    if diagonal:   # steps of at most one row per frame (S <= T) and r >= 2: the band holds a path from (0,0) to (se,te)
        t = np.minimum(np.arange(T)[None, :], bd[:, 3:4] - 1)
        s0 = np.clip(t * bd[:, 2:3] // bd[:, 3:4] - (r - 1) // 2, 0, S - r + 1)
    else:
        s0 = np.sort(rng.integers(0, S - r + 2, (B, T)), axis=1)
    ranges = (s0[..., None] + np.arange(r)).astype(np.int32)
    return logits, sym, ranges, bd


def _check_builder(px, py, want_px, want_py):
    pxn, pyn = px.detach().cpu().numpy(), py.detach().cpu().numpy()
    wx, wy = want_px.detach().cpu().numpy(), want_py.detach().cpu().numpy()
    assert np.array_equal(np.isneginf(pxn), np.isneginf(wx)) and np.array_equal(np.isneginf(pyn), np.isneginf(wy))
    assert np.isfinite(pxn[~np.isneginf(wx)]).all() and np.isfinite(pyn[~np.isneginf(wy)]).all()
    fin = np.isfinite(wx)
    np.testing.assert_allclose(pxn[fin], wx[fin], rtol=1e-5, atol=2e-5)
    fin = np.isfinite(wy)
    np.testing.assert_allclose(pyn[fin], wy[fin], rtol=1e-5, atol=2e-5)


def _check_backward(logits, px, py, l64, px64, py64, seed):
    """d/d logits of sum(wx * px) + sum(wy * py), upstream weights nonzero everywhere (-inf cells included: they must
    contribute nothing), against float64 autograd of the restatement."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    wx = torch.rand(px.shape, generator=g, dtype=torch.float64) + 0.5
    wy = torch.rand(py.shape, generator=g, dtype=torch.float64) + 0.5
    dev = logits.device
    (got,) = torch.autograd.grad((px, py), (logits,), (wx.float().to(dev), wy.float().to(dev)))
    (want,) = torch.autograd.grad((px64, py64), (l64,), (wx.to(dev), wy.to(dev)))
    assert max_rel(got.cpu().numpy(), want.cpu().numpy()) <= 2e-5


@pytest.mark.parametrize("C", [2, 7, 256, 500, 501, 1024, 2048, 4100])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_hat_builders_match_restatement(ft, dev, C, where):
    """get_hat_logprobs_pruned / get_hat_logprobs_joint against the float64 restatement: every lse_rows variant (register
    kernels up to C = 2048, the two-pass vector kernel beyond, the scalar kernel for C % 4 != 0), blank in the first, a
    middle and the tail quad; -inf pattern exact, symbols equal to blank -inf with no gradient, backward normwise."""
    blank = {"first": 0, "middle": C // 2, "last": C - 1}[where]
    B, T, S, r = 3, 12, 5, 3
    logits_np, sym, ranges, bd = _case(1000 + C + blank, B, T, S, C, r, blank)
    symt, rgt, bdt = _t(sym, dev), _t(ranges, dev), _t(bd, dev)
    for rt in TYPES:
        logits = _t(logits_np, dev).requires_grad_(True)
        px, py = ft.get_hat_logprobs_pruned(logits, symt, rgt, blank, bdt, rt)
        l64 = logits.detach().double().requires_grad_(True)
        px64, py64 = get_hat_logprobs_pruned_torch(l64, symt, rgt, blank, bdt, rt)
        _check_builder(px, py, px64, py64)
        is_blank = (symt == blank).unsqueeze(-1).expand_as(px)
        assert is_blank.any() and torch.isneginf(px[is_blank]).all()
        _check_backward(logits, px, py, l64, px64, py64, C + blank)
    # the unpruned builder: identity ranges
    rng = np.random.default_rng(C + blank)
    joint_np = (rng.standard_normal((B, 7, S + 1, C)) * 2).astype(np.float32)
    bdj = bd.copy()
    bdj[:, 3] = np.minimum(bdj[:, 3], 7)
    for rt in TYPES:
        logits = _t(joint_np, dev).requires_grad_(True)
        px, py = ft.get_hat_logprobs_joint(logits, symt, blank, _t(bdj, dev), rt)
        l64 = logits.detach().double().requires_grad_(True)
        px64, py64 = get_hat_logprobs_joint_torch(l64, symt, blank, _t(bdj, dev), rt)
        _check_builder(px, py, px64, py64)
        _check_backward(logits, px, py, l64, px64, py64, 7 * C + blank)


@pytest.mark.parametrize("C", [7, 64, 257])
def test_hat_rows_normalise(ft, dev, C):
    """Independent of the restatement: with logits constant along s and S = C-1 symbols that enumerate every non-blank
    once, py[b,0,t] and the px[b,s,t] of one frame are the log-probs of every outcome of that frame's row."""
    B, T, blank = 2, 6, C // 3
    g = torch.Generator(device="cpu").manual_seed(C)
    row = torch.randn((B, T, 1, C), generator=g) * 3
    row[0, 0, 0, blank] = 25.0
    row[1, 1, 0, blank] = -25.0
    logits = row.expand(B, T, C, C).contiguous().to(dev)
    sym = torch.tensor([c for c in range(C) if c != blank], dtype=torch.int32).expand(B, C - 1).contiguous().to(dev)
    px, py = ft.get_hat_logprobs_joint(logits, sym, blank, None, "regular")
    lp = torch.cat((py[:, :1, :], px[:, :, :T]), dim=1).double()        # [B, C, T]
    assert torch.isfinite(lp).all()
    total = torch.logsumexp(lp, dim=1)
    assert total.abs().max().item() <= 1e-5


@pytest.mark.parametrize("rnnt_type", TYPES)
@pytest.mark.parametrize("delay_penalty", [0.0, 0.1])
def test_hat_losses_match_float64_dp(ft, dev, rnnt_type, delay_penalty):
    """hat_loss_pruned and hat_loss against a float64 log-domain DP over the restated px / py with torch autograd, for
    every reduction: loss within 1e-4 relative, d/d logits within 1e-4 normwise."""
    from tf_fast_rnnt.rnnt_loss import _apply_delay_penalty
    B, T, S, C, r = 3, 10, 5, 9, 3
    blank = 4
    logits_np, sym, ranges, bd = _case(77, B, T, S, C, r, blank, blank_symbols=False, diagonal=True)
    joint_np = (np.random.default_rng(78).standard_normal((B, T, S + 1, C)) * 2).astype(np.float32)
    symt, bdt = _t(sym, dev), _t(bd, dev)
    wgt = torch.tensor([0.7, 1.3, 0.9], device=dev)
    for kind, x_np in (("pruned", logits_np), ("unpruned", joint_np)):
        l64 = torch.from_numpy(x_np).double().requires_grad_(True)
        if kind == "pruned":
            px64, py64 = get_hat_logprobs_pruned_torch(l64, torch.from_numpy(sym), torch.from_numpy(ranges), blank,
                                                       torch.from_numpy(bd), rnnt_type)
        else:
            px64, py64 = get_hat_logprobs_joint_torch(l64, torch.from_numpy(sym), blank, torch.from_numpy(bd), rnnt_type)
        px64 = _apply_delay_penalty(px64, torch.from_numpy(bd), rnnt_type, delay_penalty)
        per = lattice_loss_torch(px64, py64, bd, rnnt_type)
        for reduction in ("none", "mean", "sum"):
            logits = _t(x_np, dev).requires_grad_(True)
            if kind == "pruned":
                loss = ft.hat_loss_pruned(logits, symt, _t(ranges, dev), blank, bdt, rnnt_type, delay_penalty, reduction)
            else:
                loss = ft.hat_loss(logits, symt, blank, bdt, rnnt_type, delay_penalty, reduction)
            if reduction == "none":
                want = per
                (loss * wgt).sum().backward()
                (g64,) = torch.autograd.grad((per * wgt.cpu().double()).sum(), l64, retain_graph=True)
            else:
                want = per.mean() if reduction == "mean" else per.sum()
                loss.backward()
                (g64,) = torch.autograd.grad(want, l64, retain_graph=True)
            np.testing.assert_allclose(loss.detach().cpu().numpy(), want.detach().numpy(), rtol=1e-4)
            assert max_rel(logits.grad.cpu().numpy(), g64.numpy()) <= 1e-4, (kind, reduction)


def test_hat_identity_with_ordinary_pruned_loss(ft, dev):
    """With y = logits except y[blank] = logits[blank] - logsumexp_{c != blank} logits (torch), and symbols never blank,
    hat_loss_pruned(y) is rnnt_loss_pruned(logits).  A c3-shaped slice (S + T >= 1100): the segmented band route."""
    B, T, S, C, r = 2, 1000, 200, 500, 5
    d = synthetic(2024, B, T, S, C, ragged=True)
    blank = d["termination_symbol"]
    am, lm, sym, bd = (_t(d[k], dev) for k in ("am", "lm", "symbols", "boundary"))
    _, (gx, gy) = ft.rnnt_loss_simple(lm, am, sym, blank, bd, reduction="sum", calc_gradients=True)
    ranges = ft.get_rnnt_prune_ranges(gx, gy, bd, r)
    am_p, lm_p = ft.do_rnnt_pruning(am, lm, ranges)
    base = (am_p + lm_p).detach()
    nb = torch.ones(C, dtype=torch.bool, device=dev)
    nb[blank] = False
    x1 = base.clone().requires_grad_(True)
    want = ft.rnnt_loss_pruned(x1, sym, ranges, blank, bd, reduction="none", delay_penalty=0.05)
    want.sum().backward()
    x2 = base.clone().requires_grad_(True)
    Z = torch.logsumexp(x2[..., nb], dim=-1)
    y = torch.cat((x2[..., :blank], (x2[..., blank] - Z).unsqueeze(-1), x2[..., blank + 1:]), dim=-1)
    got = ft.hat_loss_pruned(y, sym, ranges, blank, bd, reduction="none", delay_penalty=0.05)
    got.sum().backward()
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().cpu().numpy(), rtol=1e-5)
    assert max_rel(x2.grad.cpu().numpy(), x1.grad.cpu().numpy()) <= 1e-4


@pytest.mark.parametrize("rnnt_type", ["regular", "modified"])
@pytest.mark.parametrize("cfg", [(3, 40, 12, 20, 4), (2, 90, 33, 12, 5), (4, 64, 20, 16, 2), (2, 130, 50, 24, 8), (2, 70, 40, 8, 16), (2, 70, 40, 8, 15), (2, 60, 30, 8, 7),
                                 (3, 33, 5, 7, 3), (2, 200, 50, 50, 5), (1, 300, 10, 16, 11), (2, 25, 20, 8, 6)])
def test_hat_band_route_matches_lattice_route(ft, dev, rnnt_type, cfg, monkeypatch):
    """hat_loss_pruned on the band (chain kernels and segmented route) against the full-size lattices: losses within
    1e-5 relative, d/d logits within 1e-4 normwise.  r = 16 is served by the lattice route only."""
    B, T, S, C, r = cfg
    d = synthetic(500 + T + S, B, T, S, C, ragged=True)
    blank = C // 2                                       # a blank in the middle; the symbols that equal it move to C - 1
    am, lm, sym, bd = (_t(d[k], dev) for k in ("am", "lm", "symbols", "boundary"))
    _, (gx, gy) = ft.rnnt_loss_simple(lm, am, sym, d["termination_symbol"], bd, rnnt_type, reduction="sum",
                                      calc_gradients=True)
    ranges = ft.get_rnnt_prune_ranges(gx, gy, bd, r)
    am_p, lm_p = ft.do_rnnt_pruning(am, lm, ranges)
    base = (2 * torch.tanh(am_p + lm_p)).detach()
    sym = torch.where(sym == blank, C - 1, sym).to(torch.int32)
    wgt = torch.rand((B,), generator=torch.Generator(device="cpu").manual_seed(2)).to(dev) + 0.5
    outs = {}
    for route, impl in (("band", "chain"), ("band", "segments"), ("lattice", None)):
        monkeypatch.setenv("FTR_PRUNED_ROUTE", route)
        if impl:
            monkeypatch.setenv("FTR_BAND_IMPL", impl)
        else:
            monkeypatch.delenv("FTR_BAND_IMPL", raising=False)
        logits = base.clone().requires_grad_(True)
        loss = ft.hat_loss_pruned(logits, sym, ranges, blank, bd, rnnt_type, 0.1, "none")
        (loss * wgt).sum().backward()
        outs[impl or route] = (loss.detach().cpu().numpy(), logits.grad.cpu().numpy())
    ref_loss, ref_grad = outs["lattice"]
    fin = np.isfinite(ref_loss)
    assert fin.any()
    for k in ("chain", "segments"):
        assert np.array_equal(np.isfinite(outs[k][0]), fin), k
        np.testing.assert_allclose(outs[k][0][fin], ref_loss[fin], rtol=1e-5, err_msg=k)
        assert max_rel(outs[k][1][fin], ref_grad[fin]) <= 1e-4, k


@pytest.mark.parametrize("C", [7, 64])
def test_hat_extreme_blank_logits(ft, dev, C):
    """Blank logits of -80 .. 80: finite log-probs and gradients, px and py within 1e-5 relative of float64.  py =
    -softplus(-x[blank]) is compared with atol = 0, so it checks both tails of softplus: -1.8e-35 at x[blank] = 80 needs
    log1p, not log(1 + .).  px shows its softplus(x[blank]) term only where that term is not negligible next to
    x[sym] - Z (the large tail); at x[blank] = -80 it vanishes in float32, so px does not test the small tail."""
    B, T, S, r, blank = 2, 10, 4, 2, C - 2
    logits_np, sym, ranges, bd = _case(C, B, T, S, C, r, blank, blank_symbols=False, diagonal=True)
    vals = np.array([-80.0, -30.0, 0.0, 30.0, 80.0], np.float32)
    logits_np[..., blank] = vals[np.arange(T) % 5][None, :, None]
    logits = _t(logits_np, dev).requires_grad_(True)
    symt, rgt, bdt = _t(sym, dev), _t(ranges, dev), _t(bd, dev)
    px, py = ft.get_hat_logprobs_pruned(logits, symt, rgt, blank, bdt, "modified")
    l64 = logits.detach().double()
    px64, py64 = get_hat_logprobs_pruned_torch(l64, symt, rgt, blank, bdt, "modified")
    for got, want, atol in ((px, px64, 1e-6), (py, py64, 0.0)):
        got, want = got.detach().cpu().double().numpy(), want.cpu().numpy()
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), fin)
        np.testing.assert_allclose(got[fin], want[fin], rtol=1e-5, atol=atol)
    pyf = py.detach().cpu()[torch.isfinite(py64.cpu())]
    assert pyf.min().item() < -79 and 0 > pyf.max().item() > -1e-30
    loss = ft.hat_loss_pruned(logits, symt, rgt, blank, bdt, "regular", 0.0, "none")
    assert torch.isfinite(loss).all()
    loss.sum().backward()
    assert torch.isfinite(logits.grad).all()


@pytest.mark.parametrize("route", ["band", "lattice"])
def test_hat_nan_stays_in_its_utterance(ft, dev, route, monkeypatch):
    monkeypatch.setenv("FTR_PRUNED_ROUTE", route)
    B, T, S, C, r, blank = 3, 20, 6, 9, 3, 0
    logits_np, sym, ranges, bd = _case(9, B, T, S, C, r, blank, blank_symbols=False, diagonal=True)
    assert ranges[1, 0, 0] == 0                        # row (b=1, t=0, k=0) is lattice cell (0, 0): on every path
    logits_np[1, 0, 0, 3] = np.nan
    loss = ft.hat_loss_pruned(_t(logits_np, dev), _t(sym, dev), _t(ranges, dev), blank, _t(bd, dev), reduction="none")
    loss = loss.cpu().numpy()
    assert np.isnan(loss[1]) and np.isfinite(loss[[0, 2]]).all()


@pytest.mark.parametrize("blank", [0, 6])
def test_hat_out_of_range_symbols_are_clamped(ft, dev, blank):
    """A symbol outside [0, C) reads the clamped column in the forward (as the ordinary builder does), and the backward
    sends its gradient to that same column -- or, when the clamped column is blank, px is -inf and gets no gradient."""
    B, T, S, C, r = 2, 12, 5, 7, 3
    logits_np, sym, ranges, bd = _case(55 + blank, B, T, S, C, r, blank, blank_symbols=False)
    sym[0, 1], sym[0, 3], sym[1, 2] = -1, C, -5
    symt, rgt, bdt = _t(sym, dev), _t(ranges, dev), _t(bd, dev)
    for rt in TYPES:
        logits = _t(logits_np, dev).requires_grad_(True)
        px, py = ft.get_hat_logprobs_pruned(logits, symt, rgt, blank, bdt, rt)
        l64 = logits.detach().double().requires_grad_(True)
        px64, py64 = get_hat_logprobs_pruned_torch(l64, symt.clamp(0, C - 1), rgt, blank, bdt, rt)
        _check_builder(px, py, px64, py64)
        _check_backward(logits, px, py, l64, px64, py64, 100 + blank)


def _replay_case(ft, dev):
    B, T, S, C, r = 3, 120, 30, 40, 5
    d = synthetic(31337, B, T, S, C, ragged=True)
    blank = d["termination_symbol"]
    am, lm, sym, bd = (_t(d[k], dev) for k in ("am", "lm", "symbols", "boundary"))
    _, (gx, gy) = ft.rnnt_loss_simple(lm, am, sym, blank, bd, reduction="sum", calc_gradients=True)
    ranges = ft.get_rnnt_prune_ranges(gx, gy, bd, r)        # marked as a band: no host read on the route decision
    g = torch.Generator(device="cpu").manual_seed(3)
    buf = (torch.randn((B, T, r, C), generator=g) * 2).to(dev)

    def step():
        # the leaf is made inside the step and only detached results leave it (the shape of bench.pruned_step): the
        # autograd graph, and with it the stream its leaf node was created on, never outlives one step
        logits = buf.detach().requires_grad_(True)
        loss = ft.hat_loss_pruned(logits, sym, ranges, blank, bd, "regular", 0.1, "sum")
        loss.backward()
        return {"loss": loss.detach(), "grad": logits.grad}

    return buf, g, step


def test_hat_fwd_bwd_is_deterministic(ft, dev):
    """Two eager fwd+bwd steps on the same inputs give the same bits (loss and d/d logits)."""
    _, _, step = _replay_case(ft, dev)
    a, b = step(), step()
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_hat_step_replays_from_a_graph_with_new_values(ft, dev):
    """hat_loss_pruned fwd+bwd captured into a graph once, replayed 5 times with new logits values in the same buffer:
    each replay gives what the eager step gives (the rule of test_gpu_graph._same)."""
    buf, g, step = _replay_case(ft, dev)
    graph, out = _capture(step)
    for i in range(5):
        buf.copy_(torch.randn(buf.shape, generator=g) * 2)
        graph.replay()
        torch.cuda.synchronize()
        got = {k: v.clone() for k, v in out.items()}
        ref = step()
        torch.cuda.synchronize()
        for k in got:
            _same(got[k], ref[k], f"replay {i}: {k}")
