"""rnnt_loss_tdt_mixed[_pruned] on the GPU: L = (1 - omega) L_tdt + omega L_rnnt, the TDT loss and the ordinary loss on the
token head of the same joiner rows in one pass (include/ftr_tdt_mix.h, the <MIX> kernels of csrc/tdt_logprobs.hip).

Shapes: B=2 T=12 S=5 r=3, utterance 1 ragged (boundary [0,0,3,9]), band ranges built by hand as in tests/test_gpu_lowp.py.
Row widths W = C + N where the kernels can go wrong: 16 (vector path, the token / duration border inside a 4-vector), 14 and
37 (scalar path), 504 (vector path).  Blank is the first column in some cases and the last token column in others, one symbol
sits in column 3.  Duration sets (0,1), (0,1,2,3,4), (1,2) (no zero duration: first = 0), and (0,1,2,3) for the one width that
needs four duration columns (W = 504 with C = 500: none of the other sets has four entries).

The no-path check runs at s_range = 4, not 3: its one-frame utterance with s_end = 3 needs the four cells (0..3, 0) inside the
band for the ORDINARY loss to have a path (three symbols in frame 0, then blank), which the check requires (finite loss at
omega = 1); the boundary and the durations are the stated ones.

Tolerances.  Against float64: TOL_F64 = 1e-4 normwise (tests/test_gpu_config_parity.py).  Linearity in omega: 2e-6 normwise,
derived, not measured: g(0.5) and 0.5 g(0) + 0.5 g(1) (the latter formed in float64) differ by fewer than sixteen float32
roundings of 2^-24 each on terms no larger than max|g| (halving the multipliers is exact, so the occupancies that enter are
the same numbers), 16 * 2^-24 < 1e-6 < 2e-6."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import max_rel

pytestmark = pytest.mark.gpu

B, T, S, R = 2, 12, 5, 3
BOUNDARY = np.array([[0, 0, S, T], [0, 0, 3, 9]], np.int32)
TOL_F64 = 1e-4
TOL_LINEAR = 2e-6
OMEGAS = (0.1, 0.5, 1.0)
ROUTES = ["default", "lattice"]
# name: (C, durations, blank is the last token column?, sigma, delay_penalty)
CASES = {"w16_vec_border": (11, (0, 1, 2, 3, 4), False, 0.0, 0.0),
         "w14_scalar_no_zero": (12, (1, 2), True, 0.05, 0.0),
         "w14_scalar": (12, (0, 1), False, 0.0, 0.0),
         "w37_scalar_penalty": (32, (0, 1, 2, 3, 4), True, 0.0, 0.01),
         "w504_vec": (500, (0, 1, 2, 3), False, 0.0, 0.0)}
_ERRORS = {}


@pytest.fixture(autouse=True)
def _route_unset(monkeypatch):
    monkeypatch.delenv("FTR_PRUNED_ROUTE", raising=False)
    monkeypatch.delenv("FTR_BAND_IMPL", raising=False)


def _set_route(monkeypatch, route):
    if route == "lattice":
        monkeypatch.setenv("FTR_PRUNED_ROUTE", "lattice")


def band_ranges(r=R, boundary=BOUNDARY):
    """A band built by hand: ranges[b,t,0] climbs from 0 to s_end + 1 - r over the utterance's frames, steps <= 1."""
    rg = np.zeros((B, T, r), np.int32)
    for b in range(B):
        top, te = max(int(boundary[b, 2]) + 1 - r, 0), int(boundary[b, 3])
        s0 = np.clip((np.arange(T) * top + te - 2) // max(te - 1, 1), 0, top)
        rg[b] = s0[:, None] + np.arange(r)[None, :]
    return rg


def dipped_ranges():
    """band_ranges() with the start of one frame of each utterance stepped back by one: contiguous rows that stay inside
    the lattice, but not a band (ranges[b,t,0] decreases), so every route is the lattice route."""
    rg = band_ranges()
    for b in range(B):
        s0 = rg[b, :, 0]
        t = int(np.argmax(s0 >= 1)) + 1            # the frame after the first step up
        assert s0[t] >= 1 and s0[t - 1] == s0[t]
        rg[b, t] -= 1
        assert rg[b, t, 0] < rg[b, t - 1, 0]
    return rg


_INPUTS = {}


def inputs(name, s1=R):
    """(x float32 cpu [B,T,s1,C+N], symbols, blank): standard normal x 3; one symbol sits in column 3.  Cached, never modified."""
    if (name, s1) not in _INPUTS:
        C, durs, blank_last, _, _ = CASES[name]
        rng = np.random.default_rng(2000 + C + len(durs))
        x = torch.from_numpy((3.0 * rng.standard_normal((B, T, s1, C + len(durs)))).astype(np.float32))
        blank = C - 1 if blank_last else 0
        sym = rng.integers(1, C - 1, (B, S)).astype(np.int32)
        sym[:, 0] = 3
        _INPUTS[(name, s1)] = (x, sym, blank)
    return _INPUTS[(name, s1)]


_REFS = {}


def reference(oracle, name, rg_name="band"):
    """Float64 references of the two parts on x.double(), computed once per input: the per-utterance TDT losses and the
    gradient of their sum (tests/tdt_restatement.py), the sum-reduced ordinary loss on the token columns and its gradient
    (the oracle, recursion in float64) zero-padded to width C + N."""
    if (name, rg_name) in _REFS:
        return _REFS[(name, rg_name)]
    import tdt_restatement as R64
    C, durs, _, sigma, penalty = CASES[name]
    x, sym, blank = inputs(name)
    rg = band_ranges() if rg_name == "band" else dipped_ranges()
    xd = x.double().requires_grad_(True)
    l_tdt = R64.tdt_loss(xd, sym, rg, blank, durs, BOUNDARY, sigma, penalty)
    assert torch.isfinite(l_tdt).all(), "the reference has no TDT path: the case checks nothing"
    l_tdt.sum().backward()
    l0, g0 = oracle.rnnt_loss_pruned_grad(np.ascontiguousarray(x[..., :C].numpy()), sym, rg, blank, BOUNDARY, "regular", penalty,
                                          reduction="sum", dtype=np.float64)
    g0p = np.zeros(tuple(x.shape), np.float64)
    g0p[..., :C] = g0
    _REFS[(name, rg_name)] = (float(l_tdt.detach().sum()), xd.grad.numpy(), float(l0), g0p)
    return _REFS[(name, rg_name)]


def run(ft, dev, x, sym, rg, blank, durs, omega, boundary=BOUNDARY, reduction="sum", fn=None, **kw):
    """(loss, gradient of loss.sum()) as cpu tensors; ``fn``: another loss of the same calling convention."""
    xx = x.to(dev).requires_grad_(True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if fn is None:
        loss = ft.rnnt_loss_tdt_mixed_pruned(xx, t(sym), t(rg), blank, durs, omega, boundary=t(boundary), reduction=reduction, **kw)
    else:
        loss = fn(xx, t(sym), t(rg), blank, durs, boundary=t(boundary), reduction=reduction, **kw)
    loss.sum().backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), xx.grad.cpu()


def _record(key, e_loss, e_g):
    """Keeps the measured errors; where FTR_TDT_MIX_PARITY_OUT names a file they are also written there
    (profiles/tdt_mix_parity_errors.json was recorded this way)."""
    _ERRORS[key] = dict(loss_normwise_vs_f64=e_loss, grad_normwise_vs_f64=e_g)
    path = os.environ.get("FTR_TDT_MIX_PARITY_OUT")
    if path:
        worst = {k: max(e[k] for e in _ERRORS.values()) for k in ("loss_normwise_vs_f64", "grad_normwise_vs_f64")}
        with open(path, "w") as f:
            json.dump(dict(tolerance=TOL_F64, worst=worst, cases=_ERRORS), f, indent=1, sort_keys=True)
            f.write("\n")


def _frames_past_the_end_are_zero(g):
    for b in range(B):
        assert (g[b, int(BOUNDARY[b, 3]):].numpy() == 0).all(), b


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_float64(ft, dev, oracle, monkeypatch, name, route):
    C, durs, _, sigma, penalty = CASES[name]
    x, sym, blank = inputs(name)
    ref_tdt, g_tdt, ref0, g0 = reference(oracle, name)
    _set_route(monkeypatch, route)
    for omega in OMEGAS:
        before = ft._lib.band_tdt_recursions
        loss, g = run(ft, dev, x, sym, band_ranges(), blank, durs, omega, sigma=sigma, delay_penalty=penalty)
        assert ft._lib.band_tdt_recursions - before == (1 if route == "default" and omega < 1.0 else 0)
        want_loss = (1.0 - omega) * ref_tdt + omega * ref0 if omega < 1.0 else ref0
        want_g = (1.0 - omega) * g_tdt + omega * g0 if omega < 1.0 else g0
        e_loss, e_g = max_rel(loss.numpy(), want_loss), max_rel(g.numpy(), want_g)
        print(f"{name} {route} omega={omega}: loss {e_loss:.3g} grad {e_g:.3g}")
        _record(f"{name}/{route}/omega={omega}", e_loss, e_g)
        assert e_loss <= TOL_F64 and e_g <= TOL_F64, (name, route, omega, e_loss, e_g)
        _frames_past_the_end_are_zero(g)


def test_parity_on_ranges_that_are_no_band(ft, dev, oracle):
    """Contiguous rows whose start steps back once: the lattice route without the knob, same references."""
    name = "w14_scalar"
    C, durs, _, sigma, penalty = CASES[name]
    x, sym, blank = inputs(name)
    ref_tdt, g_tdt, ref0, g0 = reference(oracle, name, "dipped")
    before = ft._lib.band_tdt_recursions
    for omega in (0.1, 1.0):
        loss, g = run(ft, dev, x, sym, dipped_ranges(), blank, durs, omega)
        want_loss = (1.0 - omega) * ref_tdt + omega * ref0 if omega < 1.0 else ref0
        want_g = (1.0 - omega) * g_tdt + omega * g0 if omega < 1.0 else g0
        e_loss, e_g = max_rel(loss.numpy(), want_loss), max_rel(g.numpy(), want_g)
        print(f"{name} dipped omega={omega}: loss {e_loss:.3g} grad {e_g:.3g}")
        _record(f"{name}/no_band/omega={omega}", e_loss, e_g)
        assert e_loss <= TOL_F64 and e_g <= TOL_F64, (omega, e_loss, e_g)
        _frames_past_the_end_are_zero(g)
    assert ft._lib.band_tdt_recursions == before


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ["w16_vec_border", "w14_scalar_no_zero", "w504_vec"])
def test_omega_zero_is_the_tdt_loss_itself(ft, dev, monkeypatch, name, route):
    C, durs, _, sigma, penalty = CASES[name]
    x, sym, blank = inputs(name)
    _set_route(monkeypatch, route)
    for reduction in ("none", "mean"):
        loss, g = run(ft, dev, x, sym, band_ranges(), blank, durs, 0.0, reduction=reduction, sigma=sigma, delay_penalty=penalty)
        loss_t, g_t = run(ft, dev, x, sym, band_ranges(), blank, durs, None, reduction=reduction, fn=ft.rnnt_loss_tdt_pruned,
                          sigma=sigma, delay_penalty=penalty)
        assert torch.equal(loss, loss_t) and torch.equal(g, g_t), (name, route, reduction)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", list(CASES))
def test_omega_one_is_the_ordinary_loss_on_the_token_columns(ft, dev, monkeypatch, name, route):
    C, durs, _, sigma, penalty = CASES[name]
    x, sym, blank = inputs(name)
    _set_route(monkeypatch, route)
    before = ft._lib.band_tdt_recursions
    loss, g = run(ft, dev, x, sym, band_ranges(), blank, durs, 1.0, reduction="none", sigma=sigma, delay_penalty=penalty)
    assert ft._lib.band_tdt_recursions == before, "omega == 1 ran a TDT recursion"
    assert (g[..., C:].numpy() == 0).all()
    ordinary = lambda xx, sy, rg, bl, _durs, boundary, reduction: ft.rnnt_loss_pruned(xx, sy, rg, bl, boundary, "regular", penalty,
                                                                                      reduction=reduction)
    loss_o, g_o = run(ft, dev, x[..., :C].contiguous(), sym, band_ranges(), blank, durs, None, reduction="none", fn=ordinary)
    assert max_rel(loss.numpy(), loss_o.numpy()) <= 1e-4 and max_rel(g[..., :C].numpy(), g_o.numpy()) <= 1e-4
    _frames_past_the_end_are_zero(g)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ["w16_vec_border", "w14_scalar_no_zero", "w37_scalar_penalty", "w504_vec"])
def test_gradient_and_loss_are_linear_in_omega(ft, dev, monkeypatch, name, route):
    C, durs, _, sigma, penalty = CASES[name]
    x, sym, blank = inputs(name)
    _set_route(monkeypatch, route)
    out = {w: run(ft, dev, x, sym, band_ranges(), blank, durs, w, reduction="none", sigma=sigma, delay_penalty=penalty)
           for w in (0.0, 0.5, 1.0)}
    for i, what in enumerate(("loss", "grad")):
        mid = 0.5 * out[0.0][i].double().numpy() + 0.5 * out[1.0][i].double().numpy()
        e = max_rel(out[0.5][i].numpy(), mid)
        print(f"{name} {route}: {what} linearity {e:.3g}")
        assert e <= TOL_LINEAR, (name, route, what, e)


@pytest.mark.parametrize("route", ROUTES)
def test_an_utterance_without_a_tdt_path(ft, dev, monkeypatch, route):
    """durations (1,2): every symbol costs a frame, and utterance 1 has three symbols in one frame."""
    import tdt_restatement as R64
    name, r = "w14_scalar_no_zero", 4
    C, durs, _, sigma, penalty = CASES[name]
    assert durs == (1, 2)
    bd = np.array([[0, 0, S, T], [0, 0, 3, 1]], np.int32)
    x, sym, blank = inputs(name, r)
    rg = band_ranges(r, bd)
    l64 = R64.tdt_loss(x.double(), sym, rg, blank, durs, bd, sigma, penalty)
    assert torch.isfinite(l64[0]) and l64[1] == float("inf"), "the restatement disagrees about the paths"
    _set_route(monkeypatch, route)
    half = run(ft, dev, x, sym, rg, blank, durs, 0.5, boundary=bd, reduction="none", sigma=sigma)
    one = run(ft, dev, x, sym, rg, blank, durs, 1.0, boundary=bd, reduction="none", sigma=sigma)
    assert torch.isfinite(half[0][0]) and half[0][1] == float("inf")
    assert torch.isfinite(one[0]).all()
    assert torch.isfinite(half[1]).all() and torch.isfinite(one[1]).all()
    # utterance 1 at omega = 0.5: the ordinary part alone, half of what omega = 1 gives (halving is exact: the derivation of
    # TOL_LINEAR with g(0) = 0)
    assert half[1][1].abs().max() > 0 and (half[1][1][..., C:].numpy() == 0).all()
    assert max_rel(half[1][1].numpy(), 0.5 * one[1][1].double().numpy()) <= TOL_LINEAR
    # the neighbour is what it is without it
    alone = {}
    for w in (0.5, 1.0):
        xx = x[:1].to(dev).requires_grad_(True)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        loss = ft.rnnt_loss_tdt_mixed_pruned(xx, t(sym[:1]), t(rg[:1]), blank, durs, w, boundary=t(bd[:1]), reduction="none", sigma=sigma)
        loss.sum().backward()
        alone[w] = (loss.detach().cpu(), xx.grad.cpu())
    for w, got in ((0.5, half), (1.0, one)):
        assert torch.equal(got[0][:1], alone[w][0]) and torch.equal(got[1][:1], alone[w][1]), w


def test_unpruned_form_is_the_pruned_form_on_identity_ranges(ft, dev):
    name = "w16_vec_border"
    C, durs, _, sigma, penalty = CASES[name]
    x, sym, blank = inputs(name, S + 1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rg = np.broadcast_to(np.arange(S + 1, dtype=np.int32), (B, T, S + 1))
    for omega in (0.1, 1.0):
        xx = x.to(dev).requires_grad_(True)
        loss = ft.rnnt_loss_tdt_mixed(xx, t(sym), blank, durs, omega, boundary=t(BOUNDARY), sigma=0.05, delay_penalty=0.01,
                                      reduction="none")
        loss.sum().backward()
        loss_p, g_p = run(ft, dev, x, sym, rg, blank, durs, omega, reduction="none", sigma=0.05, delay_penalty=0.01)
        assert torch.isfinite(loss).all()
        assert torch.equal(loss.detach().cpu(), loss_p) and torch.equal(xx.grad.cpu(), g_p), omega


def test_a_captured_step_replays_with_new_values(ft, dev):
    """One band-route step at omega = 0.1 in a graph: a single stream of kernels, no host read, no memset or memcpy node."""
    from test_gpu_graph import _capture
    name = "w504_vec"
    C, durs, _, sigma, penalty = CASES[name]
    x, sym, blank = inputs(name)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    xbuf, symd, rgd, bdd = x.to(dev).clone(), t(sym), t(band_ranges()), t(BOUNDARY)

    def step():
        xx = xbuf.detach().requires_grad_(True)
        loss = ft.rnnt_loss_tdt_mixed_pruned(xx, symd, rgd, blank, durs, 0.1, boundary=bdd, reduction="sum")
        loss.backward()
        return dict(loss=loss.detach(), grad=xx.grad)

    before = ft._lib.band_tdt_recursions
    g, out = _capture(step)
    assert ft._lib.band_tdt_recursions == before + 4, "the warm-up or the captured step left the band route"
    for seed in (21, 22, 23):
        fresh = torch.from_numpy((3.0 * np.random.default_rng(seed).standard_normal(tuple(x.shape))).astype(np.float32))
        xbuf.copy_(fresh.to(dev))                       # new values, same buffer
        g.replay()
        torch.cuda.synchronize()
        got = {k: v.clone() for k, v in out.items()}
        ref = step()                                    # eager, same buffer
        torch.cuda.synchronize()
        assert torch.isfinite(got["loss"]).all() and got["grad"].abs().max() > 0
        for k in got:
            assert torch.equal(got[k], ref[k]), (seed, k)


def test_refusals(ft, dev):
    name = "w16_vec_border"
    C, durs, _, _, _ = CASES[name]
    x, sym, blank = inputs(name)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    symd, rgd, bdd = t(sym), t(band_ranges()), t(BOUNDARY)
    for omega in (0.5, 1.0):
        with pytest.raises(TypeError, match="float32"):
            ft.rnnt_loss_tdt_mixed_pruned(x.to(dev).to(torch.bfloat16), symd, rgd, blank, durs, omega, boundary=bdd)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ft.rnnt_loss_tdt_mixed_pruned(x, sym, band_ranges(), blank, durs, omega, boundary=BOUNDARY)
        with pytest.raises(ValueError, match="positive"):
            ft.rnnt_loss_tdt_mixed_pruned(x.to(dev), symd, rgd, blank, (0,), omega, boundary=bdd)
        with pytest.raises(ValueError, match="fewer than one token column"):
            ft.rnnt_loss_tdt_mixed_pruned(x.to(dev)[..., :5].contiguous(), symd, rgd, 0, durs, omega, boundary=bdd)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ft.rnnt_loss_tdt_mixed(torch.zeros(B, T, S + 1, C + len(durs)), sym, blank, durs, 0.5)
