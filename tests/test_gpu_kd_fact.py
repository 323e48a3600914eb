"""rnnt_kd_loss_pruned_factored on the device: the softmax, HAT and TDT forms of the distillation loss and node weights,
against the float64 restatement of the definition (tests/kd_fact_restatement.py) on the up-converted values.

Geometry (tests/kd_fact_cases.py): B=2 T=6 S=4 r=3, boundary [[0,0,4,6],[0,0,2,4]]; utterance 1 has invalid nodes both by
frame and by s > s_end, and in every loss / gradient comparison here every invalid row of BOTH tensors is NaN.  Row widths W
(tdt: C = W - N token columns): 12 (register form, one quad per lane), 41 (element by element), 504 with N = 4 and 505 with
N = 5 (vector against element at c3's vocabulary), 2052 (the two-pass vector form); the hat and tdt forms also at 1000 and
1004 (four quads per lane, the register width of c4's vocabulary).  Inputs are standard normal x 3 rounded
to the dtype; in collapsed mode ln C is added to the blank and the correct-symbol columns of both tensors.

Tolerances, those of tests/test_gpu_kd.py, none measured from the code under test:
  loss      |err| <= 1e-4 |ref| + 1e-5 per utterance
  gradient  |g - g64| <= u |g64| + a + 1e-4 max|g64|, (u, a) = (0, 0) float32, (2^-8, 0) bfloat16, (2^-11, 2^-25) float16
With FTR_KD_FACT_PARITY_OUT set, the largest errors seen are written there as JSON when the module is done."""
import json
import os

import numpy as np
import pytest
import torch

import kd_fact_cases as K
import kd_fact_restatement as R
from kd_restatement import valid_nodes

pytestmark = pytest.mark.gpu

DT = {"f32": (torch.float32, 0.0, 0.0), "bf16": (torch.bfloat16, 2.0 ** -8, 0.0), "fp16": (torch.float16, 2.0 ** -11, 2.0 ** -25)}
PAIRS = [("f32", "f32"), ("bf16", "bf16"), ("fp16", "f32"), ("bf16", "fp16")]   # (student, teacher)
MODES = ["full", "collapsed"]
WIDTHS = [(12, 4), (41, 4), (504, 4), (505, 5), (2052, 4)]                        # (W, N of the tdt form)
FORMS = [(fact, W, N if fact == "tdt" else 0) for fact in K.FACTS for W, N in WIDTHS] + [("tdt", 1004, 4), ("hat", 1000, 0)]
MID = {"softmax": (504, 0), "hat": (504, 0), "tdt": (504, 4)}
# (tau, blank_last, duration_weight): each value of each of the three occurs
SETTINGS = [(1.0, False, 1.0), (2.0, True, 0.3)]
VALID = valid_nodes(K.band_ranges(), K.BOUNDARY, K.S)
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("FTR_KD_FACT_PARITY_OUT")
    if path and _WORST:
        with open(path, "w") as f:
            json.dump({k: _WORST[k] for k in sorted(_WORST)}, f, indent=1)
            f.write("\n")


def _note(key, **vals):
    rec = _WORST.setdefault(key, {})
    for k, v in vals.items():
        rec[k] = max(rec.get(k, 0.0), float(v))


_INPUTS, _REFS = {}, {}


def inputs(W, N, mode, blank_last, sdt, tdt):
    """(student, teacher, symbols, blank): cpu tensors rounded to the dtypes, every invalid row NaN; cached, never modified"""
    key = (W, N, mode == "collapsed", blank_last, sdt, tdt)
    if key not in _INPUTS:
        x, y, sym, blank = K.logits_pair(W, N, blank_last, mode == "collapsed")
        x[~VALID] = np.nan
        y[~VALID] = np.nan
        _INPUTS[key] = (torch.from_numpy(x).to(DT[sdt][0]), torch.from_numpy(y).to(DT[tdt][0]), sym, blank)
    return _INPUTS[key]


def case(fact, W, N, mode, blank_last, tau, dw, sdt, tdt, weights=None):
    """inputs() and the float64 reference (loss [B], gradient) on the up-converted values, computed once per key"""
    x, y, sym, blank = inputs(W, N, mode, blank_last, sdt, tdt)
    key = (fact, W, N, mode, blank_last, tau, dw, sdt, tdt, None if weights is None else weights.tobytes())
    if key not in _REFS:
        _REFS[key] = R.kd_fact_loss_and_grad(x.float().numpy(), y.float().numpy(), sym, K.band_ranges(), blank, K.BOUNDARY, fact, N,
                                             mode, tau, dw, weights)
    return (x, y, sym, blank) + _REFS[key]


def run(ft, dev, x, y, sym, blank, fact, N, mode, tau=1.0, dw=1.0, weights=None, reduction="none", upstream=None):
    """(loss, d (upstream . loss) / d x) for device tensors x, y (x is made a leaf here)"""
    x = x.detach().requires_grad_(True)
    y = y.detach().requires_grad_(True)
    if weights is not None:
        weights = torch.as_tensor(weights).to(dev).requires_grad_(True)
    loss = ft.rnnt_kd_loss_pruned_factored(x, y, torch.from_numpy(sym).to(dev), torch.from_numpy(K.band_ranges()).to(dev), blank,
                                           torch.from_numpy(K.BOUNDARY).to(dev), factorization=fact, num_durations=N, mode=mode,
                                           temperature=tau, duration_weight=dw, node_weights=weights, reduction=reduction)
    out = loss if upstream is None else loss * upstream
    out.sum().backward()
    assert y.grad is None and (weights is None or weights.grad is None)
    return loss.detach(), x.grad


def check_loss(loss, ref, what):
    got = loss.cpu().numpy().astype(np.float64)
    assert loss.dtype == torch.float32 and got.shape == ref.shape and np.isfinite(got).all(), what
    err = np.abs(got - ref)
    worst = float((err / (1e-4 * np.abs(ref) + 1e-5)).max())
    print(f"{what}: loss {got}, reference {ref}, |err| / bound = {worst:.3g}")
    assert worst <= 1.0, f"{what}: loss error is {worst:.3g} x its bound"
    return float((err / np.abs(ref)).max())


def check_grad(g, g64, sdt, what, zero=~VALID):
    _, u, a = DT[sdt]
    g = g.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all(), what
    bound = u * np.abs(g64) + a + 1e-4 * np.abs(g64).max()
    err = np.abs(g - g64)
    worst = float((err / bound).max())
    print(f"{what}: max |g - g64| / bound = {worst:.3g}, max |g64| = {np.abs(g64).max():.3g}")
    assert worst <= 1.0, f"{what}: gradient error is {worst:.3g} x its bound"
    assert (g[zero] == 0).all(), f"{what}: gradient in an invalid row"
    return worst, float(err.max() / np.abs(g64).max())


@pytest.mark.parametrize("sdt,tdt", PAIRS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fact,W,N", FORMS)
def test_loss_and_gradient(ft, dev, fact, W, N, mode, sdt, tdt):
    for tau, blank_last, dw in SETTINGS:
        x, y, sym, blank, ref, g64 = case(fact, W, N, mode, blank_last, tau, dw, sdt, tdt)
        what = f"{fact} W={W} N={N} {mode} blank={'last' if blank_last else 'first'} tau={tau} dw={dw} {sdt}/{tdt}"
        assert torch.isnan(x[1, 5]).all() and torch.isnan(y[1, 3, 2]).all()
        loss, g = run(ft, dev, x.to(dev), y.to(dev), sym, blank, fact, N, mode, tau, dw)
        rel = check_loss(loss, ref, what)
        assert g.dtype == x.dtype and g.shape == x.shape
        frac, gerr = check_grad(g, g64, sdt, what)
        _note(f"{fact} {mode} {sdt}/{tdt}", loss_rel_err=rel, grad_err_over_bound=frac, grad_err_over_max=gerr)


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("mode", MODES)
def test_softmax_without_weights_is_rnnt_kd_loss_pruned_bit_for_bit(ft, dev, mode, dt):
    for W in (41, 504, 2052):
        x, y, sym, blank = inputs(W, 0, mode, True, dt, dt)
        xd = x.to(dev).requires_grad_(True)
        for reduction in ("none", "mean"):
            old = ft.rnnt_kd_loss_pruned(xd, y.to(dev), torch.from_numpy(sym).to(dev), torch.from_numpy(K.band_ranges()).to(dev), blank,
                                         torch.from_numpy(K.BOUNDARY).to(dev), mode=mode, temperature=2.0, reduction=reduction)
            (g_old,) = torch.autograd.grad(old.sum(), xd)
            new, g_new = run(ft, dev, xd, y.to(dev), sym, blank, "softmax", 0, mode, 2.0, reduction=reduction)
            assert torch.isfinite(new).all() and torch.equal(old.detach(), new) and torch.equal(g_old, g_new)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W,N", [(12, 4), (41, 4), (504, 4), (2052, 4), (505, 5)])
def test_tdt_with_duration_weight_zero(ft, dev, W, N, mode, dt):
    """The token head alone: exact zeros in the duration columns, whose values do not matter (they hold NaN here), and the loss and
    token-column gradients of the softmax form on a tensor holding those columns -- bit for bit where both tensors put a
    column on the same lane in the same order (a row of C and a row of C + N both read four at a time, or both element by
    element: every width here but 505, whose C = 500 columns alone are read four at a time), within the tolerances there."""
    x, y, sym, blank = inputs(W, N, mode, False, dt, dt)
    C = W - N
    xn = x.clone()
    xn[..., C:] = float("nan")
    loss, g = run(ft, dev, xn.to(dev), y.to(dev), sym, blank, "tdt", N, mode, 2.0, 0.0)
    ls, gs = run(ft, dev, x[..., :C].contiguous().to(dev), y[..., :C].contiguous().to(dev), sym, blank, "softmax", 0, mode, 2.0)
    assert torch.isfinite(loss).all() and (g[..., C:] == 0).all() and (g[..., :C][torch.from_numpy(VALID).to(dev)] != 0).any()
    if W != 505:
        assert torch.equal(loss, ls) and torch.equal(g[..., :C], gs)
    else:
        ref, g64 = R.kd_fact_loss_and_grad(x.float().numpy(), y.float().numpy(), sym, K.band_ranges(), blank, K.BOUNDARY, "tdt", N,
                                           mode, 2.0, 0.0)
        check_loss(loss, ref, f"tdt dw=0 W=505 {mode} {dt}")
        check_grad(g, g64, dt, f"tdt dw=0 W=505 {mode} {dt}")


@pytest.mark.parametrize("sdt,tdt", [("f32", "f32"), ("bf16", "fp16")])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fact", K.FACTS)
def test_node_weights(ft, dev, fact, mode, sdt, tdt):
    """Random weights scale node losses and gradient rows; rows of weight exactly 0 are never read (they hold NaN here, as
    the invalid rows do) and come back as zeros; a NaN weight on a valid node makes its utterance NaN, and only that one."""
    for (W, N) in (MID[fact], (41, 4 if fact == "tdt" else 0)):
        w = K.node_weights()
        x, y, sym, blank, ref, g64 = case(fact, W, N, mode, True, 2.0, 0.3, sdt, tdt, weights=w)
        what = f"weights {fact} W={W} {mode} {sdt}/{tdt}"
        loss, g = run(ft, dev, x.to(dev), y.to(dev), sym, blank, fact, N, mode, 2.0, 0.3, weights=w)
        check_loss(loss, ref, what)
        frac, gerr = check_grad(g, g64, sdt, what)
        _note(f"{fact} {mode} {sdt}/{tdt} weighted", grad_err_over_bound=frac, grad_err_over_max=gerr)

        wz = K.node_weights(zeros=0.4)
        off = VALID & (wz == 0)
        assert off[0].any() and off[1].any() and (VALID & (wz != 0))[1].any()
        _, _, _, _, ref, g64 = case(fact, W, N, mode, True, 2.0, 0.3, sdt, tdt, weights=wz)
        clean = run(ft, dev, x.to(dev), y.to(dev), sym, blank, fact, N, mode, 2.0, 0.3, weights=wz)
        xp, yp = x.clone(), y.clone()
        xp[torch.from_numpy(off)] = float("nan")
        yp[torch.from_numpy(off)] = float("nan")
        poisoned = run(ft, dev, xp.to(dev), yp.to(dev), sym, blank, fact, N, mode, 2.0, 0.3, weights=wz)
        check_loss(poisoned[0], ref, what + " zeros")
        check_grad(poisoned[1], g64, sdt, what + " zeros", zero=~VALID | (wz == 0))
        assert torch.equal(clean[0], poisoned[0]) and torch.equal(clean[1], poisoned[1])

        wn = w.copy()
        wn[0, 2, 1] = np.nan
        assert VALID[0, 2, 1]
        ln, _ = run(ft, dev, x.to(dev), y.to(dev), sym, blank, fact, N, mode, 2.0, 0.3, weights=wn)
        assert torch.isnan(ln[0]) and ln[1] == loss[1]


@pytest.mark.parametrize("sdt,tdt", [("f32", "f32"), ("bf16", "f32")])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fact", K.FACTS)
def test_reductions_and_upstream_gradient(ft, dev, fact, mode, sdt, tdt):
    """"sum" and "mean" are the reductions of "none" (mean: over B of the per-utterance sums), to float32 rounding, and the
    upstream gradient -- a scalar, or one value per utterance -- is folded into the gradient."""
    W, N = MID[fact]
    w = K.node_weights(seed=78)
    x, y, sym, blank, ref, g64 = case(fact, W, N, mode, False, 2.0, 0.3, sdt, tdt, weights=w)
    args = (x.to(dev), y.to(dev), sym, blank, fact, N, mode, 2.0, 0.3, w)
    none, _ = run(ft, dev, *args)
    for reduction, want, scale in (("sum", none.double().sum().item(), 1.0), ("mean", none.double().mean().item(), 1.0 / K.B)):
        loss, g = run(ft, dev, *args, reduction=reduction)
        assert loss.shape == () and loss.dtype == torch.float32
        assert abs(loss.item() - want) <= 4 * 2.0 ** -24 * abs(want)          # B = 2 addends, one division: a few ulp
        check_grad(g, g64 * scale, sdt, f"{reduction} {fact} {mode} {sdt}/{tdt}")
        _, g = run(ft, dev, *args, reduction=reduction, upstream=2.5)
        check_grad(g, g64 * scale * 2.5, sdt, f"2.5 x {reduction} {fact} {mode} {sdt}/{tdt}")
    up = np.array([0.75, -1.5])
    _, g = run(ft, dev, *args, upstream=torch.tensor(up, dtype=torch.float32, device=dev))
    check_grad(g, g64 * up[:, None, None, None], sdt, f"per-utterance upstream {fact} {mode} {sdt}/{tdt}")


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fact", K.FACTS)
def test_self_distillation(ft, dev, fact, mode, dt):
    """Teacher = student (the same values): no loss, and a gradient within check_grad's rule of the zero reference --
    u |0| + a + 1e-4 max|0| = a, which is exact zeros for float32 and bfloat16."""
    for W, N in (MID[fact], (41, 4 if fact == "tdt" else 0), (2052, 4 if fact == "tdt" else 0)):
        x, _, sym, blank = inputs(W, N, mode, True, dt, dt)
        x = torch.nan_to_num(x, nan=0.5)            # the NaN rows are invalid either way; here they are simply equal
        loss, g = run(ft, dev, x.to(dev), x.to(dev).clone(), sym, blank, fact, N, mode, 2.0, 0.3, weights=K.node_weights())
        assert (loss.abs() <= 1e-5).all(), loss
        worst = np.abs(g.float().cpu().numpy()).max()
        print(f"self-distillation {fact} W={W} {mode} {dt}: loss {loss.tolist()}, max |g| = {worst:.3g}")
        assert worst <= DT[dt][2]


@pytest.mark.parametrize("sdt,tdt", [("f32", "f32"), ("fp16", "bf16")])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fact", K.FACTS)
def test_two_runs_are_bit_identical(ft, dev, fact, mode, sdt, tdt):
    W, N = MID[fact]
    x, y, sym, blank = inputs(W, N, mode, True, sdt, tdt)
    for reduction in ("none", "mean"):
        a = run(ft, dev, x.to(dev), y.to(dev), sym, blank, fact, N, mode, 1.0, 0.3, K.node_weights(), reduction=reduction)
        b = run(ft, dev, x.to(dev), y.to(dev), sym, blank, fact, N, mode, 1.0, 0.3, K.node_weights(), reduction=reduction)
        assert torch.isfinite(a[0]).all() and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fact", K.FACTS)
def test_tensor_at_an_odd_element(ft, dev, fact, mode, dt):
    """A contiguous 16-bit tensor whose storage starts at an odd element (2-byte aligned only: no 8-byte access may be made);
    the other tensor is aligned, so the row must run element by element for both."""
    W, N = MID[fact]
    x, y, sym, blank, ref, g64 = case(fact, W, N, mode, True, 1.0, 1.0, dt, dt)
    n = x.numel()
    for which in ("student", "teacher"):
        buf = torch.zeros(n + 9, dtype=x.dtype, device=dev)
        off = buf[1:1 + n].view(x.shape)
        off.copy_(x if which == "student" else y)
        assert off.is_contiguous() and off.data_ptr() % 4 == 2
        xd, yd = (off, y.to(dev)) if which == "student" else (x.to(dev), off)
        loss, g = run(ft, dev, xd, yd, sym, blank, fact, N, mode)
        check_loss(loss, ref, f"odd {which} {fact} {mode} {dt}")
        check_grad(g, g64, dt, f"odd {which} {fact} {mode} {dt}")
        assert float(buf[0]) == 0 and (buf[1 + n:] == 0).all()     # the neighbours are untouched
        assert torch.equal(off.view(torch.int16), (x if which == "student" else y).to(dev).view(torch.int16))


@pytest.mark.parametrize("fact", K.FACTS)
def test_non_contiguous_inputs(ft, dev, fact):
    N = 4 if fact == "tdt" else 0
    x, y, sym, blank, ref, g64 = case(fact, 41, N, "full", True, 1.0, 1.0, "f32", "f32", weights=K.node_weights())
    big =torch.full((K.B, K.T, K.R, 41 + 5), 7.0, device=dev)
    big[..., :41] = x.to(dev)
    ty = y.to(dev).transpose(1, 2).contiguous().transpose(1, 2)
    w = torch.from_numpy(K.node_weights()).to(dev).transpose(0, 1).contiguous().transpose(0, 1)
    assert not big[..., :41].is_contiguous() and not ty.is_contiguous() and not w.is_contiguous()
    loss, g = run(ft, dev, big[..., :41], ty, sym, blank, fact, N, "full", weights=w)
    check_loss(loss, ref, f"slices {fact}")
    check_grad(g, g64, "f32", f"slices {fact}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fact", K.FACTS)
def test_replays_from_a_graph_with_new_values(ft, dev, fact, mode):
    """Forward + backward captured once on one stream; two replays with other input contents and weights give the eager
    results, bit for bit."""
    W, N = MID[fact]
    x0, y0, sym, blank = inputs(W, N, mode, True, "bf16", "f32")
    x = x0.to(dev).requires_grad_(True)
    y = y0.to(dev)
    w = torch.from_numpy(K.node_weights()).to(dev)
    symd, rg, bd = torch.from_numpy(sym).to(dev), torch.from_numpy(K.band_ranges()).to(dev), torch.from_numpy(K.BOUNDARY).to(dev)

    def step():
        loss = ft.rnnt_kd_loss_pruned_factored(x, y, symd, rg, blank, bd, factorization=fact, num_durations=N, mode=mode,
                                               duration_weight=0.3, node_weights=w, reduction="mean")
        (g,) = torch.autograd.grad(loss, x)
        return loss, g

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):          # warm-up outside the capture: allocator pools
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    torch.cuda.synchronize()
    for seed in (11, 12):
        fx, fy, _, _ = K.logits_pair(W, N, True, mode == "collapsed", seed=seed)
        with torch.no_grad():
            x.copy_(torch.from_numpy(fx))                 # new values, same buffers
            y.copy_(torch.from_numpy(fy))
            w.copy_(torch.from_numpy(K.node_weights(seed=seed, zeros=0.2)))
        graph.replay()
        torch.cuda.synchronize()
        got = [v.clone() for v in out]
        ref = step()
        torch.cuda.synchronize()
        assert torch.isfinite(got[0]) and got[0] > 0
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
