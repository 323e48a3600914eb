"""rnnt_loss_pruned_kd on the device: the transducer loss on the pruned band and the distillation loss of
rnnt_kd_loss_pruned from one pass over the student (include/ftr_kd_loss.h).

What is checked, and against what:
  values    `loss` and `kd` are torch.equal to rnnt_loss_pruned / rnnt_kd_loss_pruned on the same device tensors
  gradient  against g64 = a * g_loss64 + k * g_kd64 -- the float64 oracle (rnnt_oracle.rnnt_loss_pruned_grad, dtype=float64)
            and the float64 restatement of the distillation loss (tests/kd_restatement.py), both on the up-converted inputs --
            element by element under the rule of tests/test_gpu_lowp.py,
                |g - g64| <= u |g64| + a_sub + 1e-4 max|g64|,
            u = 0 / 2^-8 / 2^-11 for float32 / bfloat16 / float16 (one rounding into the storage type), a_sub = 2^-25 for float16
            (half its subnormal spacing), the last term the float32 budget of every gradient test here.  Derived, not measured.

Geometry (tests/kd_cases.py): B=2 T=12 S=5 s_range=3, utterance 1 ragged (t_end 9, s_end 3); its band climbs one row past
s_end, so there are invalid nodes by frame and by s > s_end -- and the latter are rows the transducer loss reads although
the distillation loss does not (the band recursion's shift constants average over them).  One case runs on the band of
tests/test_gpu_lowp.py (copied below), which stays inside s_end.  C crosses every kernel path: 8 (a partly filled wave), 36
(C % 4 == 0, one quad set), 37 (scalar path), 500 (c3's vocabulary), 520 (a ragged second quad), 2048 (the largest
register-resident row), 2056 (the two-pass kernel)."""
import contextlib
import gc
import importlib

import numpy as np
import pytest
import torch

import kd_cases as K
import kd_restatement as R

pytestmark = pytest.mark.gpu

DT = {"f32": (torch.float32, 0.0, 0.0), "bf16": (torch.bfloat16, 2.0 ** -8, 0.0), "fp16": (torch.float16, 2.0 ** -11, 2.0 ** -25)}
B, T, S, RR = K.B, K.T, K.S, K.R
# (C, blank is the last column?, student, teacher, mode, temperature, rnnt_type, delay_penalty, reduction): every value of every
# axis occurs, every C with at least one 16-bit pair
CASES = [
    (8, False, "f32", "f32", "full", 1.0, "regular", 0.0, "none"),
    (8, True, "bf16", "f32", "collapsed", 2.0, "modified", 0.1, "sum"),
    (36, True, "fp16", "bf16", "full", 1.0, "modified", 0.0, "mean"),
    (36, False, "f32", "f32", "collapsed", 1.0, "regular", 0.1, "none"),
    (37, False, "bf16", "bf16", "full", 2.0, "regular", 0.1, "sum"),
    (37, True, "f32", "f32", "collapsed", 2.0, "modified", 0.0, "mean"),
    (500, True, "bf16", "f32", "full", 1.0, "regular", 0.0, "mean"),
    (500, False, "f32", "f32", "full", 2.0, "modified", 0.1, "none"),
    (500, True, "fp16", "bf16", "collapsed", 1.0, "regular", 0.0, "sum"),
    (520, False, "bf16", "bf16", "collapsed", 2.0, "regular", 0.0, "none"),
    (520, True, "f32", "f32", "full", 1.0, "modified", 0.1, "sum"),
    (2048, False, "fp16", "bf16", "full", 1.0, "regular", 0.1, "mean"),
    (2048, True, "f32", "f32", "collapsed", 2.0, "modified", 0.0, "none"),
    (2056, True, "bf16", "f32", "full", 2.0, "modified", 0.0, "sum"),
    (2056, False, "bf16", "bf16", "collapsed", 1.0, "regular", 0.1, "mean"),
    (2056, False, "f32", "f32", "full", 1.0, "regular", 0.0, "none"),
]
IDS = ["-".join(str(v) for v in c) for c in CASES]
# upstream weights (a, k) of (a * loss + k * kd).sum(); the last pair weighs the utterances one by one (reduction "none")
WEIGHTS = [(1.0, 0.5), (1.0, 0.0), (0.0, 1.0), (np.array([1.0, 0.5]), np.array([0.25, 2.0]))]


@pytest.fixture(autouse=True)
def _route_unset(monkeypatch):
    monkeypatch.delenv("FTR_PRUNED_ROUTE", raising=False)
    monkeypatch.delenv("FTR_BAND_IMPL", raising=False)


def band_ranges_inside():
    """band_ranges() of tests/test_gpu_lowp.py: ranges[b,t,0] climbs from 0 to s_end + 1 - r, so no band row lies past s_end"""
    rg = np.zeros((B, T, RR), np.int32)
    for b in range(B):
        top, te = max(int(K.BOUNDARY[b, 2]) + 1 - RR, 0), int(K.BOUNDARY[b, 3])
        s0 = np.minimum((np.arange(T) * top + te - 2) // max(te - 1, 1), top)
        rg[b] = s0[:, None] + np.arange(RR)[None, :]
    return rg


def no_band_ranges():
    """K.band_ranges() with one step backwards inside utterance 0: every row still inside the lattice, but not a band"""
    rg = K.band_ranges().copy()
    t = int(np.argmax(rg[0, :, 0] > 0))          # the first frame whose band has moved up
    rg[0, t + 1] = rg[0, t] - 1
    assert rg.min() >= 0 and (np.diff(rg[0, :, 0]) < 0).any()
    return rg


_INPUTS, _REF_LOSS, _REF_KD = {}, {}, {}


def inputs(C, collapsed, blank_last, sdt, tdt):
    """(student, teacher, symbols, blank): cpu tensors rounded to the dtypes; cached, never modified"""
    key = (C, collapsed, blank_last, sdt, tdt)
    if key not in _INPUTS:
        x, y, sym, blank = K.logits_pair(C, blank_last, collapsed)
        _INPUTS[key] = (torch.from_numpy(x).to(DT[sdt][0]), torch.from_numpy(y).to(DT[tdt][0]), sym, blank)
    return _INPUTS[key]


def ref_loss_grad(oracle, x, sym, blank, rg, rnnt_type, penalty, key):
    """d sum_b loss_b / d x of the transducer loss, recursion in float64; computed once per key"""
    if key not in _REF_LOSS:
        _, g = oracle.rnnt_loss_pruned_grad(x.float().numpy(), sym, rg, blank, K.BOUNDARY, rnnt_type, delay_penalty=penalty,
                                            reduction="sum", dtype=np.float64)
        _REF_LOSS[key] = np.asarray(g, np.float64)
    return _REF_LOSS[key]


def ref_kd_grad(x, y, sym, blank, rg, mode, tau, key):
    if key not in _REF_KD:
        _REF_KD[key] = R.kd_loss_and_grad(x.float().numpy(), y.float().numpy(), sym, rg, blank, K.BOUNDARY, mode, tau)[1]
    return _REF_KD[key]


def _dev(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _weigh(v, w, dev):
    return v * (torch.tensor(w, dtype=torch.float32, device=dev) if isinstance(w, np.ndarray) else w)


def run_new(ft, dev, x, y, sym, rg, blank, mode, tau, rnnt_type, penalty, reduction, w=None, boundary=K.BOUNDARY):
    """(loss, kd, d (a * loss + k * kd).sum() / d x) of the new function for device tensors x, y (x is made a leaf here)"""
    x = x.detach().requires_grad_(True)
    symd, rgd, bdd = _dev(dev, sym, rg, boundary)
    loss, kd = ft.rnnt_loss_pruned_kd(x, y, symd, rgd, blank, bdd, mode=mode, temperature=tau, rnnt_type=rnnt_type,
                                      delay_penalty=penalty, reduction=reduction)
    if w is not None:
        (_weigh(loss, w[0], dev) + _weigh(kd, w[1], dev)).sum().backward()
    return loss.detach(), kd.detach(), x.grad


def run_two(ft, dev, x, y, sym, rg, blank, mode, tau, rnnt_type, penalty, reduction, w=None, boundary=K.BOUNDARY):
    """the same from the two existing functions"""
    x = x.detach().requires_grad_(True)
    symd, rgd, bdd = _dev(dev, sym, rg, boundary)
    loss = ft.rnnt_loss_pruned(x, symd, rgd, blank, bdd, rnnt_type=rnnt_type, delay_penalty=penalty, reduction=reduction)
    kd = ft.rnnt_kd_loss_pruned(x, y, symd, rgd, blank, bdd, mode=mode, temperature=tau, reduction=reduction)
    if w is not None:
        (_weigh(loss, w[0], dev) + _weigh(kd, w[1], dev)).sum().backward()
    return loss.detach(), kd.detach(), x.grad


def grad_bound(g64, sdt):
    _, u, a = DT[sdt]
    return u * np.abs(g64) + a + 1e-4 * np.abs(g64).max()


def check_grad(g, g64, sdt, what, rg=None):
    g = g.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all(), what
    worst = float((np.abs(g - g64) / grad_bound(g64, sdt)).max())
    print(f"{what}: max |g - g64| / bound = {worst:.3g}, max |g64| = {np.abs(g64).max():.3g}")
    assert worst <= 1.0, f"{what}: gradient error is {worst:.3g} x its bound"
    te = int(K.BOUNDARY[1, 3])
    assert (g64[1, te:] == 0).all() and (g[1, te:] == 0).all(), f"{what}: gradient in the frames from t_end on"
    if rg is not None:
        assert (g[~R.valid_nodes(rg, K.BOUNDARY, S)] == 0).all(), f"{what}: gradient in the row of an invalid node"


def combined(gl, gk, w, reduction):
    """a * g_loss64 + k * g_kd64 for the upstream weights w under `reduction` (gl, gk: gradients of the per-utterance sums)"""
    a, k = (np.asarray(v, np.float64).reshape(-1, 1, 1, 1) if isinstance(v, np.ndarray) else float(v) for v in w)
    scale = 1.0 / B if reduction == "mean" else 1.0
    return scale * (a * gl + k * gk)


# ---- 1. values

@pytest.mark.parametrize("C,blank_last,sdt,tdt,mode,tau,rnnt_type,penalty,reduction", CASES, ids=IDS)
def test_values_are_those_of_the_two_functions(ft, dev, C, blank_last, sdt, tdt, mode, tau, rnnt_type, penalty, reduction):
    x, y, sym, blank = inputs(C, mode == "collapsed", blank_last, sdt, tdt)
    rg = K.band_ranges()
    for red in dict.fromkeys((reduction, "none", "sum", "mean")):
        loss, kd, _ = run_new(ft, dev, x.to(dev), y.to(dev), sym, rg, blank, mode, tau, rnnt_type, penalty, red)
        loss2, kd2, _ = run_two(ft, dev, x.to(dev), y.to(dev), sym, rg, blank, mode, tau, rnnt_type, penalty, red)
        print(f"{red}: loss {loss.tolist()} / {loss2.tolist()}, kd {kd.tolist()} / {kd2.tolist()}")
        assert loss.dtype == torch.float32 and kd.dtype == torch.float32 and loss.shape == loss2.shape and kd.shape == kd2.shape
        assert torch.isfinite(loss).all() and torch.isfinite(kd).all()
        assert torch.equal(loss, loss2), f"loss, reduction {red}"
        assert torch.equal(kd, kd2), f"kd, reduction {red}"


def test_values_on_a_band_inside_s_end(ft, dev):
    x, y, sym, blank = inputs(500, False, True, "bf16", "f32")
    rg = band_ranges_inside()
    a = run_new(ft, dev, x.to(dev), y.to(dev), sym, rg, blank, "full", 1.0, "regular", 0.0, "none")
    b = run_two(ft, dev, x.to(dev), y.to(dev), sym, rg, blank, "full", 1.0, "regular", 0.0, "none")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 2. gradient

@pytest.mark.parametrize("C,blank_last,sdt,tdt,mode,tau,rnnt_type,penalty,reduction", CASES, ids=IDS)
def test_gradient(ft, dev, oracle, C, blank_last, sdt, tdt, mode, tau, rnnt_type, penalty, reduction):
    coll = mode == "collapsed"
    x, y, sym, blank = inputs(C, coll, blank_last, sdt, tdt)
    rg = K.band_ranges()
    gl = ref_loss_grad(oracle, x, sym, blank, rg, rnnt_type, penalty, (C, coll, blank_last, sdt, rnnt_type, penalty))
    gk = ref_kd_grad(x, y, sym, blank, rg, mode, tau, (C, mode, blank_last, tau, sdt, tdt))
    xd, yd = x.to(dev), y.to(dev)
    args = (sym, rg, blank, mode, tau, rnnt_type, penalty)
    for w in WEIGHTS:
        red = "none" if isinstance(w[0], np.ndarray) else reduction
        what = f"C={C} {sdt}/{tdt} {mode} tau={tau} {rnnt_type} pen={penalty} {red} w={w}"
        g = run_new(ft, dev, xd, yd, *args, red, w=w)[2]
        assert g.dtype == x.dtype and g.shape == x.shape
        g64 = combined(gl, gk, w, red)
        check_grad(g, g64, sdt, what, rg)
        if isinstance(w[0], float) and 0.0 in w:          # one part alone: the single op's own gradient, within the same bound
            own = run_two(ft, dev, xd, yd, *args, red, w=w)[2].float().cpu().numpy().astype(np.float64)
            diff = np.abs(g.float().cpu().numpy().astype(np.float64) - own)
            assert (diff <= grad_bound(g64, sdt)).all(), f"{what}: against the single op's gradient"


@pytest.mark.parametrize("sdt,tdt,mode", [("f32", "f32", "full"), ("bf16", "f32", "collapsed"), ("fp16", "bf16", "full")])
def test_a_part_without_an_upstream_gradient_is_the_single_op(ft, dev, sdt, tdt, mode):
    """loss.backward() alone and kd.backward() alone: the other part arrives as None, is not read, and the row is the single
    op's row bit for bit (the same float32 operations in the same order, one rounding)."""
    x, y, sym, blank = inputs(500, mode == "collapsed", True, sdt, tdt)
    symd, rgd, bdd = _dev(dev, sym, K.band_ranges(), K.BOUNDARY)
    for which in (0, 1):
        xa = x.to(dev).requires_grad_(True)
        out = ft.rnnt_loss_pruned_kd(xa, y.to(dev), symd, rgd, blank, bdd, mode=mode, temperature=2.0, reduction="sum")
        out[which].backward()
        xb = x.to(dev).requires_grad_(True)
        if which == 0:
            ft.rnnt_loss_pruned(xb, symd, rgd, blank, bdd, reduction="sum").backward()
        else:
            ft.rnnt_kd_loss_pruned(xb, y.to(dev), symd, rgd, blank, bdd, mode=mode, temperature=2.0, reduction="sum").backward()
        assert xa.grad.abs().max() > 0 and torch.equal(xa.grad, xb.grad), which


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("mode", ["full", "collapsed"])
def test_self_distillation_leaves_no_gradient(ft, dev, mode, dt):
    x, _, sym, blank = inputs(500, mode == "collapsed", True, dt, dt)
    _, kd, g = run_new(ft, dev, x.to(dev), x.to(dev).clone(), sym, K.band_ranges(), blank, mode, 2.0, "regular", 0.0, "sum", w=(0.0, 1.0))
    assert abs(kd.item()) <= 1e-5 and (g == 0).all()


# ---- 3. invalid nodes

@pytest.mark.parametrize("C,sdt,tdt,mode,rnnt_type", [(36, "f32", "f32", "full", "regular"), (500, "bf16", "fp16", "collapsed", "modified"),
                                                     (2056, "fp16", "bf16", "full", "regular")])
def test_rows_of_invalid_nodes_hold_nan(ft, dev, C, sdt, tdt, mode, rnnt_type):
    x, y, sym, blank = inputs(C, mode == "collapsed", False, sdt, tdt)
    rg = K.band_ranges()
    bad = torch.from_numpy(~R.valid_nodes(rg, K.BOUNDARY, S))
    xp, yp = x.clone(), y.clone()
    xp[bad] = float("nan")
    yp[bad] = float("nan")
    assert torch.isnan(xp[1, 10]).all() and torch.isnan(xp[1, 8, 2]).all() and torch.isnan(yp[1, 8, 2]).all()
    args = (sym, rg, blank, mode, 1.0, rnnt_type, 0.0, "none")
    loss, kd, g = run_new(ft, dev, xp.to(dev), yp.to(dev), *args, w=(1.0, 0.5))
    loss2, kd2, _ = run_two(ft, dev, xp.to(dev), yp.to(dev), *args)
    clean = run_new(ft, dev, x.to(dev), y.to(dev), *args, w=(1.0, 0.5))
    assert torch.isfinite(kd).all() and torch.equal(kd, kd2) and torch.equal(kd, clean[1])
    assert torch.allclose(loss, loss2, rtol=0.0, atol=0.0, equal_nan=True)       # equal, a NaN being equal to a NaN
    assert (g.cpu()[bad] == 0).all()


# ---- 4. alignment

@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("mode", ["full", "collapsed"])
@pytest.mark.parametrize("which", ["student", "teacher"])
def test_tensor_at_an_odd_element(ft, dev, oracle, which, mode, dt):
    """A contiguous 16-bit tensor whose storage starts at an odd element (2-byte aligned only: no 8-byte access may be made).
    The values are those of the two functions on the same views, bit for bit -- for an odd teacher next to an aligned student
    too, where the student's logsumexp keeps the order of the loss's own pass -- and those of the aligned tensors up to the
    order of the row sums: 1e-4 relative, the project's float32 tolerance."""
    coll = mode == "collapsed"
    x, y, sym, blank = inputs(500, coll, True, dt, dt)
    rg = K.band_ranges()
    n = x.numel()
    buf = torch.zeros(n + 9, dtype=x.dtype, device=dev)
    off = buf[1:1 + n].view(x.shape)
    off.copy_(x if which == "student" else y)
    assert off.is_contiguous() and off.data_ptr() % 4 == 2
    xd, yd = (off, y.to(dev)) if which == "student" else (x.to(dev), off)
    args = (sym, rg, blank, mode, 1.0, "regular", 0.0, "sum")
    loss, kd, g = run_new(ft, dev, xd, yd, *args, w=(1.0, 0.5))
    loss2, kd2, _ = run_two(ft, dev, xd, yd, *args)
    assert torch.equal(loss, loss2) and torch.equal(kd, kd2)
    al = run_new(ft, dev, x.to(dev), y.to(dev), *args, w=(1.0, 0.5))
    assert abs(loss.item() - al[0].item()) <= 1e-4 * abs(al[0].item()) and abs(kd.item() - al[1].item()) <= 1e-4 * abs(al[1].item())
    gl = ref_loss_grad(oracle, x, sym, blank, rg, "regular", 0.0, (500, coll, True, dt, "regular", 0.0))
    gk = ref_kd_grad(x, y, sym, blank, rg, mode, 1.0, (500, mode, True, 1.0, dt, dt))
    check_grad(g, combined(gl, gk, (1.0, 0.5), "sum"), dt, f"odd {which} {mode} {dt}", rg)
    assert float(buf[0]) == 0 and (buf[1 + n:] == 0).all()     # the neighbours are untouched
    assert torch.equal(off, (x if which == "student" else y).to(dev))


# ---- 5. routes

@pytest.mark.parametrize("route", ["lattice", "no_band", "constrained"])
@pytest.mark.parametrize("sdt,tdt,mode", [("f32", "f32", "full"), ("f32", "f32", "collapsed"), ("bf16", "f32", "collapsed")])
def test_other_routes_are_the_composition(ft, dev, oracle, route, sdt, tdt, mode, monkeypatch):
    """FTR_PRUNED_ROUTE=lattice, ranges that are no band, and "constrained": the two functions are called, so values and
    gradient are theirs bit for bit.  Against g64 the float32 cases keep the rule of this file.  A 16-bit student cannot: the
    composition rounds each part into the storage type and autograd rounds their sum, three roundings where the rule allows
    one (the lattice route with bfloat16 came out at 1.53 x that bound when this test was written), so its bound is the one
    three roundings give: u (|a g_loss64| + |k g_kd64| + |g64|) in place of u |g64|, the other terms as they are."""
    coll = mode == "collapsed"
    x, y, sym, blank = inputs(36, coll, True, sdt, tdt)
    rg = no_band_ranges() if route == "no_band" else K.band_ranges()
    rnnt_type = "constrained" if route == "constrained" else "regular"
    if route == "lattice":
        monkeypatch.setenv("FTR_PRUNED_ROUTE", "lattice")
    calls = []
    ft._lib.set_profile_hook(lambda name: calls.append(name) or contextlib.nullcontext())
    try:
        args = (sym, rg, blank, mode, 2.0, rnnt_type, 0.0, "sum")
        loss, kd, g = run_new(ft, dev, x.to(dev), y.to(dev), *args, w=(1.0, 0.5))
    finally:
        ft._lib.set_profile_hook(None)
    assert not [c for c in calls if "band_kd" in c], calls
    loss2, kd2, g2 = run_two(ft, dev, x.to(dev), y.to(dev), *args, w=(1.0, 0.5))
    assert torch.equal(loss, loss2) and torch.equal(kd, kd2) and torch.equal(g, g2)
    gl = ref_loss_grad(oracle, x, sym, blank, rg, rnnt_type, 0.0, (36, coll, True, sdt, rnnt_type, 0.0, route))
    gk = ref_kd_grad(x, y, sym, blank, rg, mode, 2.0, (36, mode, True, 2.0, sdt, tdt, route))
    g64 = combined(gl, gk, (1.0, 0.5), "sum")
    what = f"{route} {sdt}/{tdt} {mode}"
    if sdt == "f32":
        check_grad(g, g64, sdt, what, rg)
    else:
        _, u, a = DT[sdt]
        gnp = g.float().cpu().numpy().astype(np.float64)
        bound = u * (np.abs(gl) + np.abs(0.5 * gk) + np.abs(g64)) + 3 * a + 1e-4 * np.abs(g64).max()
        worst = float((np.abs(gnp - g64) / bound).max())
        print(f"{what}: max |g - g64| / three-rounding bound = {worst:.3g}")
        assert np.isfinite(gnp).all() and worst <= 1.0, f"{what}: gradient error is {worst:.3g} x its bound"
        assert (gnp[~R.valid_nodes(rg, K.BOUNDARY, S)] == 0).all(), what


def test_the_band_route_is_the_fused_one(ft, dev):
    x, y, sym, blank = inputs(36, False, True, "f32", "f32")
    calls = []
    ft._lib.set_profile_hook(lambda name: calls.append(name) or contextlib.nullcontext())
    try:
        run_new(ft, dev, x.to(dev), y.to(dev), sym, K.band_ranges(), blank, "full", 1.0, "modified", 0.0, "mean", w=(1.0, 0.5))
    finally:
        ft._lib.set_profile_hook(None)
    calls = [c for c in calls if c != "ftr_band_ranges_check_i32"]
    assert calls == ["ftr_pruned_band_kd_fwd_dt", "ftr_mutual_information_band_ws_f32", "ftr_pruned_kd_reduce_f32",
                     "ftr_negated_reduce_f32", "ftr_pruned_band_kd_bwd_scaled_dt"], calls


# ---- 6. determinism and capture

def _capture(step):
    """_capture() of tests/test_gpu_graph.py: warm-up on a side stream, then one captured step"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):          # warm-up outside the capture: allocator pools
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    torch.cuda.synchronize()
    return g, out


@pytest.mark.parametrize("sdt,tdt,mode", [("f32", "f32", "full"), ("fp16", "bf16", "collapsed")])
def test_two_runs_are_bit_identical(ft, dev, sdt, tdt, mode):
    x, y, sym, blank = inputs(500, mode == "collapsed", True, sdt, tdt)
    args = (sym, K.band_ranges(), blank, mode, 1.0, "regular", 0.1, "mean")
    a = run_new(ft, dev, x.to(dev), y.to(dev), *args, w=(1.0, 0.5))
    b = run_new(ft, dev, x.to(dev), y.to(dev), *args, w=(1.0, 0.5))
    assert all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("sdt,tdt,mode", [("f32", "f32", "full"), ("bf16", "f32", "collapsed")])
def test_a_captured_step_replays_with_new_values(ft, dev, sdt, tdt, mode):
    """Forward + backward on a marked band captured once; three replays with other input contents give the eager results bit
    for bit (the second and third are what a graph with a memset or memcpy node gets wrong here)."""
    C = 500
    x0, y0, sym, blank = inputs(C, mode == "collapsed", True, sdt, tdt)
    xbuf, ybuf = x0.to(dev).clone(), y0.to(dev).clone()
    symd, rgd, bdd = _dev(dev, sym, K.band_ranges(), K.BOUNDARY)
    importlib.import_module("tf_fast_rnnt.rnnt_loss")._mark_band(rgd)     # (ft.rnnt_loss is the function of that name)

    def step():
        xx = xbuf.detach().requires_grad_(True)
        loss, kd = ft.rnnt_loss_pruned_kd(xx, ybuf, symd, rgd, blank, bdd, mode=mode, temperature=2.0, reduction="mean")
        (loss + 0.5 * kd).backward()
        return dict(loss=loss.detach(), kd=kd.detach(), grad=xx.grad)

    calls = []
    ft._lib.set_profile_hook(lambda name: calls.append(name) or contextlib.nullcontext())
    try:
        g, out = _capture(step)
    finally:
        ft._lib.set_profile_hook(None)
    assert calls.count("ftr_pruned_band_kd_bwd_scaled_dt") == 4, "the warm-up or the captured step left the fused route"
    for seed in (21, 22, 23):
        fx, fy, _, _ = K.logits_pair(C, True, mode == "collapsed", seed=seed)
        xbuf.copy_(torch.from_numpy(fx).to(dev))          # new values, same buffers
        ybuf.copy_(torch.from_numpy(fy).to(dev))
        g.replay()
        torch.cuda.synchronize()
        got = {k: v.clone() for k, v in out.items()}
        ref = step()
        torch.cuda.synchronize()
        assert torch.isfinite(got["loss"]) and torch.isfinite(got["kd"]) and got["grad"].abs().max() > 0
        for k in got:
            assert torch.equal(got[k], ref[k]), (seed, k)


# ---- 7. unchanged neighbours

def test_the_two_functions_are_untouched_by_calls_of_the_new_one(ft, dev):
    """The same float32 calls of rnnt_loss_pruned and rnnt_kd_loss_pruned before and after calls of the new function on other
    dtypes, in one process: bit-identical losses and gradients."""
    x, y, sym, blank = inputs(500, False, True, "f32", "f32")
    xd, yd = x.to(dev) * 1.37, y.to(dev) * 1.37       # not representable in 16 bits
    args = (sym, K.band_ranges(), blank, "full", 2.0, "regular", 0.0, "sum")
    before = [run_two(ft, dev, xd, yd, *args, w=w) for w in ((1.0, 0.0), (0.0, 1.0))]
    for sdt, tdt in (("bf16", "f32"), ("fp16", "bf16"), ("f32", "f32")):
        xs, ys, _, _ = inputs(500, False, True, sdt, tdt)
        run_new(ft, dev, xs.to(dev), ys.to(dev), *args, w=(1.0, 0.5))
    after = [run_two(ft, dev, xd, yd, *args, w=w) for w in ((1.0, 0.0), (0.0, 1.0))]
    for a, b in zip(before, after):
        assert a[2].dtype == torch.float32 and all(torch.equal(u, v) for u, v in zip(a, b))


# ---- a tensor past 2^31 elements

def test_logits_past_2_31_elements(ft, dev):
    """The scheme of tests/test_gpu_large.py: 2.26e9 student elements (B = 27, utterance 25 straddles element 2^31), the whole
    batch against the three-utterance batch of utterance 0, the straddler and the last one.  Utterances are independent, so
    the per-utterance values and their slices of the gradient must agree (normwise max|d| / max|ref| <= 1e-4, that file's
    tolerance); one 32-bit product in an index would make the big run read or write another utterance's rows.  float32
    student (a 16-bit gradient would turn a last-bit difference upstream into a whole rounding step), bfloat16 teacher."""
    Bn, Tn, Sn, r, C = 27, 8192, 24, 5, 2048
    per = Tn * r * C
    k = (1 << 31) // per
    idx = [0, k, Bn - 1]
    assert 0 < k < Bn - 1 and k * per < (1 << 31) < (k + 1) * per
    need = (4 + 4 + 2) * Bn * per + 3 * (4 + 4 + 2) * per
    free, total = torch.cuda.mem_get_info(dev)
    if free < need + (4 << 30):
        pytest.skip(f"needs {need / 2 ** 30:.1f} GiB + 4 GiB headroom, device reports {free / 2 ** 30:.1f} GiB free")
    g = torch.Generator(device=dev).manual_seed(31)
    sym = torch.randint(1, C - 1, (Bn, Sn), generator=g, device=dev, dtype=torch.int32)
    bd = torch.zeros((Bn, 4), dtype=torch.int32, device=dev)
    bd[:, 2] = torch.randint(Sn // 2, Sn + 1, (Bn,), generator=g, device=dev, dtype=torch.int32)
    bd[:, 3] = torch.randint(Tn // 2, Tn + 1, (Bn,), generator=g, device=dev, dtype=torch.int32)
    bd[0, 2], bd[0, 3] = Sn, Tn
    am = torch.randn((Bn, Tn, 16), generator=g, device=dev)
    lm = torch.randn((Bn, Sn + 1, 16), generator=g, device=dev)
    _, (gx, gy) = ft.rnnt_loss_simple(lm, am, sym % 15, 15, boundary=bd, reduction="sum", calc_gradients=True)
    ranges = ft.get_rnnt_prune_ranges(gx, gy, bd, r)
    w = torch.rand((Bn,), generator=g, device=dev) + 0.5
    x = torch.empty((Bn, Tn, r, C), dtype=torch.float32, device=dev)
    y = torch.empty((Bn, Tn, r, C), dtype=torch.bfloat16, device=dev)
    for b in range(Bn):                 # utterance by utterance: the generator kernels stay far below 2^31 themselves
        x[b].normal_(0.0, 2.0, generator=g)
        y[b].copy_(torch.randn((Tn, r, C), generator=g, device=dev) * 2.0)
    assert x.numel() > (1 << 31)

    def run(xx, yy, sel):
        xx = xx.requires_grad_(True)
        loss, kd = ft.rnnt_loss_pruned_kd(xx, yy, sym[sel], ranges[sel].contiguous(), 0, bd[sel], delay_penalty=0.05, reduction="none")
        ((loss + 0.5 * kd) * w[sel]).sum().backward()
        return loss.detach(), kd.detach(), xx.grad

    every = torch.arange(Bn, device=dev)
    pick = torch.tensor(idx, device=dev)
    big = run(x, y, every)
    small = run(torch.stack([x.detach()[i] for i in idx]), torch.stack([y[i] for i in idx]), pick)
    assert bool(torch.isfinite(big[0]).all()) and bool(torch.isfinite(big[1]).all()) and bool(torch.isfinite(big[2]).all())
    errs = {}
    for name, a, b in (("loss", big[0][pick], small[0]), ("kd", big[1][pick], small[1]),
                       ("grad", torch.stack([big[2][i] for i in idx]), small[2])):
        errs[name] = float((a - b).abs().max() / b.abs().max())
    print("past 2^31: big run vs three-utterance run:", ", ".join(f"{n} {e:.3g}" for n, e in errs.items()))
    assert all(e <= 1e-4 for e in errs.values()), errs
    del x, y, big, small
    gc.collect()
    torch.cuda.empty_cache()


# ---- 8. refusals

def test_refusals(ft, dev):
    x, y, sym, blank = inputs(36, False, True, "f32", "f32")
    symd, rgd, bdd = _dev(dev, sym, K.band_ranges(), K.BOUNDARY)
    xd, yd = x.to(dev), y.to(dev)
    f = ft.rnnt_loss_pruned_kd
    for bad_x, bad_y in ((xd.double(), yd), (xd, yd.double()), (xd.to(torch.int32), yd), (xd, yd.to(torch.int32))):
        with pytest.raises(TypeError):
            f(bad_x, bad_y, symd, rgd, blank, bdd)
    with pytest.raises(ValueError, match="shape"):
        f(xd, yd[..., :32].contiguous(), symd, rgd, blank, bdd)
    with pytest.raises(ValueError, match="mode"):
        f(xd, yd, symd, rgd, blank, bdd, mode="both")
    for tau in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            f(xd, yd, symd, rgd, blank, bdd, temperature=tau)
    with pytest.raises(ValueError, match="reduction"):
        f(xd, yd, symd, rgd, blank, bdd, reduction="max")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(x, y, torch.from_numpy(sym), torch.from_numpy(K.band_ranges()), blank, torch.from_numpy(K.BOUNDARY))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(xd, y, symd, rgd, blank, bdd)
