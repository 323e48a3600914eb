"""rnnt_loss_pruned_kd_factored and rnnt_node_occupancy_pruned on the device (include/ftr_kd_loss_fact.h): the transducer loss
on the pruned band -- ordinary or HAT -- and the factored distillation loss from one pass over the student, with node weights
that are a tensor or the student's own occupancies.

What is checked, and against what:
  values     `loss` torch.equal to rnnt_loss_pruned / hat_loss_pruned, `kd` torch.equal to rnnt_kd_loss_pruned_factored
  occupancy  against float64: the lattices of the oracle (softmax) or of tests/hat_restatement.py (HAT) + the delay penalty
             through the oracle's recursion in float64, gathered onto the band; 2e-4 absolute (two occupancies, each under the
             project's 1e-4).  `kd` with occupancy weights against sum occ64 * KL64 within 1e-4 kd64 + 2e-4 sum_valid KL64,
             which is what those two bounds give.
  gradient   against g64 = a * g_loss64 + k * g_kd64 under the rule of tests/test_gpu_kd_loss.py,
                 |g - g64| <= u |g64| + a_sub + 1e-4 max|g64|;
             g_loss64 from the float64 oracle, for HAT from the float64 autograd of tests/hat_restatement.py; g_kd64 from
             tests/kd_fact_restatement.py with the weights.

Geometry: tests/kd_cases.py, B=2 T=12 S=5 s_range=3, utterance 1 ragged with a band that climbs past s_end.  C crosses every
kernel path: 8, 36, 37, 500, 520, 2048, 2056 (see tests/test_gpu_kd_loss.py)."""
import contextlib
import importlib

import numpy as np
import pytest
import torch

import hat_restatement as H
import kd_cases as K
import kd_fact_cases as F
import kd_fact_restatement as FR
import kd_restatement as R
from test_gpu_kd_loss import DT, WEIGHTS, _capture, _dev, _weigh, check_grad, combined, no_band_ranges

pytestmark = pytest.mark.gpu

B, T, S, RR = K.B, K.T, K.S, K.R
# (C, blank is the last column?, student, teacher, factorization, weights, mode, temperature, rnnt_type, delay_penalty, reduction)
CASES = [
    (8, False, "f32", "f32", "hat", "none", "full", 1.0, "regular", 0.0, "none"),
    (8, True, "bf16", "f32", "softmax", "tensor", "collapsed", 2.0, "modified", 0.1, "sum"),
    (36, True, "fp16", "bf16", "hat", "tensor", "full", 1.0, "modified", 0.0, "mean"),
    (36, False, "f32", "f32", "softmax", "tensor", "collapsed", 1.0, "regular", 0.1, "none"),
    (37, False, "bf16", "bf16", "hat", "none", "full", 2.0, "regular", 0.1, "sum"),
    (37, True, "f32", "f32", "hat", "tensor", "collapsed", 2.0, "modified", 0.0, "mean"),
    (500, True, "bf16", "f32", "hat", "none", "full", 1.0, "regular", 0.0, "mean"),
    (500, False, "f32", "f32", "softmax", "tensor", "full", 2.0, "modified", 0.1, "none"),
    (500, True, "fp16", "bf16", "hat", "tensor", "collapsed", 1.0, "regular", 0.0, "sum"),
    (520, False, "bf16", "bf16", "softmax", "tensor", "collapsed", 2.0, "regular", 0.0, "none"),
    (520, True, "f32", "f32", "hat", "none", "full", 1.0, "modified", 0.1, "sum"),
    (2048, False, "fp16", "bf16", "hat", "tensor", "full", 1.0, "regular", 0.1, "mean"),
    (2048, True, "f32", "f32", "softmax", "tensor", "collapsed", 2.0, "modified", 0.0, "none"),
    (2056, True, "bf16", "f32", "hat", "tensor", "full", 2.0, "modified", 0.0, "sum"),
    (2056, False, "bf16", "bf16", "softmax", "tensor", "collapsed", 1.0, "regular", 0.1, "mean"),
    (2056, False, "f32", "f32", "hat", "none", "collapsed", 1.0, "regular", 0.0, "none"),
]
# the occupancy cases: (C, student, teacher, factorization, mode, temperature, rnnt_type, delay_penalty)
OCC_CASES = [
    (8, "f32", "f32", "softmax", "full", 1.0, "regular", 0.0),
    (36, "bf16", "f32", "hat", "collapsed", 2.0, "modified", 0.1),
    (37, "fp16", "bf16", "softmax", "collapsed", 1.0, "modified", 0.0),
    (500, "f32", "f32", "hat", "full", 1.0, "regular", 0.1),
    (520, "bf16", "bf16", "softmax", "full", 2.0, "regular", 0.1),
    (2048, "fp16", "f32", "hat", "full", 2.0, "modified", 0.0),
    (2056, "bf16", "f32", "hat", "collapsed", 1.0, "regular", 0.0),
]


@pytest.fixture(autouse=True)
def _route_unset(monkeypatch):
    monkeypatch.delenv("FTR_PRUNED_ROUTE", raising=False)
    monkeypatch.delenv("FTR_BAND_IMPL", raising=False)


def tensor_weights():
    """float32 [B,T,r] in (0.25, 1.75), about a third exact zeros: kd_fact_cases.node_weights (T = 6 there) twice along T"""
    w = np.concatenate([F.node_weights(77, zeros=1.0 / 3.0), F.node_weights(78, zeros=1.0 / 3.0)], axis=1)
    assert w.shape == (B, T, RR) and 0.2 < (w == 0).mean() < 0.45
    valid = R.valid_nodes(K.band_ranges(), K.BOUNDARY, S)
    assert (w[valid] == 0).any() and (w[valid] != 0).any()
    return w


_INPUTS, _REF_LOSS, _REF_KD, _REF_OCC = {}, {}, {}, {}


def inputs(C, collapsed, blank_last, sdt, tdt):
    """(student, teacher, symbols, blank): cpu tensors rounded to the dtypes; cached, never modified"""
    key = (C, collapsed, blank_last, sdt, tdt)
    if key not in _INPUTS:
        x, y, sym, blank = K.logits_pair(C, blank_last, collapsed)
        _INPUTS[key] = (torch.from_numpy(x).to(DT[sdt][0]), torch.from_numpy(y).to(DT[tdt][0]), sym, blank)
    return _INPUTS[key]


def hat_lattices64(x, sym, blank, rg, rnnt_type, penalty, boundary=K.BOUNDARY):
    """(x64 leaf, px, py) of the HAT lattices in float64 with the delay penalty (tests/hat_restatement.py)"""
    from tf_fast_rnnt.rnnt_loss import _apply_delay_penalty
    x64 = x.float().double().requires_grad_(True)
    bd = torch.from_numpy(boundary)
    px, py = H.get_hat_logprobs_pruned_torch(x64, torch.from_numpy(sym), torch.from_numpy(rg), blank, bd, rnnt_type)
    return x64, _apply_delay_penalty(px, bd, rnnt_type, penalty), py


def ref_loss_grad(oracle, fact, x, sym, blank, rg, rnnt_type, penalty, key):
    """d sum_b loss_b / d x of the transducer loss in float64; computed once per key"""
    key = (fact,) + key
    if key not in _REF_LOSS:
        if fact == "hat":
            x64, px, py = hat_lattices64(x, sym, blank, rg, rnnt_type, penalty)
            H.lattice_loss_torch(px, py, K.BOUNDARY, rnnt_type).sum().backward()
            _REF_LOSS[key] = x64.grad.numpy().copy()
        else:
            _, g = oracle.rnnt_loss_pruned_grad(x.float().numpy(), sym, rg, blank, K.BOUNDARY, rnnt_type, delay_penalty=penalty,
                                                reduction="sum", dtype=np.float64)
            _REF_LOSS[key] = np.asarray(g, np.float64)
    return _REF_LOSS[key]


def ref_kd(fact, x, y, sym, blank, rg, mode, tau, w, key):
    """(loss [B], gradient) of the distillation loss in float64 with node weights w (None, or an array)"""
    key = (fact,) + key
    if key not in _REF_KD:
        _REF_KD[key] = FR.kd_fact_loss_and_grad(x.float().numpy(), y.float().numpy(), sym, rg, blank, K.BOUNDARY, fact, 0, mode, tau,
                                                node_weights=w)
    return _REF_KD[key]


def ref_occupancy(oracle, fact, x, sym, blank, rg, rnnt_type, penalty, key):
    """float64 node occupancies [B,T,r]: the lattices, the delay penalty, the oracle's recursion in float64, gathered"""
    key = (fact,) + key
    if key not in _REF_OCC:
        if fact == "hat":
            _, px, py = hat_lattices64(x, sym, blank, rg, rnnt_type, penalty)
            px, py = px.detach().numpy(), py.detach().numpy()
        else:
            px, py = oracle.get_rnnt_logprobs_pruned(x.float().numpy(), sym, rg, blank, K.BOUNDARY, rnnt_type)
            px = oracle._delay_penalty(px, K.BOUNDARY, rnnt_type, penalty)
        _, (gx, gy) = oracle.mutual_information_recursion(px, py, K.BOUNDARY, True, np.float64)
        gx, gy = np.asarray(gx, np.float64), np.asarray(gy, np.float64)
        occ = np.zeros((B, T, RR))
        valid = R.valid_nodes(rg, K.BOUNDARY, S)
        for b, t, k in zip(*np.nonzero(valid)):
            s = int(rg[b, t, k])
            occ[b, t, k] = (gx[b, s, t] if s < S else 0.0) + gy[b, s, t]
        _REF_OCC[key] = occ
    return _REF_OCC[key]


def _wts(dev, wk):
    """the node_weights argument for a kind: "none", "tensor", "occupancy", or an array / tensor as it is"""
    if isinstance(wk, str):
        return {"none": None, "occupancy": "occupancy"}[wk] if wk != "tensor" else torch.from_numpy(tensor_weights()).to(dev)
    return torch.as_tensor(wk).to(dev)


def run_new(ft, dev, x, y, sym, rg, blank, fact, wk, mode, tau, rnnt_type, penalty, reduction, w=None, boundary=K.BOUNDARY, part=None):
    """(loss, kd, d (a * loss + k * kd).sum() / d x) of the new function for device tensors x, y (x is made a leaf here).
    part = 0 / 1: loss.sum().backward() / kd.sum().backward() alone instead -- the other output gets NO upstream gradient (None
    reaches the node, not a zero tensor as with a weight of 0.0)"""
    x = x.detach().requires_grad_(True)
    symd, rgd, bdd = _dev(dev, sym, rg, boundary)
    loss, kd = ft.rnnt_loss_pruned_kd_factored(x, y, symd, rgd, blank, bdd, factorization=fact, mode=mode, temperature=tau,
                                               node_weights=_wts(dev, wk), rnnt_type=rnnt_type, delay_penalty=penalty,
                                               reduction=reduction)
    if part is not None:
        (loss, kd)[part].sum().backward()
    elif w is not None:
        (_weigh(loss, w[0], dev) + _weigh(kd, w[1], dev)).sum().backward()
    return loss.detach(), kd.detach(), x.grad


def run_two(ft, dev, x, y, sym, rg, blank, fact, wk, mode, tau, rnnt_type, penalty, reduction, w=None, boundary=K.BOUNDARY, part=None):
    """the same from the existing functions ("occupancy": the weights from rnnt_node_occupancy_pruned); part = 0 / 1: the
    gradient of that single function alone"""
    x = x.detach().requires_grad_(True)
    symd, rgd, bdd = _dev(dev, sym, rg, boundary)
    single = ft.hat_loss_pruned if fact == "hat" else ft.rnnt_loss_pruned
    loss = single(x, symd, rgd, blank, bdd, rnnt_type=rnnt_type, delay_penalty=penalty, reduction=reduction)
    wts = _wts(dev, wk)
    if isinstance(wts, str):
        wts = ft.rnnt_node_occupancy_pruned(x, symd, rgd, blank, bdd, factorization=fact, rnnt_type=rnnt_type, delay_penalty=penalty)
    kd = ft.rnnt_kd_loss_pruned_factored(x, y, symd, rgd, blank, bdd, factorization=fact, mode=mode, temperature=tau,
                                         node_weights=wts, reduction=reduction)
    if part is not None:
        (loss, kd)[part].sum().backward()
    elif w is not None:
        (_weigh(loss, w[0], dev) + _weigh(kd, w[1], dev)).sum().backward()
    return loss.detach(), kd.detach(), x.grad


# ---- 1. values

def _each(cases, check, *fixtures):
    """Every case through `check`, its name printed first; a failing case does not hide the ones after it: all of them run,
    and the test fails at the end with the name and the error of each that failed."""
    failed = []
    for case in cases:
        name = "-".join(str(v) for v in case)
        print("case", name)
        try:
            check(*fixtures, *case)
        except Exception as e:      # noqa: BLE001  (an AssertionError as a rule; anything else is reported the same way)
            failed.append(f"{check.__name__}[{name}]: {type(e).__name__}: {e}")
    assert not failed, "\n".join(failed)


def test_values_are_those_of_the_single_functions(ft, dev):
    _each(CASES, _values, ft, dev)
    _each([(500, "f32", "f32", "full"), (36, "bf16", "f32", "collapsed"), (2056, "fp16", "bf16", "full")],
          _softmax_without_weights_is_rnnt_loss_pruned_kd, ft, dev)
    _each([("hat", "none", 0), ("softmax", "tensor", 0), ("hat", "occupancy", 2)], _the_band_route_is_the_fused_one, ft, dev)


def _values(ft, dev, C, blank_last, sdt, tdt, fact, wk, mode, tau, rnnt_type, penalty, reduction):
    x, y, sym, blank = inputs(C, mode == "collapsed", blank_last, sdt, tdt)
    rg = K.band_ranges()
    for kind in dict.fromkeys((wk, "none", "tensor")):
        if kind == "none" and fact == "softmax":
            continue          # rnnt_loss_pruned_kd itself: _softmax_without_weights_is_rnnt_loss_pruned_kd
        for red in dict.fromkeys((reduction, "none", "sum", "mean")):
            args = (sym, rg, blank, fact, kind, mode, tau, rnnt_type, penalty, red)
            loss, kd, _ = run_new(ft, dev, x.to(dev), y.to(dev), *args)
            loss2, kd2, _ = run_two(ft, dev, x.to(dev), y.to(dev), *args)
            print(f"{kind} {red}: loss {loss.tolist()} / {loss2.tolist()}, kd {kd.tolist()} / {kd2.tolist()}")
            assert loss.dtype == torch.float32 and kd.dtype == torch.float32 and loss.shape == loss2.shape and kd.shape == kd2.shape
            assert torch.isfinite(loss).all() and torch.isfinite(kd).all()
            assert torch.equal(loss, loss2), f"loss, weights {kind}, reduction {red}"
            assert torch.equal(kd, kd2), f"kd, weights {kind}, reduction {red}"


def _softmax_without_weights_is_rnnt_loss_pruned_kd(ft, dev, C, sdt, tdt, mode):
    x, y, sym, blank = inputs(C, mode == "collapsed", True, sdt, tdt)
    symd, rgd, bdd = _dev(dev, sym, K.band_ranges(), K.BOUNDARY)
    calls, out = [], []
    ft._lib.set_profile_hook(lambda name: calls.append(name) or contextlib.nullcontext())
    try:
        for f in (ft.rnnt_loss_pruned_kd_factored, ft.rnnt_loss_pruned_kd):
            xx = x.to(dev).requires_grad_(True)
            loss, kd = f(xx, y.to(dev), symd, rgd, blank, bdd, mode=mode, temperature=2.0, rnnt_type="modified", delay_penalty=0.1,
                         reduction="sum")
            (loss + 0.5 * kd).backward()
            out.append((loss.detach(), kd.detach(), xx.grad))
    finally:
        ft._lib.set_profile_hook(None)
    assert all(torch.equal(u, v) for u, v in zip(*out))
    assert not [c for c in calls if "fact" in c], calls       # the same kernels, through the same entries


# ---- 2. occupancy

def test_occupancy(ft, dev, oracle, monkeypatch):
    _each(OCC_CASES, _occupancy, ft, dev, oracle, monkeypatch)


def _occupancy(ft, dev, oracle, monkeypatch, C, sdt, tdt, fact, mode, tau, rnnt_type, penalty):
    coll = mode == "collapsed"
    x, y, sym, blank = inputs(C, coll, True, sdt, tdt)
    rg = K.band_ranges()
    symd, rgd, bdd = _dev(dev, sym, rg, K.BOUNDARY)
    xd, yd = x.to(dev), y.to(dev)
    occ64 = ref_occupancy(oracle, fact, x, sym, blank, rg, rnnt_type, penalty, (C, coll, sdt, rnnt_type, penalty))
    valid = R.valid_nodes(rg, K.BOUNDARY, S)
    xr = xd.clone().requires_grad_(True)
    occ = ft.rnnt_node_occupancy_pruned(xr, symd, rgd, blank, bdd, factorization=fact, rnnt_type=rnnt_type, delay_penalty=penalty)
    assert occ.dtype == torch.float32 and tuple(occ.shape) == (B, T, RR) and not occ.requires_grad and occ.is_contiguous()
    o = occ.cpu().numpy().astype(np.float64)
    err = float(np.abs(o - occ64).max())
    print(f"occupancy: max |occ - occ64| = {err:.3g}, max occ64 = {occ64.max():.3g}, sum = {occ64.sum():.4g}")
    assert err <= 2e-4
    assert (o[~valid] == 0).all() and (occ64[~valid] == 0).all() and (o[valid] > 0).any()
    monkeypatch.setenv("FTR_PRUNED_ROUTE", "lattice")
    ol = ft.rnnt_node_occupancy_pruned(xd, symd, rgd, blank, bdd, factorization=fact, rnnt_type=rnnt_type, delay_penalty=penalty)
    monkeypatch.delenv("FTR_PRUNED_ROUTE")
    ol = ol.cpu().numpy().astype(np.float64)
    print(f"occupancy, lattice route: max |occ - occ64| = {np.abs(ol - occ64).max():.3g}")
    assert np.abs(ol - occ64).max() <= 2e-4 and (ol[~valid] == 0).all()
    # node_weights="occupancy" is the call with node_weights=occ, and the single function given occ: values and gradients
    args = (sym, rg, blank, fact)
    tail = (mode, tau, rnnt_type, penalty)
    for red, w in (("none", WEIGHTS[3]), ("mean", WEIGHTS[0]), ("sum", WEIGHTS[2])):
        a = run_new(ft, dev, xd, yd, *args, "occupancy", *tail, red, w=w)
        b = run_new(ft, dev, xd, yd, *args, occ, *tail, red, w=w)
        c = run_two(ft, dev, xd, yd, *args, occ, *tail, red)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), red
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]), red
        assert torch.isfinite(a[2].float()).all() and a[2].abs().max() > 0
    # a part without an upstream gradient (None): the single op's gradient given occ; the loss alone reads no teacher row
    for part, yy in ((0, torch.full_like(yd, float("nan"))), (1, yd)):
        g = run_new(ft, dev, xd, yy, *args, "occupancy", *tail, "sum", part=part)[2]
        own = run_two(ft, dev, xd, yd, *args, occ, *tail, "sum", part=part)[2]
        assert torch.isfinite(g.float()).all() and g.abs().max() > 0 and torch.equal(g, own), f"part {part} alone"
    # kd against float64: sum occ64 * KL64
    kd = run_new(ft, dev, xd, yd, *args, "occupancy", *tail, "none")[1].cpu().numpy().astype(np.float64)
    kd64 = ref_kd(fact, x, y, sym, blank, rg, mode, tau, occ64, (C, mode, tau, sdt, tdt, "occ", rnnt_type, penalty))[0]
    kl64 = ref_kd(fact, x, y, sym, blank, rg, mode, tau, None, (C, mode, tau, sdt, tdt, "none"))[0]
    bound = 1e-4 * np.abs(kd64) + 2e-4 * kl64
    print(f"kd {kd.tolist()} kd64 {kd64.tolist()} |d| / bound {(np.abs(kd - kd64) / bound).tolist()}")
    assert (np.abs(kd - kd64) <= bound).all()


# ---- 3. gradient

def test_gradient(ft, dev, oracle):
    _each(CASES, _gradient, ft, dev, oracle)


def _gradient(ft, dev, oracle, C, blank_last, sdt, tdt, fact, wk, mode, tau, rnnt_type, penalty, reduction):
    coll = mode == "collapsed"
    x, y, sym, blank = inputs(C, coll, blank_last, sdt, tdt)
    rg = K.band_ranges()
    wts = tensor_weights() if wk == "tensor" else None
    gl = ref_loss_grad(oracle, fact, x, sym, blank, rg, rnnt_type, penalty, (C, coll, blank_last, sdt, rnnt_type, penalty))
    gk = ref_kd(fact, x, y, sym, blank, rg, mode, tau, wts, (C, mode, blank_last, tau, sdt, tdt, wk))[1]
    xd, yd = x.to(dev), y.to(dev)
    args = (sym, rg, blank, fact, wk, mode, tau, rnnt_type, penalty)
    valid = R.valid_nodes(rg, K.BOUNDARY, S)
    for w in WEIGHTS:
        red = "none" if isinstance(w[0], np.ndarray) else reduction
        what = f"C={C} {sdt}/{tdt} {fact} {wk} {mode} tau={tau} {rnnt_type} pen={penalty} {red} w={w}"
        g = run_new(ft, dev, xd, yd, *args, red, w=w)[2]
        assert g.dtype == x.dtype and g.shape == x.shape
        check_grad(g, combined(gl, gk, w, red), sdt, what, rg)       # also: zeros past t_end and in the rows of invalid nodes
        if isinstance(w[0], float) and 0.0 in w:          # a part under a zero upstream gradient: still the single op's gradient
            own = run_two(ft, dev, xd, yd, *args, red, w=w)[2]
            assert torch.equal(g, own), f"{what}: against the single op's gradient"
    # A part WITHOUT an upstream gradient (None, not a zero): the single op's gradient bit for bit.  For the loss alone every
    # teacher row holds NaN: an absent distillation part reads none of them.
    nan_teacher = torch.full_like(yd, float("nan"))
    alone = {}
    for part, yy in ((0, nan_teacher), (1, yd)):
        alone[part] = run_new(ft, dev, xd, yy, *args, reduction, part=part)[2]
        own = run_two(ft, dev, xd, yd, *args, reduction, part=part)[2]
        assert torch.isfinite(alone[part].float()).all() and alone[part].abs().max() > 0, f"part {part} alone"
        assert torch.equal(alone[part], own), f"part {part} alone against the single op's gradient"
    if wts is not None:       # where the weight is 0 the distillation part is skipped: the row is the loss-only (None) row
        zero = torch.from_numpy(valid & (wts == 0))
        assert zero.any()
        both = run_new(ft, dev, xd, yd, *args, reduction, w=(1.0, 1.0))[2]
        assert torch.equal(both.cpu()[zero], alone[0].cpu()[zero]), "distillation part in rows of weight 0"
        assert (alone[1].cpu()[zero] == 0).all(), "kd-only gradient in rows of weight 0"
        assert not torch.equal(both, alone[0])


# ---- 4. what is not read

def test_rows_that_are_not_read_hold_nan(ft, dev):
    _each([(36, "f32", "f32", "hat", "tensor", "full", "regular"), (500, "bf16", "fp16", "softmax", "tensor", "collapsed", "modified"),
           (2056, "fp16", "bf16", "hat", "occupancy", "full", "regular"), (520, "f32", "f32", "hat", "none", "collapsed", "modified")],
          _rows_that_are_not_read_hold_nan, ft, dev)


def _rows_that_are_not_read_hold_nan(ft, dev, C, sdt, tdt, fact, wk, mode, rnnt_type):
    x, y, sym, blank = inputs(C, mode == "collapsed", False, sdt, tdt)
    rg = K.band_ranges()
    valid = R.valid_nodes(rg, K.BOUNDARY, S)
    skip_teacher = ~valid
    if wk == "tensor":
        skip_teacher = skip_teacher | (tensor_weights() == 0)
    frames_out = np.zeros((B, T, RR), bool)
    frames_out[1, int(K.BOUNDARY[1, 3]):] = True
    xp, yp = x.clone(), y.clone()
    yp[torch.from_numpy(skip_teacher)] = float("nan")
    xp[torch.from_numpy(frames_out)] = float("nan")
    assert torch.isnan(yp[1, 8, 2]).all() and torch.isnan(xp[1, 10]).all() and torch.isfinite(xp[1, 8, 2]).all()
    args = (sym, rg, blank, fact, wk, mode, 1.0, rnnt_type, 0.1, "none")
    for w, part in (((1.0, 0.5), None), (None, 0), (None, 1)):      # both parts; each alone, the other without a gradient
        got = run_new(ft, dev, xp.to(dev), yp.to(dev), *args, w=w, part=part)
        clean = run_new(ft, dev, x.to(dev), y.to(dev), *args, w=w, part=part)
        assert all(torch.isfinite(v.float()).all() for v in got), (w, part)
        assert all(torch.equal(u, v) for u, v in zip(got, clean)), (w, part)
        assert (got[2].cpu()[torch.from_numpy(~valid)] == 0).all()


# ---- 5. other routes

def _wide_case(dev):
    """s_range = 16: B=2 T=12 S=17 C=8, a band of 16 rows that climbs from 0 to 2"""
    rng = np.random.default_rng(616)
    Sn, r, C = 17, 16, 8
    x = (2.0 * rng.standard_normal((B, T, r, C))).astype(np.float32)
    y = (2.0 * rng.standard_normal((B, T, r, C))).astype(np.float32)
    sym = rng.integers(1, C - 1, (B, Sn)).astype(np.int32)
    s0 = np.minimum(np.arange(T) // 4, Sn + 1 - r)
    rg = np.broadcast_to(s0[None, :, None] + np.arange(r)[None, None, :], (B, T, r)).astype(np.int32)
    bd = np.array([[0, 0, Sn, T], [0, 0, Sn - 2, T - 3]], np.int32)
    w = (0.25 + rng.random((B, T, r))).astype(np.float32)
    w[rng.random((B, T, r)) < 0.3] = 0.0
    return x, y, sym, rg, bd, w


def test_other_routes_are_the_composition(ft, dev, monkeypatch):
    kinds = [("f32", "f32", "hat", "none", "full"), ("bf16", "f32", "softmax", "tensor", "collapsed"), ("f32", "bf16", "hat", "occupancy", "full")]
    _each([(route,) + k for route in ("lattice", "no_band", "constrained", "s_range_16") for k in kinds],
          _other_route_is_the_composition, ft, dev, monkeypatch)


def _other_route_is_the_composition(ft, dev, monkeypatch, route, sdt, tdt, fact, wk, mode):
    if route == "s_range_16":
        x, y, sym, rg, bd, w16 = _wide_case(dev)
        x, y, blank = torch.from_numpy(x).to(DT[sdt][0]), torch.from_numpy(y).to(DT[tdt][0]), 0
        if wk == "tensor":
            wk = w16
    else:
        x, y, sym, blank = inputs(36, mode == "collapsed", True, sdt, tdt)
        rg = no_band_ranges() if route == "no_band" else K.band_ranges()
        bd = K.BOUNDARY
    rnnt_type = "constrained" if route == "constrained" else "regular"
    if route == "lattice":
        monkeypatch.setenv("FTR_PRUNED_ROUTE", "lattice")
    calls = []
    ft._lib.set_profile_hook(lambda name: calls.append(name) or contextlib.nullcontext())
    try:
        args = (sym, rg, blank, fact, wk, mode, 2.0, rnnt_type, 0.1, "sum")
        loss, kd, g = run_new(ft, dev, x.to(dev), y.to(dev), *args, w=(1.0, 0.5), boundary=bd)
    finally:
        ft._lib.set_profile_hook(None)
    assert not [c for c in calls if "band_kd" in c or "node_occupancy" in c], calls
    loss2, kd2, g2 = run_two(ft, dev, x.to(dev), y.to(dev), *args, w=(1.0, 0.5), boundary=bd)
    assert torch.isfinite(loss) and torch.isfinite(kd) and g.abs().max() > 0
    assert torch.equal(loss, loss2) and torch.equal(kd, kd2) and torch.equal(g, g2)
    monkeypatch.delenv("FTR_PRUNED_ROUTE", raising=False)


def _the_band_route_is_the_fused_one(ft, dev, fact, wk, entries):
    x, y, sym, blank = inputs(36, False, True, "f32", "f32")
    calls = []
    ft._lib.set_profile_hook(lambda name: calls.append(name) or contextlib.nullcontext())
    try:
        run_new(ft, dev, x.to(dev), y.to(dev), sym, K.band_ranges(), blank, fact, wk, "full", 1.0, "modified", 0.0, "mean", w=(1.0, 0.5))
    finally:
        ft._lib.set_profile_hook(None)
    calls = [c for c in calls if c != "ftr_band_ranges_check_i32"]
    occ = ["ftr_band_node_occupancy_f32", "ftr_pruned_kd_weighted_utt_sum_f32"][:entries]
    assert calls == ["ftr_pruned_band_kd_fact_fwd_dt", "ftr_mutual_information_band_ws_f32", *occ, "ftr_pruned_kd_reduce_f32",
                     "ftr_negated_reduce_f32", "ftr_pruned_band_kd_fact_bwd_scaled_dt"], calls


# ---- 6. determinism and capture

def _two_runs_are_bit_identical(ft, dev, sdt, tdt, fact, wk, mode):
    x, y, sym, blank = inputs(500, mode == "collapsed", True, sdt, tdt)
    args = (sym, K.band_ranges(), blank, fact, wk, mode, 1.0, "regular", 0.1, "mean")
    a = run_new(ft, dev, x.to(dev), y.to(dev), *args, w=(1.0, 0.5))
    b = run_new(ft, dev, x.to(dev), y.to(dev), *args, w=(1.0, 0.5))
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_determinism_and_capture(ft, dev):
    """Two runs are bit-identical.  Forward + backward on a marked band captured once; three replays with other input contents
    give the eager results bit for bit (the pattern of tests/test_gpu_kd_loss.py)."""
    _each([("f32", "f32", "hat", "tensor", "full"), ("fp16", "bf16", "softmax", "occupancy", "collapsed")], _two_runs_are_bit_identical, ft, dev)
    _each([("f32", "f32", "hat", "occupancy", "full"), ("bf16", "f32", "softmax", "tensor", "collapsed")], _a_captured_step_replays, ft, dev)


def _a_captured_step_replays(ft, dev, sdt, tdt, fact, wk, mode):
    C = 500
    x0, y0, sym, blank = inputs(C, mode == "collapsed", True, sdt, tdt)
    xbuf, ybuf = x0.to(dev).clone(), y0.to(dev).clone()
    symd, rgd, bdd = _dev(dev, sym, K.band_ranges(), K.BOUNDARY)
    wts = _wts(dev, wk)
    importlib.import_module("tf_fast_rnnt.rnnt_loss")._mark_band(rgd)     # (ft.rnnt_loss is the function of that name)

    def step():
        xx = xbuf.detach().requires_grad_(True)
        loss, kd = ft.rnnt_loss_pruned_kd_factored(xx, ybuf, symd, rgd, blank, bdd, factorization=fact, mode=mode, temperature=2.0,
                                                   node_weights=wts, reduction="mean")
        (loss + 0.5 * kd).backward()
        return dict(loss=loss.detach(), kd=kd.detach(), grad=xx.grad)

    calls = []
    ft._lib.set_profile_hook(lambda name: calls.append(name) or contextlib.nullcontext())
    try:
        g, out = _capture(step)
    finally:
        ft._lib.set_profile_hook(None)
    assert calls.count("ftr_pruned_band_kd_fact_bwd_scaled_dt") == 4, "the warm-up or the captured step left the fused route"
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

def test_the_neighbours_are_untouched_by_calls_of_the_new_functions(ft, dev):
    """The same float32 calls of rnnt_loss_pruned_kd, rnnt_kd_loss_pruned_factored and hat_loss_pruned before and after calls
    of the new functions, in one process: bit-identical values and gradients."""
    x, y, sym, blank = inputs(500, False, True, "f32", "f32")
    xd, yd = x.to(dev) * 1.37, y.to(dev) * 1.37       # not representable in 16 bits
    symd, rgd, bdd = _dev(dev, sym, K.band_ranges(), K.BOUNDARY)
    wts = torch.from_numpy(tensor_weights()).to(dev)

    def neighbours():
        out = []
        xx = xd.clone().requires_grad_(True)
        loss, kd = ft.rnnt_loss_pruned_kd(xx, yd, symd, rgd, blank, bdd, temperature=2.0, reduction="sum")
        (loss + 0.5 * kd).backward()
        out += [loss.detach(), kd.detach(), xx.grad]
        for fact in ("softmax", "hat"):
            xx = xd.clone().requires_grad_(True)
            kd = ft.rnnt_kd_loss_pruned_factored(xx, yd, symd, rgd, blank, bdd, factorization=fact, temperature=2.0,
                                                 node_weights=wts, reduction="sum")
            kd.backward()
            out += [kd.detach(), xx.grad]
        xx = xd.clone().requires_grad_(True)
        loss = ft.hat_loss_pruned(xx, symd, rgd, blank, bdd, delay_penalty=0.1, reduction="sum")
        loss.backward()
        return out + [loss.detach(), xx.grad]

    before = neighbours()
    for sdt, tdt, fact, wk in (("bf16", "f32", "hat", "tensor"), ("fp16", "bf16", "softmax", "occupancy"), ("f32", "f32", "hat", "occupancy")):
        xs, ys, _, _ = inputs(500, False, True, sdt, tdt)
        run_new(ft, dev, xs.to(dev), ys.to(dev), sym, K.band_ranges(), blank, fact, wk, "full", 2.0, "regular", 0.0, "sum", w=(1.0, 0.5))
        ft.rnnt_node_occupancy_pruned(xs.to(dev), symd, rgd, blank, bdd, factorization=fact)
    after = neighbours()
    assert all(torch.equal(u, v) for u, v in zip(before, after))


# ---- 8. layout

def test_student_at_an_odd_element(ft, dev, oracle):
    """A contiguous 16-bit student whose storage starts at an odd element (2-byte aligned only): the scalar path.  The values
    are those of the single functions on the same view, bit for bit; the gradient keeps the rule of this file."""
    _each([("bf16", "hat", "tensor", "full"), ("fp16", "softmax", "tensor", "collapsed"), ("bf16", "hat", "occupancy", "collapsed")],
          _student_at_an_odd_element, ft, dev, oracle)


def _student_at_an_odd_element(ft, dev, oracle, dt, fact, wk, mode):
    coll = mode == "collapsed"
    x, y, sym, blank = inputs(500, coll, True, dt, dt)
    rg = K.band_ranges()
    n = x.numel()
    buf = torch.zeros(n + 9, dtype=x.dtype, device=dev)
    off = buf[1:1 + n].view(x.shape)
    off.copy_(x)
    assert off.is_contiguous() and off.data_ptr() % 4 == 2
    args = (sym, rg, blank, fact, wk, mode, 1.0, "regular", 0.0, "sum")
    loss, kd, g = run_new(ft, dev, off, y.to(dev), *args, w=(1.0, 0.5))
    loss2, kd2, _ = run_two(ft, dev, off, y.to(dev), *args)
    assert torch.equal(loss, loss2) and torch.equal(kd, kd2)
    al = run_new(ft, dev, x.to(dev), y.to(dev), *args)
    assert abs(loss.item() - al[0].item()) <= 1e-4 * abs(al[0].item()) and abs(kd.item() - al[1].item()) <= 1e-4 * abs(al[1].item())
    wts = tensor_weights()
    if wk == "occupancy":     # the weights the op used: this student's occupancies, float32 -> exact in float64
        symd, rgd, bdd = _dev(dev, sym, rg, K.BOUNDARY)
        wts = ft.rnnt_node_occupancy_pruned(off, symd, rgd, blank, bdd, factorization=fact).cpu().numpy()
        occ64 = ref_occupancy(oracle, fact, x, sym, blank, rg, "regular", 0.0, (500, coll, dt, "regular", 0.0))
        assert np.abs(wts - occ64).max() <= 2e-4
    gl = ref_loss_grad(oracle, fact, x, sym, blank, rg, "regular", 0.0, (500, coll, True, dt, "regular", 0.0))
    gk = ref_kd(fact, x, y, sym, blank, rg, mode, 1.0, wts, (500, mode, True, 1.0, dt, dt, wk, "odd"))[1]
    check_grad(g, combined(gl, gk, (1.0, 0.5), "sum"), dt, f"odd student {fact} {wk} {mode} {dt}", rg)
    assert float(buf[0]) == 0 and (buf[1 + n:] == 0).all()     # the neighbours are untouched
    assert torch.equal(off, x.to(dev))


# ---- 9. refusals

def test_refusals(ft, dev):
    x, y, sym, blank = inputs(36, False, True, "f32", "f32")
    symd, rgd, bdd = _dev(dev, sym, K.band_ranges(), K.BOUNDARY)
    xd, yd = x.to(dev), y.to(dev)
    f, occ = ft.rnnt_loss_pruned_kd_factored, ft.rnnt_node_occupancy_pruned
    with pytest.raises(ValueError, match="out of scope"):
        f(xd, yd, symd, rgd, blank, bdd, factorization="tdt")
    with pytest.raises(ValueError, match="out of scope"):
        occ(xd, symd, rgd, blank, bdd, factorization="tdt")
    with pytest.raises(ValueError, match="factorization"):
        f(xd, yd, symd, rgd, blank, bdd, factorization="other")
    with pytest.raises(ValueError, match="node_weights"):
        f(xd, yd, symd, rgd, blank, bdd, node_weights="occupancies")
    w = torch.ones((B, T, RR), device=dev)
    with pytest.raises(TypeError, match="node_weights"):
        f(xd, yd, symd, rgd, blank, bdd, node_weights=w.double())
    with pytest.raises(ValueError, match="node_weights"):
        f(xd, yd, symd, rgd, blank, bdd, node_weights=w[:, :-1].contiguous())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(xd, yd, symd, rgd, blank, bdd, node_weights=w.cpu())
    x1, y1 = xd[..., :1].contiguous(), yd[..., :1].contiguous()
    with pytest.raises(ft.FtrError, match="HAT") as new:          # the refusal of hat_loss_pruned, which is asked first
        f(x1, y1, symd * 0, rgd, 0, bdd, factorization="hat", node_weights="occupancy")
    with pytest.raises(ft.FtrError, match="HAT") as old:
        ft.hat_loss_pruned(x1, symd * 0, rgd, 0, bdd)
    assert str(new.value) == str(old.value)
    with pytest.raises(ValueError, match="hat"):
        occ(x1, symd * 0, rgd, 0, bdd, factorization="hat")
    for bad_x, bad_y in ((xd.double(), yd), (xd, yd.double())):
        with pytest.raises(TypeError):
            f(bad_x, bad_y, symd, rgd, blank, bdd, factorization="hat")
    with pytest.raises(ValueError, match="mode"):
        f(xd, yd, symd, rgd, blank, bdd, factorization="hat", mode="both")
    with pytest.raises(ValueError, match="temperature"):
        f(xd, yd, symd, rgd, blank, bdd, node_weights=w, temperature=0.0)
    with pytest.raises(ValueError, match="reduction"):
        f(xd, yd, symd, rgd, blank, bdd, node_weights="occupancy", reduction="max")
    with pytest.raises(ValueError, match="rnnt_type"):
        occ(xd, symd, rgd, blank, bdd, rnnt_type="other")
    cpu = (torch.from_numpy(sym), torch.from_numpy(K.band_ranges()), blank, torch.from_numpy(K.BOUNDARY))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(x, y, *cpu, factorization="hat")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(xd, y, symd, rgd, blank, bdd, node_weights="occupancy")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        occ(x, *cpu)
