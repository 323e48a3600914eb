"""rnnt_kd_loss_pruned on the device: knowledge distillation on the pruned band, against the float64 restatement of its
definition (tests/kd_restatement.py) on the up-converted values.

Geometry (tests/kd_cases.py): B=2 T=12 S=5 r=3, boundary [[0,0,5,12],[0,0,3,9]], a hand-built band; utterance 1 has invalid
nodes both by frame and by s > s_end.  C crosses every path of the kernels: 8 (vector path, 2 of 64 lanes live), 37 (element
path), 500 (c3's vocabulary, 16-bit rows 8- but not 16-byte aligned), 1000 (four quads per lane, the register width of c4's
vocabulary), 2048 (the largest register-resident row), 2056 (the two-pass form).  Inputs are standard normal x 3 rounded to
the dtype; in collapsed mode ln C is added to the blank and the correct-symbol columns of both tensors so that all three
classes carry mass.

Tolerances, none of them measured from the code under test:
  loss      |err| <= 1e-4 |ref| + 1e-5 per utterance: the project's tolerance against float64
  gradient  |g - g64| <= u |g64| + a + 1e-4 max|g64|, (u, a) = (0, 0) float32, (2^-8, 0) bfloat16, (2^-11, 2^-25) float16:
            check_grad's rule of tests/test_gpu_lowp.py -- one rounding into the storage type on top of the float32 budget
With FTR_KD_PARITY_OUT set, the largest errors seen are written there as JSON when the module is done."""
import json
import os

import numpy as np
import pytest
import torch

import kd_cases as K
import kd_restatement as R

pytestmark = pytest.mark.gpu

DT = {"f32": (torch.float32, 0.0, 0.0), "bf16": (torch.bfloat16, 2.0 ** -8, 0.0), "fp16": (torch.float16, 2.0 ** -11, 2.0 ** -25)}
PAIRS = [("f32", "f32"), ("bf16", "bf16"), ("fp16", "fp16"), ("f32", "bf16"), ("bf16", "f32")]   # (student, teacher)
CS = [8, 37, 500, 1000, 2048, 2056]
MODES = ["full", "collapsed"]
VALID = R.valid_nodes(K.band_ranges(), K.BOUNDARY, K.S)
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("FTR_KD_PARITY_OUT")
    if path and _WORST:
        with open(path, "w") as f:
            json.dump({k: _WORST[k] for k in sorted(_WORST)}, f, indent=1)
            f.write("\n")


def _note(key, **vals):
    rec = _WORST.setdefault(key, {})
    for k, v in vals.items():
        rec[k] = max(rec.get(k, 0.0), float(v))


_INPUTS, _REFS = {}, {}


def inputs(C, mode, blank_last, sdt, tdt):
    """(student, teacher, symbols, blank): cpu tensors rounded to the dtypes; cached, never modified"""
    key = (C, mode == "collapsed", blank_last, sdt, tdt)
    if key not in _INPUTS:
        x, y, sym, blank = K.logits_pair(C, blank_last, mode == "collapsed")
        _INPUTS[key] = (torch.from_numpy(x).to(DT[sdt][0]), torch.from_numpy(y).to(DT[tdt][0]), sym, blank)
    return _INPUTS[key]


def case(C, mode, blank_last, tau, sdt, tdt):
    """inputs() and the float64 reference (loss [B], gradient) on the up-converted values, computed once per key"""
    key = (C, mode, blank_last, tau, sdt, tdt)
    x, y, sym, blank = inputs(C, mode, blank_last, sdt, tdt)
    if key not in _REFS:
        _REFS[key] = R.kd_loss_and_grad(x.float().numpy(), y.float().numpy(), sym, K.band_ranges(), blank, K.BOUNDARY, mode, tau)
    return (x, y, sym, blank) + _REFS[key]


def run(ft, dev, x, y, sym, blank, mode, tau, reduction="none", weight=None, teacher_grad=False):
    """(loss, d (weight . loss) / d x) for device tensors x, y (x is made a leaf here)"""
    x = x.detach().requires_grad_(True)
    y = y.detach().requires_grad_(teacher_grad)
    loss = ft.rnnt_kd_loss_pruned(x, y, torch.from_numpy(sym).to(dev), torch.from_numpy(K.band_ranges()).to(dev), blank,
                                  torch.from_numpy(K.BOUNDARY).to(dev), mode=mode, temperature=tau, reduction=reduction)
    out = loss if weight is None else loss * weight
    out.sum().backward()
    assert y.grad is None
    return loss.detach(), x.grad


def check_loss(loss, ref, what):
    got = loss.cpu().numpy().astype(np.float64)
    assert loss.dtype == torch.float32 and got.shape == ref.shape and np.isfinite(got).all(), what
    err = np.abs(got - ref)
    worst = float((err / (1e-4 * np.abs(ref) + 1e-5)).max())
    print(f"{what}: loss {got}, reference {ref}, |err| / bound = {worst:.3g}")
    assert worst <= 1.0, f"{what}: loss error is {worst:.3g} x its bound"
    return float((err / np.abs(ref)).max())


def check_grad(g, g64, sdt, what):
    _, u, a = DT[sdt]
    g = g.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all(), what
    bound = u * np.abs(g64) + a + 1e-4 * np.abs(g64).max()
    err = np.abs(g - g64)
    worst = float((err / bound).max())
    print(f"{what}: max |g - g64| / bound = {worst:.3g}, max |g64| = {np.abs(g64).max():.3g}")
    assert worst <= 1.0, f"{what}: gradient error is {worst:.3g} x its bound"
    assert (g[~VALID] == 0).all(), f"{what}: gradient in an invalid row"
    return worst, float(err.max() / np.abs(g64).max())


@pytest.mark.parametrize("sdt,tdt", PAIRS)
@pytest.mark.parametrize("tau", [1.0, 2.0])
@pytest.mark.parametrize("blank_last", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", CS)
def test_loss_and_gradient(ft, dev, C, mode, blank_last, tau, sdt, tdt):
    x, y, sym, blank, ref, g64 = case(C, mode, blank_last, tau, sdt, tdt)
    what = f"C={C} {mode} blank={'last' if blank_last else 'first'} tau={tau} {sdt}/{tdt}"
    loss, g = run(ft, dev, x.to(dev), y.to(dev), sym, blank, mode, tau, teacher_grad=True)
    rel = check_loss(loss, ref, what)
    assert g.dtype == x.dtype and g.shape == x.shape
    frac, gerr = check_grad(g, g64, sdt, what)
    _note(f"{mode} {sdt}/{tdt}", loss_rel_err=rel, grad_err_over_bound=frac, grad_err_over_max=gerr)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", [8, 37, 500])
def test_plain_c_entries_are_the_op_bit_for_bit(ft, dev, C, mode):
    """ftr_pruned_kd_fwd_dt and ftr_pruned_kd_bwd_scaled_dt (include/ftr_kd.h) called directly, upstream scale 1: the op itself
    goes through the entries of include/ftr_kd_fact.h, so this is what runs the plain ones on the device."""
    x, y, sym, blank = inputs(C, mode, False, "f32", "f32")
    x, y = x.to(dev), y.to(dev)
    loss, g = run(ft, dev, x, y, sym, blank, mode, 2.0)
    symd, rg, bd = torch.from_numpy(sym).to(dev), torch.from_numpy(K.band_ranges()).to(dev), torch.from_numpy(K.BOUNDARY).to(dev)
    code = ft._lib.FTR_KD_COLLAPSED if mode == "collapsed" else ft._lib.FTR_KD_FULL
    f32 = ft._lib.FTR_DTYPE_F32
    node = torch.empty((K.B, K.T, K.R), device=dev)
    saved = torch.empty((4 if mode == "collapsed" else 2, K.B, K.T, K.R), device=dev)
    utt, gx, one = torch.empty(K.B, device=dev), torch.empty_like(x), torch.ones(K.B, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    ft._lib.call("ftr_pruned_kd_fwd_dt", x.data_ptr(), f32, y.data_ptr(), f32, symd.data_ptr(), rg.data_ptr(), bd.data_ptr(), blank,
                 2.0, code, node.data_ptr(), saved.data_ptr(), utt.data_ptr(), K.B, K.T, K.S, C, K.R, st)
    ft._lib.call("ftr_pruned_kd_bwd_scaled_dt", x.data_ptr(), f32, y.data_ptr(), f32, symd.data_ptr(), rg.data_ptr(), bd.data_ptr(),
                 blank, 2.0, code, saved.data_ptr(), one.data_ptr(), 1, 1.0, gx.data_ptr(), K.B, K.T, K.S, C, K.R, st)
    assert torch.isfinite(utt).all() and (utt > 0).all() and gx.abs().max() > 0
    assert torch.equal(utt, loss) and torch.equal(gx, g)


@pytest.mark.parametrize("sdt,tdt", [("f32", "f32"), ("bf16", "f32")])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", [37, 500])
def test_reductions(ft, dev, C, mode, sdt, tdt):
    """"sum" and "mean" are the reductions of "none" (mean: over B of the per-utterance sums), to float32 rounding."""
    x, y, sym, blank, ref, g64 = case(C, mode, True, 1.0, sdt, tdt)
    none, _ = run(ft, dev, x.to(dev), y.to(dev), sym, blank, mode, 1.0)
    for reduction, want, scale in (("sum", none.double().sum().item(), 1.0), ("mean", none.double().mean().item(), 1.0 / K.B)):
        loss, g = run(ft, dev, x.to(dev), y.to(dev), sym, blank, mode, 1.0, reduction=reduction)
        assert loss.shape == () and loss.dtype == torch.float32
        assert abs(loss.item() - want) <= 4 * 2.0 ** -24 * abs(want)          # B = 2 addends, one division: a few ulp
        check_grad(g, g64 * scale, sdt, f"{reduction} C={C} {mode} {sdt}/{tdt}")


@pytest.mark.parametrize("sdt,tdt", [("f32", "f32"), ("bf16", "fp16")])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", CS)
def test_invalid_rows_are_never_read(ft, dev, C, mode, sdt, tdt):
    """Every invalid row of both tensors filled with NaN: loss and valid gradient rows bit-identical, invalid rows zero."""
    x, y, sym, blank = inputs(C, mode, False, sdt, tdt)
    clean = run(ft, dev, x.to(dev), y.to(dev), sym, blank, mode, 1.0)
    xp, yp = x.clone(), y.clone()
    bad = torch.from_numpy(~VALID)
    xp[bad] = float("nan")
    yp[bad] = float("nan")
    assert torch.isnan(xp).any() and torch.isnan(yp[1, 10]).all() and torch.isnan(xp[1, 8, 2]).all()
    poisoned = run(ft, dev, xp.to(dev), yp.to(dev), sym, blank, mode, 1.0)
    assert torch.equal(clean[0], poisoned[0]) and torch.isfinite(poisoned[0]).all()
    assert torch.equal(clean[1], poisoned[1])
    assert (poisoned[1].cpu()[bad] == 0).all()


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", [37, 500, 2056])
def test_self_distillation(ft, dev, C, mode, dt):
    """Teacher = student (the same values): no loss, and a gradient within check_grad's rule of the zero reference --
    u |0| + a + 1e-4 max|0| = a, which is exact zeros for float32 and bfloat16."""
    x, _, sym, blank = inputs(C, mode, True, dt, dt)
    loss, g = run(ft, dev, x.to(dev), x.to(dev).clone(), sym, blank, mode, 2.0)
    assert (loss.abs() <= 1e-5).all(), loss
    worst = np.abs(g.float().cpu().numpy()).max()
    print(f"self-distillation C={C} {mode} {dt}: loss {loss.tolist()}, max |g| = {worst:.3g}")
    assert worst <= DT[dt][2]


@pytest.mark.parametrize("sdt,tdt", [("f32", "f32"), ("fp16", "bf16")])
@pytest.mark.parametrize("mode", MODES)
def test_two_runs_are_bit_identical(ft, dev, mode, sdt, tdt):
    x, y, sym, blank = inputs(500, mode, True, sdt, tdt)
    for reduction in ("none", "mean"):
        a = run(ft, dev, x.to(dev), y.to(dev), sym, blank, mode, 1.0, reduction=reduction)
        b = run(ft, dev, x.to(dev), y.to(dev), sym, blank, mode, 1.0, reduction=reduction)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("sdt,tdt", [("f32", "f32"), ("bf16", "bf16")])
@pytest.mark.parametrize("mode", MODES)
def test_upstream_gradient_is_folded_in(ft, dev, mode, sdt, tdt):
    x, y, sym, blank, ref, g64 = case(500, mode, False, 2.0, sdt, tdt)
    for reduction, scale in (("sum", 2.5), ("mean", 2.5 / K.B)):
        _, g = run(ft, dev, x.to(dev), y.to(dev), sym, blank, mode, 2.0, reduction=reduction, weight=2.5)
        check_grad(g, g64 * scale, sdt, f"2.5 x {reduction} {mode} {sdt}")
    w = np.array([0.75, -1.5])
    _, g = run(ft, dev, x.to(dev), y.to(dev), sym, blank, mode, 2.0, weight=torch.tensor(w, dtype=torch.float32, device=dev))
    check_grad(g, g64 * w[:, None, None, None], sdt, f"weighted none {mode} {sdt}")


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", ["student", "teacher"])
def test_tensor_at_an_odd_element(ft, dev, which, mode, dt):
    """A contiguous 16-bit tensor whose storage starts at an odd element (2-byte aligned only: no 8-byte access may be made);
    the other tensor is aligned, so the row must run element by element for both."""
    x, y, sym, blank, ref, g64 = case(500, mode, True, 1.0, dt, dt)
    n = x.numel()
    buf = torch.zeros(n + 9, dtype=x.dtype, device=dev)
    off = buf[1:1 + n].view(x.shape)
    off.copy_(x if which == "student" else y)
    assert off.is_contiguous() and off.data_ptr() % 4 == 2
    xd, yd = (off, y.to(dev)) if which == "student" else (x.to(dev), off)
    loss, g = run(ft, dev, xd, yd, sym, blank, mode, 1.0)
    check_loss(loss, ref, f"odd {which} {mode} {dt}")
    check_grad(g, g64, dt, f"odd {which} {mode} {dt}")
    aligned = run(ft, dev, x.to(dev), y.to(dev), sym, blank, mode, 1.0)
    assert float(buf[0]) == 0 and (buf[1 + n:] == 0).all()     # the neighbours are untouched
    assert torch.equal(off, (x if which == "student" else y).to(dev))
    assert (aligned[0] - loss).abs().max() <= 1e-4 * loss.abs().max()


def test_non_contiguous_inputs(ft, dev):
    x, y, sym, blank, ref, g64 = case(37, "full", True, 1.0, "f32", "f32")
    big = torch.full((K.B, K.T, K.R, 37 + 5), 7.0, device=dev)
    big[..., :37] = x.to(dev)
    ty = y.to(dev).transpose(1, 2).contiguous().transpose(1, 2)
    assert not big[..., :37].is_contiguous() and not ty.is_contiguous()
    loss, g = run(ft, dev, big[..., :37], ty, sym, blank, "full", 1.0)
    check_loss(loss, ref, "slices")
    check_grad(g, g64, "f32", "slices")


@pytest.mark.parametrize("sdt,tdt", [("f32", "f32"), ("bf16", "f32")])
@pytest.mark.parametrize("mode", MODES)
def test_replays_from_a_graph_with_new_values(ft, dev, mode, sdt, tdt):
    """Forward + backward captured once on one stream; two replays with other input contents give the eager results, bit
    for bit."""
    C = 500
    x0, y0, sym, blank, _, _ = case(C, mode, True, 1.0, sdt, tdt)
    x = x0.to(dev).requires_grad_(True)
    y = y0.to(dev)
    symd, rg, bd = torch.from_numpy(sym).to(dev), torch.from_numpy(K.band_ranges()).to(dev), torch.from_numpy(K.BOUNDARY).to(dev)

    def step():
        loss = ft.rnnt_kd_loss_pruned(x, y, symd, rg, blank, bd, mode=mode, reduction="mean")
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
        fx, fy, _, _ = K.logits_pair(C, True, mode == "collapsed", seed=seed)
        with torch.no_grad():
            x.copy_(torch.from_numpy(fx))                 # new values, same buffers
            y.copy_(torch.from_numpy(fy))
        graph.replay()
        torch.cuda.synchronize()
        got = [v.clone() for v in out]
        ref = step()
        torch.cuda.synchronize()
        assert torch.isfinite(got[0]) and got[0] > 0
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
