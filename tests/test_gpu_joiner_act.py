"""do_rnnt_pruning_act (include/ftr_joiner_act.h, csrc/prune.hip, csrc/act_math.h): y[b,t,k,:] = act(am[b,t,:] +
lm[b, ranges[b,t,k], :]) for tanh and relu in float32, bfloat16 and float16, and its backward from g and the stored y.

* relu forward: bit-exact against torch.relu of the float32 sum, rounded once into the dtype.
* tanh forward: per element |y - want| <= u |want| + E 2^-24 |want| (+ 2^-25 for float16), want = the float64 tanh of the
  float32 sum, u = 2^-24, 2^-8, 2^-11.  E = max(2 E_ref, 2), where E_ref is the largest error, in float32 ulps of the
  result, of torch.tanh on the same float32 sums, measured in the test itself (never taken from the kernel under test).
  Exactly: +-1 at +-inf, NaN at NaN, 0 at 0, |y| <= 1 everywhere.
* backward: bit-exact against ftr_do_pruning_bwd_ws_f32 given the float32 tensor dz (formed by torch, every operation
  rounded on its own) as both gradients, rounded once into the dtype -- the definition.
* backward against float64 segment sums, independent of the project's kernels, per element within
      u |want| + (2n + 4) 2^-24 sum|g|  (+ 2^-25 for float16)
  (joiner_act_cases.bwd_bound); this includes 16-bit g / y at an odd element with C % 4 == 0, which no float twin covers.
* autograd, refusals, reproducibility and one graph capture.

With FTR_JOINER_ACT_PARITY_OUT set, E_ref, E, the forward's largest tanh error per dtype and the largest ratio to the backward
bound per dtype and activation are written to that file as JSON when the module is done; a run on MI355X is committed as
profiles/joiner_act_parity_errors.json."""
import json
import os

import pytest
import torch

import joiner_act_cases as jc
from joiner_act_cases import ACTS, BWD_SHAPES, DTYPES, FWD_SHAPES, RANGE_KINDS, SCALAR_SHAPE, SEG_SHAPES, UNIT, _name

pytestmark = pytest.mark.gpu

_REPORT = {"backward_largest_ratio_to_bound": {}, "tanh_forward": {}}


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    out = os.environ.get("FTR_JOINER_ACT_PARITY_OUT")
    if out and (_REPORT["tanh_forward"] or _REPORT["backward_largest_ratio_to_bound"]):
        with open(out, "w") as f:
            json.dump({"backward_bound": "u |want| + (2n + 4) 2^-24 sum|g| (+ 2^-25 for float16), per element of d am and d lm",
                       "tanh_forward_bound": "u |want| + E 2^-24 |want| (+ 2^-25 for float16); E = max(2 E_ref, 2), E_ref = torch.tanh's "
                                             "largest error on the float32 sums in float32 ulps of the result", **_REPORT},
                      f, indent=1, sort_keys=True)
            f.write("\n")


def _same_values(a, b):
    """torch.equal, with NaN equal to NaN."""
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(nan=7.0), b.nan_to_num(nan=7.0))


# ---------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("shape", FWD_SHAPES)
def test_relu_forward_is_exact(ft, dev, shape, dtype):
    am, lm, ranges = jc._fwd_case(shape, dtype, dev)            # ranges below 0 and above S among them: clamped
    want = torch.relu(jc.fwd_sum32(am, lm, ranges)).to(dtype)
    y = ft.do_rnnt_pruning_act(am, lm, ranges, activation="relu")
    assert y.dtype == dtype and y.is_contiguous() and tuple(y.shape) == (shape[0], shape[1], shape[4], shape[3])
    assert torch.equal(y, want) and bool((want == 0).any()) and bool((want > 0).any())
    if dtype != torch.float32:                                   # all three tensors at an odd element: element by element
        assert torch.equal(jc.act_forward(ft, am, lm, ranges, "relu", odd=True), want)
    # NaN and +-inf where IEEE puts them
    where = jc.plant(am, lm, ranges, [float("nan"), float("inf"), float("-inf")])
    want = torch.relu(jc.fwd_sum32(am, lm, ranges)).to(dtype)
    y = ft.do_rnnt_pruning_act(am, lm, ranges, activation="relu")
    assert _same_values(y, want)
    (tn, cn), (tp, cp), (tm, cm) = where
    assert torch.isnan(y[0, tn, :, cn]).all() and bool((y[0, tp, :, cp] == float("inf")).all()) and bool((y[0, tm, :, cm] == 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("shape", FWD_SHAPES)
def test_tanh_forward_is_within_the_ulp_budget(ft, dev, shape, dtype):
    am, lm, ranges = jc._fwd_case(shape, dtype, dev)
    where = jc.plant(am, lm, ranges)
    z32 = jc.fwd_sum32(am, lm, ranges)
    want = torch.tanh(z32.double())
    e_ref, E = jc.tanh_budget(z32)
    extra = 2.0 ** -25 if dtype == torch.float16 else 0.0
    for odd in ([False] if dtype == torch.float32 else [False, True]):
        y = ft.do_rnnt_pruning_act(am, lm, ranges) if not odd else jc.act_forward(ft, am, lm, ranges, "tanh", odd=True)
        assert y.dtype == dtype and tuple(y.shape) == tuple(z32.shape)
        yd = y.double()
        # exactly: NaN at NaN, +-1 at +-inf, 0 at 0, never beyond 1
        assert torch.equal(torch.isnan(y), torch.isnan(z32)) and bool(torch.isnan(y).any())
        assert bool((yd[z32 == float("inf")] == 1).all()) and bool((yd[z32 == float("-inf")] == -1).all())
        assert bool((z32 == 0).any()) and bool((yd[z32 == 0] == 0).all())
        finite = ~torch.isnan(z32)
        assert float(yd[finite].abs().max()) <= 1.0
        for i, v in enumerate(jc.PLANTED):                      # the planted sums are where they were put (k = 0 gathers the zeroed row)
            t, c = where[i]
            got = float(z32[0, t, 0, c])
            assert got == float(torch.tensor(v, dtype=dtype)) or (v != v and got != got), (i, v, got)
        err = (yd - want).abs()[finite]
        bound = (UNIT[dtype] * want.abs() + E * 2.0 ** -24 * want.abs() + extra)[finite]
        nz = bound > 0
        worst = float((err[nz] / bound[nz]).max())
        wf = want[finite]
        nzw = wf != 0
        own = float((err[nzw] / (jc.ulp32(wf[nzw]) if dtype == torch.float32 else UNIT[dtype] * wf[nzw].abs())).max())
        print(f"tanh {_name(dtype)} {shape} odd={odd}: E_ref = {e_ref:.3f} ulp, E = {E:.3f}, largest |y - want| / bound = {worst:.4f}, "
              f"largest error = {own:.3f} {'float32 ulp' if dtype == torch.float32 else 'u |want|'}")
        rec = _REPORT["tanh_forward"].setdefault(_name(dtype), {"E_ref_ulps": 0.0, "E": 0.0, "largest_ratio_to_bound": 0.0, "largest_error": 0.0,
                                                               "largest_error_unit": "float32 ulps of the result" if dtype == torch.float32 else "u |want|"})
        rec["E_ref_ulps"] = max(rec["E_ref_ulps"], e_ref); rec["E"] = max(rec["E"], E)
        rec["largest_ratio_to_bound"] = max(rec["largest_ratio_to_bound"], worst); rec["largest_error"] = max(rec["largest_error"], own)
        assert bool((err[~nz] == 0).all())
        assert worst <= 1.0


# --------------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("kind", RANGE_KINDS)
@pytest.mark.parametrize("shape", BWD_SHAPES)
def test_backward_has_the_bits_of_the_float32_twin(ft, dev, kind, shape, dtype, act, monkeypatch):
    monkeypatch.setenv("FTR_PRUNE_SEG", "16")
    g, y, ranges, d_am, d_lm = jc.bwd_case(ft, dev, shape, kind, dtype, act)
    if act == "relu":
        assert bool((y == 0).any()) and bool((y > 0).any())
    want_am, want_lm = jc._bwd_f32_twin(ft, jc.dz_float32(g, y, act), ranges, shape)
    assert torch.equal(d_am, want_am.to(dtype)) and torch.equal(d_lm, want_lm.to(dtype))
    if dtype != torch.float32 and shape == SCALAR_SHAPE:
        # g, y and both results at an odd element: element by element, as the float twin runs at C % 4 != 0
        d_am, d_lm = jc.act_backward(ft, g, y, ranges, shape, act, odd=True)
        assert torch.equal(d_am, want_am.to(dtype)) and torch.equal(d_lm, want_lm.to(dtype))


def _check_against_float64(got_am, got_lm, g, y, ranges, shape, act):
    dtype = g.dtype
    worst = 0.0
    sums = jc.segment_sums_float64(jc.dz_float64(g, y, act), g.double().abs(), ranges, shape)
    for what, got, (want, n, sabs) in zip(("d_am", "d_lm"), (got_am, got_lm), sums):
        assert not torch.isnan(got).any(), what
        err = (got.double() - want).abs()
        bound = jc.bwd_bound(want, n, sabs, dtype)
        exact = (bound == 0)                                  # rows nobody selects: exact zeros
        assert bool((err[exact] == 0).all()), what
        ratio = float((err[~exact] / bound[~exact]).max()) if bool((~exact).any()) else 0.0
        print(f"{what} {act} {_name(dtype)} {shape}: largest |got - want| / bound = {ratio:.4f}")
        worst = max(worst, ratio)
    key = f"{_name(dtype)}/{act}"
    _REPORT["backward_largest_ratio_to_bound"][key] = max(_REPORT["backward_largest_ratio_to_bound"].get(key, 0.0), worst)
    return worst


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("kind", RANGE_KINDS)
@pytest.mark.parametrize("shape", BWD_SHAPES)
def test_backward_against_float64_segment_sums(ft, dev, kind, shape, dtype, act, monkeypatch):
    monkeypatch.setenv("FTR_PRUNE_SEG", "16")
    g, y, ranges, d_am, d_lm = jc.bwd_case(ft, dev, shape, kind, dtype, act)
    assert _check_against_float64(d_am, d_lm, g, y, ranges, shape, act) <= 1.0
    if dtype != torch.float32 and shape == SEG_SHAPES[0]:
        d_am, d_lm = jc.act_backward(ft, g, y, ranges, shape, act, odd=True)   # C % 4 == 0 at an odd element: element by element
        assert _check_against_float64(d_am, d_lm, g, y, ranges, shape, act) <= 1.0


# --------------------------------------------------------------------------------------------------------------- autograd
def _leaves(shape, dtype, dev, seed):
    B, T, S1, C, r = shape
    gen = torch.Generator(device="cpu").manual_seed(seed)
    am = torch.randn((B, T, C), generator=gen).to(dtype).to(dev).requires_grad_(True)
    lm = torch.randn((B, S1, C), generator=gen).to(dtype).to(dev).requires_grad_(True)
    return am, lm


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("kind", ["flat_then_steep", "half_garbage"])
def test_autograd_bfloat16(ft, dev, kind, act, monkeypatch):
    monkeypatch.setenv("FTR_PRUNE_SEG", "16")
    shape = SEG_SHAPES[0]
    B, T, S1, C, r = shape
    ranges, w = jc._seg_case(shape, kind)
    ranges = ranges.to(dev); g = w.to(torch.bfloat16).to(dev)
    am, lm = _leaves(shape, torch.bfloat16, dev, 37)
    y = ft.do_rnnt_pruning_act(am, lm, ranges, activation=act)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (B, T, r, C) and y.is_contiguous()
    y.backward(g)
    assert am.grad.dtype == torch.bfloat16 and lm.grad.dtype == torch.bfloat16
    assert am.grad.shape == am.shape and lm.grad.shape == lm.shape
    want_am, want_lm = jc.act_backward(ft, g, y.detach(), ranges, shape, act)
    assert torch.equal(am.grad, want_am) and torch.equal(lm.grad, want_lm)
    # a non-contiguous am (a slice of a wider tensor) and a non-contiguous upstream gradient: the bits of their contiguous copies
    wide = torch.zeros((B, T, 2 * C), dtype=torch.bfloat16, device=dev)
    wide[:, :, :C] = am.detach()
    am_s = wide[:, :, :C].requires_grad_(True)
    g_t = g.transpose(1, 2).contiguous().transpose(1, 2)
    assert not am_s.is_contiguous() and not g_t.is_contiguous()
    lm2 = lm.detach().clone().requires_grad_(True)
    y2 = ft.do_rnnt_pruning_act(am_s, lm2, ranges, activation=act)
    assert torch.equal(y2, y)
    y2.backward(g_t)
    assert torch.equal(am_s.grad, want_am) and torch.equal(lm2.grad, want_lm) and am_s.grad.shape == am_s.shape
    # the node keeps its output: changing it in place before the backward is caught
    y3 = ft.do_rnnt_pruning_act(am, lm, ranges, activation=act)
    y3.mul_(2)
    with pytest.raises(RuntimeError):
        y3.backward(g)


def test_autograd_float32_relu_equals_the_unfused_pair(ft, dev, monkeypatch):
    monkeypatch.setenv("FTR_PRUNE_SEG", "16")
    shape = SEG_SHAPES[0]
    ranges, w = jc._seg_case(shape, "owner_conflict")
    ranges = ranges.to(dev); w = w.to(dev)
    a1, l1 = _leaves(shape, torch.float32, dev, 41)
    a2, l2 = _leaves(shape, torch.float32, dev, 41)
    y1 = ft.do_rnnt_pruning_act(a1, l1, ranges, activation="relu")
    y2 = torch.relu(ft.do_rnnt_pruning_sum(a2, l2, ranges))
    assert torch.equal(y1, y2)
    y1.backward(w); y2.backward(w)
    assert torch.equal(a1.grad, a2.grad) and torch.equal(l1.grad, l2.grad)


def test_autograd_float32_tanh_is_close_to_the_unfused_pair(ft, dev, monkeypatch):
    """Not bits: torch's tanh rounds elsewhere and its backward may contract.  The bound of the float64 test, with the unfused
    pair's gradients in the place of the float64 sums."""
    monkeypatch.setenv("FTR_PRUNE_SEG", "16")
    shape = SEG_SHAPES[0]
    B, T, S1, C, r = shape
    ranges, w = jc._seg_case(shape, "owner_conflict")
    ranges = ranges.to(dev); w = w.to(dev)
    a1, l1 = _leaves(shape, torch.float32, dev, 41)
    a2, l2 = _leaves(shape, torch.float32, dev, 41)
    ft.do_rnnt_pruning_act(a1, l1, ranges, activation="tanh").backward(w)
    torch.tanh(ft.do_rnnt_pruning_sum(a2, l2, ranges)).backward(w)
    zero = torch.zeros((B, T, r, C), dtype=torch.float64, device=dev)
    (_, n_am, abs_am), (_, n_lm, abs_lm) = jc.segment_sums_float64(zero, w.double().abs(), ranges, shape)
    for got, want, n, sabs in ((a1.grad, a2.grad, n_am, abs_am), (l1.grad, l2.grad, n_lm, abs_lm)):
        err = (got.double() - want.double()).abs()
        bound = jc.bwd_bound(want.double(), n, sabs, torch.float32)
        assert bool((err <= bound).all())


def test_refusals(ft, dev):
    B, T, S1, C, r = 2, 5, 4, 8, 2
    am = torch.zeros((B, T, C), device=dev); lm = torch.zeros((B, S1, C), device=dev)
    ranges = torch.zeros((B, T, r), dtype=torch.int32, device=dev)
    with pytest.raises(TypeError):
        ft.do_rnnt_pruning_act(am.bfloat16(), lm, ranges)
    with pytest.raises(TypeError):
        ft.do_rnnt_pruning_act(am.double(), lm.double(), ranges)
    for bad in ("gelu", "TANH", "", None, 1):
        with pytest.raises(ValueError):
            ft.do_rnnt_pruning_act(am, lm, ranges, activation=bad)
    with pytest.raises(ValueError):
        ft.do_rnnt_pruning_act(am[0], lm, ranges)                 # wrong rank
    with pytest.raises(ValueError):
        ft.do_rnnt_pruning_act(am, lm, ranges[0])
    with pytest.raises(ValueError):
        ft.do_rnnt_pruning_act(am[:1], lm, ranges)                # inconsistent shapes
    with pytest.raises(ValueError):
        ft.do_rnnt_pruning_act(am[:, :4], lm, ranges)
    with pytest.raises(ValueError):
        ft.do_rnnt_pruning_act(am[:, :, :4], lm, ranges)
    with pytest.raises(Exception) as e:
        ft.do_rnnt_pruning_act(am.cpu(), lm, ranges)
    with pytest.raises(type(e.value)):                 # the package's usual error for a tensor that is not on the GPU
        ft.do_rnnt_pruning_sum(am.cpu(), lm, ranges)
    for act in ACTS:
        assert ft.do_rnnt_pruning_act(am, lm, ranges.long(), activation=act).shape == (B, T, r, C)      # ranges: converted to int32


def _step(ft, am, lm, ranges, w, act):
    am.grad = None; lm.grad = None
    y = ft.do_rnnt_pruning_act(am, lm, ranges, activation=act)
    (y.float() * w).sum().backward()
    return y.detach().clone(), am.grad.clone(), lm.grad.clone()


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_two_runs_give_identical_bits(ft, dev, dtype, act, monkeypatch):
    monkeypatch.setenv("FTR_PRUNE_SEG", "16")
    shape = SEG_SHAPES[2]
    ranges, w = jc._seg_case(shape, "half_garbage")
    ranges = ranges.to(dev); w = w.to(dev)
    am, lm = _leaves(shape, dtype, dev, 43)
    first, second = _step(ft, am, lm, ranges, w, act), _step(ft, am, lm, ranges, w, act)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


@pytest.mark.parametrize("act", ACTS)
def test_graph_capture_replays_the_eager_bits(ft, dev, act):
    """Forward plus backward are kernels only: one capture, replayed twice with new values in the static inputs."""
    shape = (2, 40, 20, 24, 5)
    B, T, S1, C, r = shape
    gen = torch.Generator(device="cpu").manual_seed(47)
    s0 = torch.sort(torch.randint(0, S1 - r + 1, (B, T), generator=gen), dim=1).values
    ranges = (s0.unsqueeze(2) + torch.arange(r)).to(torch.int32).to(dev)
    draw = lambda *s: torch.randn(s, generator=gen).to(torch.bfloat16).to(dev)
    am = draw(B, T, C).requires_grad_(True); lm = draw(B, S1, C).requires_grad_(True)
    w = torch.randn((B, T, r, C), generator=gen).to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # warm up off the capture, as tests/test_gpu_graph.py does
        for _ in range(2):
            _step(ft, am, lm, ranges, w, act)
    torch.cuda.current_stream().wait_stream(side)
    am.grad = None; lm.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = ft.do_rnnt_pruning_act(am, lm, ranges, activation=act)
        (y.float() * w).sum().backward()
    for _ in range(2):
        new_am, new_lm, new_w = draw(B, T, C), draw(B, S1, C), torch.randn((B, T, r, C), generator=gen).to(dev)
        with torch.no_grad():
            am.copy_(new_am); lm.copy_(new_lm); w.copy_(new_w)
        graph.replay()
        torch.cuda.synchronize()
        got = (y.detach().clone(), am.grad.clone(), lm.grad.clone())
        am2 = new_am.clone().requires_grad_(True); lm2 = new_lm.clone().requires_grad_(True)
        want = _step(ft, am2, lm2, ranges, new_w, act)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
