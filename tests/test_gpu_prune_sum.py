"""do_rnnt_pruning_sum (include/ftr_prune_sum.h, csrc/prune.hip): z[b,t,k,:] = am[b,t,:] + lm[b, ranges[b,t,k], :] in float32,
bfloat16 and float16, and its backward.

* forward: bit-exact against the float32 sum by torch indexing, rounded once into the dtype.
* backward: bit-exact against ftr_do_pruning_bwd_ws_f32 on float(g) given as both gradients, rounded once into the dtype
  (the definition: the float32 summation order of that call), over the shapes and ranges of
  tests/test_gpu_pipeline.py::test_do_pruning_backward_segments (direct rows, partial rows, the rescan, two column sweeps,
  the generic kernels at r = 17) and one C % 4 != 0 shape, where both sides run element by element.
* backward against float64 segment sums, independent of the project's kernels, per element within
      u |want| + 2 n 2^-24 sum|g|  (+ 2^-25 for float16)
  -- one rounding into the dtype (u = 2^-24, 2^-8, 2^-11) on top of a float32 sum of n terms in any order (the standard bound
  n 2^-24 sum|g| to first order, doubled), and half of float16's smallest subnormal, which a result near zero is rounded by.
  A 16-bit g at an odd element with C % 4 == 0 (no float twin has its order: element by element in (t,k) order) is checked here.
* autograd, refusals, reproducibility and one graph capture.

With FTR_PRUNE_SUM_PARITY_OUT set, the largest ratio to that bound per dtype is written to that file as JSON when the module
is done; a run on MI355X is committed as profiles/prune_sum_parity_errors.json."""
import functools
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
KIND = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
UNIT = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
FWD_SHAPES = [(2, 9, 7, 24, 5), (2, 9, 7, 520, 3), (2, 9, 7, 37, 1), (1, 6, 40, 16, 17)]
SEG_SHAPES = [(3, 150, 60, 24, 5), (2, 90, 50, 520, 3), (2, 64, 80, 40, 10), (1, 50, 90, 16, 17)]
SCALAR_SHAPE = (2, 30, 20, 37, 5)
RANGE_KINDS = ["flat_then_steep", "gaps", "half_garbage", "owner_conflict", "out_of_range"]
_RATIOS = {}


def _name(dtype):
    return str(dtype).replace("torch.", "")


@pytest.fixture(scope="module", autouse=True)
def _write_ratios():
    yield
    out = os.environ.get("FTR_PRUNE_SUM_PARITY_OUT")
    if out and _RATIOS:
        with open(out, "w") as f:
            json.dump({"bound": "u |want| + 2 n 2^-24 sum|g| (+ 2^-25 for float16), per element of d am and d lm",
                       "largest_ratio_to_bound": _RATIOS}, f, indent=1, sort_keys=True)
            f.write("\n")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _at_odd_element(t):
    """A contiguous copy of t whose first element sits at an odd element of its buffer (2-byte aligned only)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 4 == 2 or t.element_size() != 2
    return view


@functools.lru_cache(maxsize=None)
def _seg_case(shape, kind):
    """ranges (on the CPU, int32) and a float32 weight tensor w: those of test_do_pruning_backward_segments."""
    B, T, S1, C, r = shape
    g = torch.Generator(device="cpu").manual_seed(23)
    top = S1 - r
    if kind == "flat_then_steep":
        s0 = torch.zeros((B, T), dtype=torch.int64)
        s0 += torch.clamp((torch.arange(T) - (T - top // max(r - 1, 1) - 3)) * max(r - 1, 1), 0, top)
    elif kind == "gaps":
        s0 = torch.clamp(torch.cumsum((torch.rand((B, T), generator=g) < 0.1).long() * (r + 3), 1), 0, top)
    elif kind == "owner_conflict":
        s0 = torch.sort(torch.randint(0, top + 1, (B, T), generator=g), dim=1).values
        s0[:, T // 2:] = torch.sort(torch.randint(0, top + 1, (B, T - T // 2), generator=g), dim=1).values
    else:
        s0 = torch.sort(torch.randint(0, top + 1, (B, T), generator=g), dim=1).values
    ranges = (s0.unsqueeze(2) + torch.arange(r)).clone()
    if kind == "half_garbage":
        ranges[:, T // 2:] = torch.randint(0, S1, (B, T - T // 2, r), generator=g)
    w = torch.randn((B, T, r, C), generator=g)
    if kind == "out_of_range":
        ranges[:, 5:9] += S1; ranges[:, 20:22] -= 2 * S1
    return ranges.to(torch.int32), w


def _bwd_f32_twin(ft, gf, ranges, shape):
    """ftr_do_pruning_bwd_ws_f32 with the float32 tensor gf as both incoming gradients; outputs pre-filled with NaN."""
    B, T, S1, C, r = shape
    dev = gf.device
    d_am = torch.full((B, T, C), float("nan"), device=dev); d_lm = torch.full((B, S1, C), float("nan"), device=dev)
    nbytes = int(ft._lib.lib().ftr_do_pruning_bwd_workspace_bytes(B, T, S1, C, r))
    ws = torch.empty((nbytes + 3) // 4 + 4, device=dev)
    ft._lib.call("ftr_do_pruning_bwd_ws_f32", gf.data_ptr(), gf.data_ptr(), ranges.data_ptr(), d_am.data_ptr(), d_lm.data_ptr(),
                 B, T, S1, C, r, ws.data_ptr(), nbytes, _stream())
    return d_am, d_lm


def _bwd_sum(ft, g, ranges, shape, odd=False):
    """ftr_do_pruning_sum_bwd_ws_dt on g (any of the three dtypes); outputs pre-filled with NaN.  odd: g, d_am and d_lm at an
    odd element of their buffers."""
    B, T, S1, C, r = shape
    dev = g.device
    d_am = torch.full((B, T, C), float("nan"), dtype=g.dtype, device=dev)
    d_lm = torch.full((B, S1, C), float("nan"), dtype=g.dtype, device=dev)
    if odd:
        g, d_am, d_lm = _at_odd_element(g), _at_odd_element(d_am), _at_odd_element(d_lm)
    nbytes = int(ft._lib.lib().ftr_do_pruning_bwd_workspace_bytes(B, T, S1, C, r))
    ws = torch.empty((nbytes + 3) // 4 + 4, device=dev)
    ft._lib.call("ftr_do_pruning_sum_bwd_ws_dt", g.data_ptr(), KIND[g.dtype], ranges.data_ptr(), d_am.data_ptr(), d_lm.data_ptr(),
                 B, T, S1, C, r, ws.data_ptr(), nbytes, _stream())
    return d_am, d_lm


def _fwd_reference(am, lm, ranges):
    B, T, r = ranges.shape
    bi = torch.arange(B, device=am.device).view(B, 1, 1).expand(B, T, r)
    rows = ranges.long().clamp(0, lm.shape[1] - 1)
    return (am.float()[:, :, None, :] + lm.float()[bi, rows]).to(am.dtype)


def _fwd_case(shape, dtype, dev):
    B, T, S1, C, r = shape
    g = torch.Generator(device="cpu").manual_seed(31)
    am = torch.randn((B, T, C), generator=g).to(dtype).to(dev)
    lm = torch.randn((B, S1, C), generator=g).to(dtype).to(dev)
    ranges = torch.randint(0, S1, (B, T, r), generator=g).to(torch.int32)
    ranges[0, 1, 0] = -3; ranges[-1, T - 1, r - 1] = S1 + 2; ranges[0, 3, r // 2] = S1 + 2; ranges[-1, 2, 0] = -3
    return am, lm, ranges.to(dev)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("shape", FWD_SHAPES)
def test_forward_is_the_rounded_float32_sum(ft, dev, shape, dtype):
    am, lm, ranges = _fwd_case(shape, dtype, dev)
    want = _fwd_reference(am, lm, ranges)
    z = ft.do_rnnt_pruning_sum(am, lm, ranges)
    assert z.dtype == dtype and z.is_contiguous() and tuple(z.shape) == (shape[0], shape[1], shape[4], shape[3])
    assert torch.equal(z, want)
    if dtype == torch.float32:
        assert torch.equal(z, sum(ft.do_rnnt_pruning(am, lm, ranges)))
    else:
        # am, lm and the output at an odd element of their buffers: the element-by-element kernel, through the C ABI
        B, T, S1, C, r = shape
        a1, l1 = _at_odd_element(am), _at_odd_element(lm)
        out = _at_odd_element(torch.full((B, T, r, C), float("nan"), dtype=dtype, device=dev))
        ft._lib.call("ftr_do_pruning_sum_dt", a1.data_ptr(), l1.data_ptr(), KIND[dtype], ranges.data_ptr(), out.data_ptr(),
                     B, T, S1, C, r, _stream())
        assert torch.equal(out, want)


def test_forward_carries_nan_and_inf(ft, dev):
    B, T, S1, C, r = 1, 3, 4, 8, 2
    for dtype in DTYPES:
        am = torch.zeros((B, T, C), dtype=dtype, device=dev); lm = torch.ones((B, S1, C), dtype=dtype, device=dev)
        am[0, 0, 0] = float("inf"); am[0, 1, 1] = float("nan"); lm[0, 2, 2] = float("-inf"); lm[0, 2, 0] = float("-inf")
        ranges = torch.tensor([[[2, 3], [1, 2], [0, 2]]], dtype=torch.int32, device=dev)
        z = ft.do_rnnt_pruning_sum(am, lm, ranges)
        want = _fwd_reference(am, lm, ranges)
        assert torch.equal(torch.isnan(z), torch.isnan(want)) and torch.isnan(z[0, 0, 0, 0]) and torch.isnan(z[0, 1, :, 1]).all()
        assert torch.equal(z.nan_to_num(nan=7.0), want.nan_to_num(nan=7.0)) and z[0, 2, 1, 2] == float("-inf")


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("kind", RANGE_KINDS)
@pytest.mark.parametrize("shape", SEG_SHAPES + [SCALAR_SHAPE])
def test_backward_has_the_bits_of_the_float32_twin(ft, dev, kind, shape, dtype, monkeypatch):
    monkeypatch.setenv("FTR_PRUNE_SEG", "16")
    ranges, w = _seg_case(shape, kind)
    ranges = ranges.to(dev)
    g = w.to(dtype).to(dev)
    want_am, want_lm = _bwd_f32_twin(ft, g.float(), ranges, shape)
    d_am, d_lm = _bwd_sum(ft, g, ranges, shape)
    assert torch.equal(d_am, want_am.to(dtype)) and torch.equal(d_lm, want_lm.to(dtype))
    if dtype != torch.float32 and shape == SCALAR_SHAPE:
        # g and both results at an odd element: element by element, as the float twin runs at C % 4 != 0
        d_am, d_lm = _bwd_sum(ft, g, ranges, shape, odd=True)
        assert torch.equal(d_am, want_am.to(dtype)) and torch.equal(d_lm, want_lm.to(dtype))


def _check_against_float64(got_am, got_lm, g, ranges, shape):
    B, T, S1, C, r = shape
    dev = g.device
    dtype = g.dtype
    gd = g.double()
    idx = ranges.long()
    valid = (idx >= 0) & (idx < S1)
    bi = torch.arange(B, device=dev).view(B, 1, 1).expand(B, T, r)
    want_lm = torch.zeros((B, S1, C), dtype=torch.float64, device=dev)
    abs_lm = torch.zeros_like(want_lm)
    n_lm = torch.zeros((B, S1), dtype=torch.float64, device=dev)
    want_lm.index_put_((bi[valid], idx[valid]), gd[valid], accumulate=True)
    abs_lm.index_put_((bi[valid], idx[valid]), gd[valid].abs(), accumulate=True)
    n_lm.index_put_((bi[valid], idx[valid]), torch.ones_like(idx[valid], dtype=torch.float64), accumulate=True)
    extra = 2.0 ** -25 if dtype == torch.float16 else 0.0
    worst = 0.0
    for what, got, want, n, sabs in (("d_am", got_am, gd.sum(2), float(r), gd.abs().sum(2)),
                                     ("d_lm", got_lm, want_lm, n_lm.unsqueeze(2), abs_lm)):
        assert not torch.isnan(got).any(), what
        err = (got.double() - want).abs()
        bound = UNIT[dtype] * want.abs() + 2.0 * n * 2.0 ** -24 * sabs + extra
        exact = (bound == 0)                                  # rows nobody selects: exact zeros
        assert bool((err[exact] == 0).all()), what
        ratio = float((err[~exact] / bound[~exact]).max()) if bool((~exact).any()) else 0.0
        print(f"{what} {_name(dtype)} {shape}: largest |got - want| / bound = {ratio:.4f}")
        worst = max(worst, ratio)
    _RATIOS[_name(dtype)] = max(_RATIOS.get(_name(dtype), 0.0), worst)
    return worst


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("kind", RANGE_KINDS)
@pytest.mark.parametrize("shape", SEG_SHAPES + [SCALAR_SHAPE])
def test_backward_against_float64_segment_sums(ft, dev, kind, shape, dtype, monkeypatch):
    monkeypatch.setenv("FTR_PRUNE_SEG", "16")
    ranges, w = _seg_case(shape, kind)
    ranges = ranges.to(dev)
    g = w.to(dtype).to(dev)
    d_am, d_lm = _bwd_sum(ft, g, ranges, shape)
    assert _check_against_float64(d_am, d_lm, g, ranges, shape) <= 1.0
    if dtype != torch.float32 and shape == SEG_SHAPES[0]:
        d_am, d_lm = _bwd_sum(ft, g, ranges, shape, odd=True)        # C % 4 == 0 at an odd element: element by element
        assert _check_against_float64(d_am, d_lm, g, ranges, shape) <= 1.0


@pytest.mark.parametrize("kind", ["flat_then_steep", "half_garbage"])
def test_autograd_bfloat16(ft, dev, kind, monkeypatch):
    monkeypatch.setenv("FTR_PRUNE_SEG", "16")
    shape = SEG_SHAPES[0]
    B, T, S1, C, r = shape
    ranges, w = _seg_case(shape, kind)
    ranges = ranges.to(dev); w = w.to(dev)
    gen = torch.Generator(device="cpu").manual_seed(37)
    am = torch.randn((B, T, C), generator=gen).to(torch.bfloat16).to(dev).requires_grad_(True)
    lm = torch.randn((B, S1, C), generator=gen).to(torch.bfloat16).to(dev).requires_grad_(True)
    (ft.do_rnnt_pruning_sum(am, lm, ranges).float() * w).sum().backward()
    want_am, want_lm = _bwd_sum(ft, w.to(torch.bfloat16), ranges, shape)
    assert am.grad.dtype == torch.bfloat16 and lm.grad.dtype == torch.bfloat16
    assert torch.equal(am.grad, want_am) and torch.equal(lm.grad, want_lm)
    # a non-contiguous am (a transposed view): the result and the gradient of its .contiguous()
    am_t = am.detach().transpose(0, 1).contiguous().transpose(0, 1).requires_grad_(True)
    assert not am_t.is_contiguous()
    z = ft.do_rnnt_pruning_sum(am_t, lm, ranges)
    assert torch.equal(z, ft.do_rnnt_pruning_sum(am.detach(), lm.detach(), ranges))
    (z.float() * w).sum().backward()
    assert torch.equal(am_t.grad, want_am) and am_t.grad.shape == am_t.shape


def test_autograd_float32_equals_the_unfused_pair(ft, dev, monkeypatch):
    monkeypatch.setenv("FTR_PRUNE_SEG", "16")
    shape = SEG_SHAPES[0]
    B, T, S1, C, r = shape
    ranges, w = _seg_case(shape, "owner_conflict")
    ranges = ranges.to(dev); w = w.to(dev)
    gen = torch.Generator(device="cpu").manual_seed(41)
    am = torch.randn((B, T, C), generator=gen).to(dev); lm = torch.randn((B, S1, C), generator=gen).to(dev)
    a1, l1 = am.clone().requires_grad_(True), lm.clone().requires_grad_(True)
    a2, l2 = am.clone().requires_grad_(True), lm.clone().requires_grad_(True)
    z1 = ft.do_rnnt_pruning_sum(a1, l1, ranges)
    z2 = sum(ft.do_rnnt_pruning(a2, l2, ranges))
    assert torch.equal(z1, z2)
    z1.backward(w); z2.backward(w)
    assert torch.equal(a1.grad, a2.grad) and torch.equal(l1.grad, l2.grad)


def test_refusals(ft, dev):
    B, T, S1, C, r = 2, 5, 4, 8, 2
    am = torch.zeros((B, T, C), device=dev); lm = torch.zeros((B, S1, C), device=dev)
    ranges = torch.zeros((B, T, r), dtype=torch.int32, device=dev)
    with pytest.raises(TypeError):
        ft.do_rnnt_pruning_sum(am.bfloat16(), lm, ranges)
    with pytest.raises(TypeError):
        ft.do_rnnt_pruning_sum(am.double(), lm.double(), ranges)
    with pytest.raises(TypeError):
        ft.do_rnnt_pruning_sum(am.int(), lm.int(), ranges)
    with pytest.raises(ValueError):
        ft.do_rnnt_pruning_sum(am[:1], lm, ranges)
    with pytest.raises(ValueError):
        ft.do_rnnt_pruning_sum(am[:, :4], lm, ranges)
    with pytest.raises(Exception) as e:
        ft.do_rnnt_pruning_sum(am.cpu(), lm, ranges)
    with pytest.raises(type(e.value)):                 # the package's usual error for a tensor that is not on the GPU
        ft.do_rnnt_pruning(am.cpu(), lm, ranges)
    assert ft.do_rnnt_pruning_sum(am, lm, ranges.long()).shape == (B, T, r, C)      # ranges: converted to int32


def _step(ft, am, lm, ranges, w):
    am.grad = None; lm.grad = None
    z = ft.do_rnnt_pruning_sum(am, lm, ranges)
    (z.float() * w).sum().backward()
    return z.detach().clone(), am.grad.clone(), lm.grad.clone()


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_two_runs_give_identical_bits(ft, dev, dtype, monkeypatch):
    monkeypatch.setenv("FTR_PRUNE_SEG", "16")
    shape = SEG_SHAPES[2]
    B, T, S1, C, r = shape
    ranges, w = _seg_case(shape, "half_garbage")
    ranges = ranges.to(dev); w = w.to(dev)
    gen = torch.Generator(device="cpu").manual_seed(43)
    am = torch.randn((B, T, C), generator=gen).to(dtype).to(dev).requires_grad_(True)
    lm = torch.randn((B, S1, C), generator=gen).to(dtype).to(dev).requires_grad_(True)
    first, second = _step(ft, am, lm, ranges, w), _step(ft, am, lm, ranges, w)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


def test_graph_capture_replays_the_eager_bits(ft, dev):
    """Forward plus backward are kernels only: one capture, replayed with new values in the static inputs."""
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
            _step(ft, am, lm, ranges, w)
    torch.cuda.current_stream().wait_stream(side)
    am.grad = None; lm.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        z = ft.do_rnnt_pruning_sum(am, lm, ranges)
        (z.float() * w).sum().backward()
    new_am, new_lm, new_w = draw(B, T, C), draw(B, S1, C), torch.randn((B, T, r, C), generator=gen).to(dev)
    with torch.no_grad():
        am.copy_(new_am); lm.copy_(new_lm); w.copy_(new_w)
    graph.replay()
    torch.cuda.synchronize()
    got = (z.detach().clone(), am.grad.clone(), lm.grad.clone())
    am2 = new_am.clone().requires_grad_(True); lm2 = new_lm.clone().requires_grad_(True)
    want = _step(ft, am2, lm2, ranges, new_w)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
