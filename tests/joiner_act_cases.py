"""Case builders and references shared by tests/test_gpu_joiner_act.py (do_rnnt_pruning_act, include/ftr_joiner_act.h).  The
shapes, range kinds and float32 twin are those of tests/test_gpu_prune_sum.py, imported from there."""
import functools

import torch

from test_gpu_prune_sum import (DTYPES, FWD_SHAPES, KIND, RANGE_KINDS, SCALAR_SHAPE, SEG_SHAPES, UNIT,   # noqa: F401
                                _at_odd_element, _bwd_f32_twin, _fwd_case, _name, _seg_case, _stream)

ACTS = ["tanh", "relu"]
ACT_CODE = {"tanh": 1, "relu": 2}                      # FTR_ACT_TANH, FTR_ACT_RELU
BWD_SHAPES = SEG_SHAPES + [SCALAR_SHAPE]
# sums planted into the tanh forward: am takes the value, the gathered lm element is 0
PLANTED = [0.0] + [s * v for v in (1e-30, 1e-4, 1e-2, 0.5, 9.0, 20.0, float("inf")) for s in (1.0, -1.0)] + [float("nan")]


def fwd_sum32(am, lm, ranges):
    """The float32 sum the activation is applied to: am[b,t,:] + lm[b, clamp(ranges[b,t,k]), :], one float32 addition."""
    B, T, r = ranges.shape
    bi = torch.arange(B, device=am.device).view(B, 1, 1).expand(B, T, r)
    rows = ranges.long().clamp(0, lm.shape[1] - 1)
    return am.float()[:, :, None, :] + lm.float()[bi, rows]


def plant(am, lm, ranges, values=PLANTED):
    """Writes values[i] into am[0, t, c] and 0 into the lm element that k = 0 of that frame gathers (t = i % T, c = i // T);
    returns the [(t, c)] list.  A value the dtype cannot hold (1e-30 in float16) becomes what the dtype rounds it to."""
    T = am.shape[1]
    where = []
    for i, v in enumerate(values):
        t, c = i % T, i // T
        row = int(ranges[0, t, 0].clamp(0, lm.shape[1] - 1))
        am[0, t, c] = v
        lm[0, row, c] = 0.0
        where.append((t, c))
    return where


def act_forward(ft, am, lm, ranges, act, odd=False):
    """ftr_pruned_joiner_act_dt through the C ABI, the output pre-filled with NaN bits; odd: all three tensors at an odd element."""
    B, T, r = ranges.shape
    S1, C = lm.shape[1], lm.shape[2]
    out = torch.full((B, T, r, C), float("nan"), dtype=am.dtype, device=am.device)
    if odd:
        am, lm, out = _at_odd_element(am), _at_odd_element(lm), _at_odd_element(out)
    ft._lib.call("ftr_pruned_joiner_act_dt", am.data_ptr(), lm.data_ptr(), KIND[am.dtype], ACT_CODE[act], ranges.data_ptr(),
                 out.data_ptr(), B, T, S1, C, r, _stream())
    return out


def act_backward(ft, g, y, ranges, shape, act, odd=False):
    """ftr_pruned_joiner_act_bwd_ws_dt; outputs pre-filled with NaN.  odd: g, y, d_am and d_lm at an odd element."""
    B, T, S1, C, r = shape
    dev = g.device
    d_am = torch.full((B, T, C), float("nan"), dtype=g.dtype, device=dev)
    d_lm = torch.full((B, S1, C), float("nan"), dtype=g.dtype, device=dev)
    if odd:
        g, y, d_am, d_lm = _at_odd_element(g), _at_odd_element(y), _at_odd_element(d_am), _at_odd_element(d_lm)
    nbytes = int(ft._lib.lib().ftr_do_pruning_bwd_workspace_bytes(B, T, S1, C, r))
    ws = torch.empty((nbytes + 3) // 4 + 4, device=dev)
    ft._lib.call("ftr_pruned_joiner_act_bwd_ws_dt", g.data_ptr(), y.data_ptr(), KIND[g.dtype], ACT_CODE[act], ranges.data_ptr(),
                 d_am.data_ptr(), d_lm.data_ptr(), B, T, S1, C, r, ws.data_ptr(), nbytes, _stream())
    return d_am, d_lm


def dz_float32(g, y, act):
    """dz as the definition forms it, by torch in float32: every operation a kernel of its own, so separately rounded."""
    gf, yf = g.float(), y.float()
    if act == "tanh":
        yy = yf * yf
        one_minus = 1.0 - yy
        return gf * one_minus
    return torch.where(yf <= 0, torch.zeros_like(gf), gf)


def dz_float64(g, y, act):
    gd, yd = g.double(), y.double()
    return gd * (1.0 - yd * yd) if act == "tanh" else torch.where(yd <= 0, torch.zeros_like(gd), gd)


@functools.lru_cache(maxsize=None)
def _inputs(shape, dtype):
    B, T, S1, C, r = shape
    gen = torch.Generator(device="cpu").manual_seed(53)
    return torch.randn((B, T, C), generator=gen).to(dtype), torch.randn((B, S1, C), generator=gen).to(dtype)


_BWD = {}


def bwd_case(ft, dev, shape, kind, dtype, act):
    """(g, y, ranges, d_am, d_lm) of one backward case: y from the forward on standard-normal am / lm, g the weights of
    tests/test_gpu_prune_sum.py in the dtype.  Computed once per case (with FTR_PRUNE_SEG as the caller has set it) and shared
    by the tests that look at it; nobody writes into these tensors."""
    key = (shape, kind, dtype, act)
    if key not in _BWD:
        ranges, w = _seg_case(shape, kind)
        ranges = ranges.to(dev)
        am, lm = _inputs(shape, dtype)
        y = act_forward(ft, am.to(dev), lm.to(dev), ranges, act)
        g = w.to(dtype).to(dev)
        _BWD[key] = (g, y, ranges) + act_backward(ft, g, y, ranges, shape, act)
    return _BWD[key]


def segment_sums_float64(dz, gabs, ranges, shape):
    """Independent of the project's kernels: (want, n, sum|g|) for d am and for d lm from a float64 dz and |g|."""
    B, T, S1, C, r = shape
    dev = dz.device
    idx = ranges.long()
    valid = (idx >= 0) & (idx < S1)
    bi = torch.arange(B, device=dev).view(B, 1, 1).expand(B, T, r)
    want_lm = torch.zeros((B, S1, C), dtype=torch.float64, device=dev)
    abs_lm = torch.zeros_like(want_lm)
    n_lm = torch.zeros((B, S1), dtype=torch.float64, device=dev)
    want_lm.index_put_((bi[valid], idx[valid]), dz[valid], accumulate=True)
    abs_lm.index_put_((bi[valid], idx[valid]), gabs[valid], accumulate=True)
    n_lm.index_put_((bi[valid], idx[valid]), torch.ones_like(idx[valid], dtype=torch.float64), accumulate=True)
    return (dz.sum(2), float(r), gabs.sum(2)), (want_lm, n_lm.unsqueeze(2), abs_lm)


def bwd_bound(want, n, sabs, dtype):
    """u |want| + (2n + 4) 2^-24 sum|g| (+ 2^-25 for float16): a float32 sum of n terms in any order (2n 2^-24 sum|dz|,
    |dz| <= |g|), three roundings in each dz (the one in y*y is absolute in 1 - y^2: at most 3 * 2^-24 |g| per term, taken
    as 4), one rounding into the dtype."""
    extra = 2.0 ** -25 if dtype == torch.float16 else 0.0
    return UNIT[dtype] * want.abs() + (2.0 * n + 4.0) * 2.0 ** -24 * sabs + extra


def ulp32(x):
    """The float32 spacing at the float64 values x (normal range)."""
    _, e = torch.frexp(x.abs())                          # |x| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(x), e - 24)


def tanh_budget(z32):
    """(E_ref, E) on the float32 sums z32: E_ref = the largest error of torch.tanh(z32) against the float64 tanh in float32
    ulps of the result, E = max(2 E_ref, 2) the budget of a second implementation."""
    want = torch.tanh(z32.double())
    ok = torch.isfinite(want) & (want != 0)
    e_ref = float(((torch.tanh(z32).double() - want).abs()[ok] / ulp32(want[ok])).max())
    return e_ref, max(2.0 * e_ref, 2.0)
