"""The band-native multi-blank loss on the GPU (the multi-blank domain of csrc/mi_band_tdt.hip, the band-shaped mb_* kernels
of csrc/pruned_logprobs.hip, include/ftr_band_multiblank.h): the recursion on band-shaped operands against the float64
restatement of tests/multiblank_restatement.py on the band scattered into full-size lattices, the two routes of
rnnt_loss_multiblank_pruned against the restatement, and the band-shaped builders against their lattice twins bit for bit.
The tolerance is the project's: normwise max|d| / max|ref| <= 1e-4, helpers.max_rel asserting the same -inf pattern.

Inputs are made on the CPU (tests/band_multiblank_cases.py).  A band is drawn around a random path of the case's own moves,
so every reference loss is finite, with two exceptions that are stated where they occur: the designated no-path test, and
the recursion shape (B,S,T,r) = (2,5,1,4), which cannot have a path whatever the seed: all five symbols must be emitted on
its single frame, that is rows 0..5 (0..4 under the boundary), and a band holds 4 rows of a frame.  Whether a path exists
is decided by the planter's reachability count alone, never by the values; where none exists the reference is -inf with
zero occupancies, and the recursion must say the same."""
import ctypes

import numpy as np
import pytest
import torch

import band_multiblank_cases as MC
from band_tdt_cases import _gather, _scatter
from helpers import max_rel
from multiblank_restatement import multiblank_loss
from test_gpu_graph import _capture
from test_gpu_multiblank import BIG_BLANKS, LOSS_SHAPES, _big, _loss_inputs, _loss_reference

pytestmark = pytest.mark.gpu

TOL_F64 = 1e-4
NEG = float("-inf")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _n(t):
    return t.detach().cpu().numpy()


def _run_recursion(ft, dev, pxb, pyb, ranges, durations, bd, S, weights=None, grads=True):
    x, y = _t(pxb, dev).requires_grad_(grads), _t(pyb, dev).requires_grad_(grads)
    ans = ft.mutual_information_recursion_multiblank_band(x, y, _t(ranges, dev), durations, None if bd is None else _t(bd, dev), S=S)
    if not grads:
        return _n(ans)
    (ans * weights).sum().backward() if weights is not None else ans.sum().backward()
    return _n(ans), _n(x.grad), _n(y.grad)


# ---------------------------------------------------------------------------------------- recursion against restatement
@pytest.mark.parametrize("with_boundary", [False, True], ids=["full", "subrect"])
@pytest.mark.parametrize("durations", MC.RECURSION_DURATIONS, ids=str)
@pytest.mark.parametrize("shape", MC.RECURSION_SHAPES, ids=str)
def test_recursion_matches_restatement(ft, dev, shape, durations, with_boundary):
    pxb, pyb, ranges, bd, has_path, (w_ans, w_gx, w_gy) = MC.recursion_case(shape, durations, with_boundary)
    assert has_path or shape == MC.ONE_FRAME
    if has_path:
        assert np.isfinite(w_ans).all(), "the inputs of a parity case must leave every utterance a path"
    else:
        assert (w_ans == NEG).all() and not w_gx.any() and not w_gy.any()
    ans, gx, gy = _run_recursion(ft, dev, pxb, pyb, ranges, durations, bd, shape[1])
    assert gx.shape == pxb.shape and gy.shape == pyb.shape
    e = (max_rel(ans, w_ans), max_rel(gx, w_gx), max_rel(gy, w_gy))
    print(f"band multiblank recursion {shape} {durations} boundary={with_boundary}: ans {e[0]:.3g} gx_band {e[1]:.3g} gy_band {e[2]:.3g}")
    assert max(e) <= TOL_F64, e
    # the forward-only launch (one chain, no occupancies) has the bits of the launch with gradients
    assert _run_recursion(ft, dev, pxb, pyb, ranges, durations, bd, shape[1], grads=False).tobytes() == ans.tobytes()


def test_recursion_autograd_scales_by_upstream(ft, dev):
    shape, durations = (3, 12, 40, 4), (1, 2, 4, 8)
    pxb, pyb, ranges, bd, _, (w_ans, w_gx, w_gy) = MC.recursion_case(shape, durations, True)
    w = torch.tensor([0.5, -2.0, 3.0], device=dev)
    before = ft._lib.band_multiblank_recursions
    ans, gx, gy = _run_recursion(ft, dev, pxb, pyb, ranges, durations, bd, shape[1], weights=w)
    assert ft._lib.band_multiblank_recursions == before + 1
    assert max_rel(ans, w_ans) <= TOL_F64
    assert max_rel(gx, w_gx * _n(w)[:, None, None]) <= TOL_F64
    assert max_rel(gy, w_gy * _n(w)[:, None, None, None]) <= TOL_F64
    # without S the last band row stands for it (one host read): the same lattice here, the same bits
    x, y = _t(pxb, dev), _t(pyb, dev)
    a0 = ft.mutual_information_recursion_multiblank_band(x, y, _t(ranges, dev), durations, _t(bd, dev), S=shape[1])
    a1 = ft.mutual_information_recursion_multiblank_band(x, y, _t(ranges, dev), durations, _t(bd, dev))
    assert int(ranges.max()) == shape[1] and _n(a0).tobytes() == _n(a1).tobytes() == ans.tobytes()


def test_recursion_value_errors(ft, dev):
    x, y = torch.zeros(1, 4, 3, device=dev), torch.zeros(1, 2, 4, 3, device=dev)
    rg = torch.arange(3, dtype=torch.int32, device=dev).expand(1, 4, 3).contiguous()
    f = ft.mutual_information_recursion_multiblank_band
    assert torch.isfinite(f(x, y, rg, (1, 2), S=2)).all()
    for durations in ((), (1, 33), (0, 1), (2, 2), (2, 1), (1,), (1, 2, 3)):            # the last two: not py_band's D
        with pytest.raises(ValueError):
            f(x, y, rg, durations, S=2)
    with pytest.raises(ValueError):             # D = 9
        f(x, torch.zeros(1, 9, 4, 3, device=dev), rg, tuple(range(1, 10)), S=2)
    with pytest.raises(ValueError):             # ranges of another length
        f(x, y, rg[:, :3], (1, 2), S=2)
    with pytest.raises(ValueError):             # px_band with a move axis, as the TDT recursion takes it
        f(x[:, None], y, rg, (1, 2), S=2)
    with pytest.raises(ValueError):
        f(x, y[:, :, :3], rg, (1, 2), S=2)
    with pytest.raises(ValueError):
        f(x, y, rg, (1, 2), S=-1)
    with pytest.raises(TypeError):
        f(x.half(), y.half(), rg, (1, 2), S=2)
    with pytest.raises(TypeError):
        f(x.double(), y.double(), rg, (1, 2), S=2)
    wide = torch.arange(16, dtype=torch.int32, device=dev).expand(1, 4, 16).contiguous()
    with pytest.raises(ValueError):             # r = 16 is outside the band kernels
        f(torch.zeros(1, 4, 16, device=dev), torch.zeros(1, 2, 4, 16, device=dev), wide, (1, 2), S=15)


def test_decreasing_band_is_answered_with_nan(ft, dev):
    """As ftr_mutual_information_band_f32: two cells would share a slot.  Its batch neighbour is what it is without it."""
    shape, durations = (2, 33, 70, 5), (1, 2, 4, 8)
    pxb, pyb, ranges, _, _, _ = MC.recursion_case(shape, durations, False)
    bad = ranges.copy()
    t = int(np.argmax(bad[1, :, 0] > 0))
    bad[1, t + 1:t + 3] = bad[1, t] - 1
    ans0, gx0, gy0 = _run_recursion(ft, dev, pxb, pyb, ranges, durations, None, shape[1])
    ans, gx, gy = _run_recursion(ft, dev, pxb, pyb, bad, durations, None, shape[1])
    assert np.isnan(ans[1]) and not gx[1].any() and not gy[1].any()
    assert ans[0].tobytes() == ans0[0].tobytes() and gx[0].tobytes() == gx0[0].tobytes() and gy[0].tobytes() == gy0[0].tobytes()


# ------------------------------------------------------------------------------------------------------------ builders
# C = 512 takes the vector path of the gradient kernel, the others the scalar one.  A vocabulary of 6 columns holds the
# blank, at most three big blanks and two symbols, so (C, D) = (6, 8) does not exist; every other pair is here.
BUILDER_CD = [(C, D) for C in (6, 13, 507, 512) for D in (1, 2, 4, 8) if D + 2 <= C]


@pytest.mark.parametrize("r", [1, 2, 5, 7, 8, 15])               # one band row, two, and the widest bands of 8 and 16 lanes
@pytest.mark.parametrize("CD", BUILDER_CD, ids=str)
def test_band_builders_are_bit_identical_to_the_lattice_ones(ft, dev, CD, r):
    """px_band / py_band are the lattice builder's values at the band cells; d logits of the band gradient kernel fed the
    occupancies gathered at the band cells is that of the lattice kernel fed the same occupancies scattered (zero
    elsewhere), per-utterance scale and scale_mul included.  A symbol equal to a big-blank id and one equal to the blank;
    utterance 1's boundary ends ten frames before T, so py_j's rule t + d_j > t_end bites for every j of the list
    (durations up to 8 with T = 24) and px's t == t_end as well; sigma = 0.05, delay penalty 0.1."""
    C, D = CD
    durs = (1, 2, 3, 4, 5, 6, 7, 8)[:D] if D != 4 else (1, 2, 4, 8)
    B, T, S, blank = 2, 24, max(9, r + 1), 1
    assert S + 1 - r >= 2
    rng = np.random.default_rng([C, r, D])
    ids = [0, C - 1, C // 2, 2, 3, 4, 5][:D - 1]
    assert blank not in ids and len(set(ids)) == len(ids)
    logits = _t((rng.standard_normal((B, T, r, C)) * 2).astype(np.float32), dev)
    others = np.array([c for c in range(C) if c != blank and c not in ids])
    sym_np = others[rng.integers(0, len(others), (B, S))].astype(np.int32)
    if ids:
        sym_np[0, 2] = ids[len(ids) // 2]            # a symbol that is a big blank: px = -inf, no gradient
    sym_np[1, 0] = blank
    s0 = np.sort(rng.integers(0, S - r + 2, (B, T)), axis=1)
    ranges_np = (s0[..., None] + np.arange(r)).astype(np.int32)
    bd_np = np.array([[0, 0, S, T], [0, 0, S - 1, T - 10]], np.int32)
    sym, ranges, bd = _t(sym_np, dev), _t(ranges_np, dev), _t(bd_np, dev)
    id_arr, dur_arr = (ctypes.c_int32 * max(D - 1, 1))(*ids), (ctypes.c_int32 * D)(*durs)
    p = lambda t: t.data_ptr()
    st = torch.cuda.current_stream(dev).cuda_stream
    f32 = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device=dev)
    ll, px, py = f32(B, T, r), f32(B, S, T + 1), f32(B, D, S + 1, T)
    bl, pxb, pyb = f32(B, T, r), f32(B, T, r), f32(B, D, T, r)
    ft._lib.call("ftr_multiblank_pruned_logprobs_fwd_f32", p(logits), p(sym), p(ranges), p(bd), blank, id_arr, dur_arr, D, 0.05,
                 0.1, p(ll), p(px), p(py), B, T, S, C, r, st)
    ft._lib.call("ftr_multiblank_pruned_band_fwd_f32", p(logits), p(sym), p(ranges), p(bd), blank, id_arr, dur_arr, D, 0.05, 0.1,
                 p(bl), p(pxb), p(pyb), B, T, S, C, r, st)
    assert _n(bl).tobytes() == _n(ll).tobytes()
    want_x, want_y = _gather(_n(px)[:, None], ranges_np)[:, 0], _gather(_n(py), ranges_np)
    want_x[ranges_np >= S] = NEG                                         # row S has no symbol: no px there
    assert _n(pxb).tobytes() == want_x.tobytes() and _n(pyb).tobytes() == want_y.tobytes()
    assert np.isfinite(want_x).any() and np.isfinite(want_y).all(axis=(2, 3)).any()
    if ids:
        assert (want_x[0][ranges_np[0] == 2] == NEG).all()
    te1 = int(bd_np[1, 3])
    for j, d in enumerate(durs):                                          # the rule bites, and only where it should
        assert (want_y[1, j, te1 - d + 1:] == NEG).all() and np.isfinite(want_y[1, j, :te1 - d + 1]).all()
    gxb_np = rng.random((B, T, r)).astype(np.float32)
    gyb_np = rng.random((B, D, T, r)).astype(np.float32)
    gx_np, gy_np = _scatter(gxb_np[:, None], ranges_np, S, S, T + 1)[:, 0], _scatter(gyb_np, ranges_np, S, S + 1, T)
    gx_np[~np.isfinite(gx_np)] = 0.0
    gy_np[~np.isfinite(gy_np)] = 0.0
    scale = _t(np.array([0.5, -1.5], np.float32), dev)
    gx, gy, gxb, gyb = _t(gx_np, dev), _t(gy_np, dev), _t(gxb_np, dev), _t(gyb_np, dev)     # alive until the synchronisation
    g_lat, g_band = f32(B, T, r, C), f32(B, T, r, C)
    ft._lib.call("ftr_multiblank_pruned_logprobs_bwd_scaled_f32", p(logits), p(sym), p(ranges), p(bd), blank, id_arr, dur_arr, D,
                 p(ll), p(gx), p(gy), p(scale), 1, 0.25, p(g_lat), B, T, S, C, r, st)
    ft._lib.call("ftr_multiblank_pruned_band_bwd_scaled_f32", p(logits), p(sym), p(ranges), p(bd), blank, id_arr, dur_arr, D,
                 p(bl), p(gxb), p(gyb), p(scale), 1, 0.25, p(g_band), B, T, S, C, r, st)
    torch.cuda.synchronize()
    assert _n(g_band).any() and _n(g_band).tobytes() == _n(g_lat).tobytes()


# ------------------------------------------------------------------------------------------------------ route vs route
def _loss_step(ft, dev, logits_np, sym, ranges, blank, big, bd, reduction="none", weights=None, **kw):
    logits = _t(logits_np, dev).requires_grad_(True)
    loss = ft.rnnt_loss_multiblank_pruned(logits, _t(sym, dev), _t(ranges, dev), blank, big, None if bd is None else _t(bd, dev),
                                          reduction=reduction, **kw)
    (loss * _t(weights, dev)).sum().backward() if weights is not None else loss.sum().backward()
    return _n(loss), _n(logits.grad)


@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
@pytest.mark.parametrize("bb", BIG_BLANKS)
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=str)
def test_both_routes_match_the_restatement(ft, dev, monkeypatch, shape, bb, reduction):
    B, T, S, C, r = shape
    logits_np, sym, ranges, bd, blank = _loss_inputs(shape)
    per, grad = _loss_reference(shape, bb, 0.1)
    assert np.isfinite(per).all()
    w = np.array([0.7, 1.3, 0.9])[:B]
    if reduction == "none":
        want, want_g = per, grad * w[:, None, None, None]
    else:
        want = per.mean() if reduction == "mean" else per.sum()
        want_g = grad / B if reduction == "mean" else grad
    for route in ("band", "lattice"):
        if route == "lattice":
            monkeypatch.setenv("FTR_PRUNED_ROUTE", "lattice")
        else:
            monkeypatch.delenv("FTR_PRUNED_ROUTE", raising=False)
        before = ft._lib.band_multiblank_recursions
        loss, g = _loss_step(ft, dev, logits_np, sym, ranges, blank, _big(bb, C), bd, reduction,
                             w.astype(np.float32) if reduction == "none" else None, sigma=0.05, delay_penalty=0.1)
        assert ft._lib.band_multiblank_recursions - before == (1 if route == "band" else 0), route     # the route that was meant
        el, eg = max_rel(loss, want), max_rel(g, want_g)
        print(f"band multiblank loss {shape} {bb} {reduction} route={route}: loss {el:.3g} dlogits {eg:.3g}")
        assert el <= TOL_F64 and eg <= TOL_F64, (route, el, eg)


@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=str)
def test_band_route_without_big_blanks_is_the_ordinary_pruned_loss(ft, dev, monkeypatch, shape):
    monkeypatch.delenv("FTR_PRUNED_ROUTE", raising=False)
    B, T, S, C, r = shape
    logits_np, sym, ranges, bd, blank = _loss_inputs(shape)
    before = ft._lib.band_multiblank_recursions
    loss, g = _loss_step(ft, dev, logits_np, sym, ranges, blank, (), bd)
    assert ft._lib.band_multiblank_recursions == before + 1
    x = _t(logits_np, dev).requires_grad_(True)
    ref = ft.rnnt_loss_pruned(x, _t(sym, dev), _t(ranges, dev), blank, _t(bd, dev), reduction="none")
    ref.sum().backward()
    assert np.isfinite(loss).all()
    assert max_rel(loss, _n(ref)) <= TOL_F64 and max_rel(g, _n(x.grad)) <= TOL_F64


# --------------------------------------------------------------------------------------------------------- other cases
def test_band_that_never_reaches_the_end_gives_inf_and_zero_gradients(ft, dev):
    """The designated no-path case: utterance 1's band stays on rows 0..r-1 while s_end = 12, so no band cell has a move
    into the end cell.  Loss +inf, every gradient zero; utterance 0 and 2 as without it."""
    shape, big = LOSS_SHAPES[0], _big("three", LOSS_SHAPES[0][3])
    logits_np, sym, ranges, bd, blank = _loss_inputs(shape)
    stuck = ranges.copy()
    stuck[1] = np.arange(shape[4])
    assert bd[1, 2] > shape[4]
    per = multiblank_loss(torch.from_numpy(logits_np).double(), sym, stuck, blank, big, bd, 0.05, 0.0).numpy()
    assert per[1] == np.inf and np.isfinite(per[[0, 2]]).all()
    before = ft._lib.band_multiblank_recursions
    loss, g = _loss_step(ft, dev, logits_np, sym, stuck, blank, big, bd, sigma=0.05)
    assert ft._lib.band_multiblank_recursions == before + 1
    assert loss[1] == np.inf and not g[1].any() and np.isfinite(g).all()
    assert max_rel(loss, per) <= TOL_F64
    loss0, g0 = _loss_step(ft, dev, logits_np, sym, ranges, blank, big, bd, sigma=0.05)
    for b in (0, 2):
        assert loss[b].tobytes() == loss0[b].tobytes() and g[b].tobytes() == g0[b].tobytes()


def test_nan_stays_in_its_utterance(ft, dev):
    shape, big = LOSS_SHAPES[0], _big("three", LOSS_SHAPES[0][3])
    logits_np, sym, ranges, bd, blank = _loss_inputs(shape)
    poisoned = logits_np.copy()
    poisoned[1, 3, 0, 2] = np.nan
    before = ft._lib.band_multiblank_recursions
    loss0, g0 = _loss_step(ft, dev, logits_np, sym, ranges, blank, big, bd)
    loss, g = _loss_step(ft, dev, poisoned, sym, ranges, blank, big, bd)
    assert ft._lib.band_multiblank_recursions == before + 2
    assert np.isnan(loss[1])
    for b in (0, 2):
        assert loss[b].tobytes() == loss0[b].tobytes() and g[b].tobytes() == g0[b].tobytes()


def _float64_loss(logits_np, sym, ranges, blank, big, bd, sigma):
    l64 = torch.from_numpy(logits_np).double().requires_grad_(True)
    per = multiblank_loss(l64, sym, ranges, blank, big, bd, sigma, 0.0)
    per.sum().backward()
    return per.detach().numpy(), l64.grad.numpy()


def test_non_band_ranges_take_the_lattice_route(ft, dev):
    """One row of the ranges set back by one (the band start decreases there): silently the lattice route, and the
    restatement's loss and gradient all the same."""
    shape, big = LOSS_SHAPES[1], _big("three", LOSS_SHAPES[1][3])
    logits_np, sym, ranges, bd, blank = _loss_inputs(shape)
    back = ranges.copy()
    for b in range(shape[0]):
        t = next(t for t in range(5, bd[b, 3] - 1) if back[b, t, 0] == back[b, t - 1, 0] and back[b, t, 0] >= 1)
        back[b, t] -= 1
    per, grad = _float64_loss(logits_np, sym, back, blank, big, bd, 0.05)
    assert np.isfinite(per).all()
    before = ft._lib.band_multiblank_recursions
    loss, g = _loss_step(ft, dev, logits_np, sym, back, blank, big, bd, sigma=0.05)
    assert ft._lib.band_multiblank_recursions == before
    assert max_rel(loss, per) <= TOL_F64 and max_rel(g, grad) <= TOL_F64


def test_s_range_16_takes_the_lattice_route(ft, dev):
    B, T, S, C, r, big, blank = 2, 24, 17, 8, 16, ((1, 2), (2, 4)), 0
    rng = np.random.default_rng(16)
    logits_np = (rng.standard_normal((B, T, r, C)) * 2).astype(np.float32)
    sym = rng.integers(3, C, (B, S)).astype(np.int32)
    s0 = np.minimum(np.arange(T) * (S + 1 - r + 1) // T, S + 1 - r)
    ranges = np.broadcast_to((s0[:, None] + np.arange(r))[None], (B, T, r)).astype(np.int32).copy()
    per, grad = _float64_loss(logits_np, sym, ranges, blank, big, None, 0.0)
    assert np.isfinite(per).all()
    before = ft._lib.band_multiblank_recursions
    loss, g = _loss_step(ft, dev, logits_np, sym, ranges, blank, big, None)
    assert ft._lib.band_multiblank_recursions == before
    assert max_rel(loss, per) <= TOL_F64 and max_rel(g, grad) <= TOL_F64


def test_unpruned_loss_follows_through_identity_ranges(ft, dev):
    """rnnt_loss_multiblank: identity ranges are a band, so S + 1 <= 15 takes the band route and S + 1 = 16 the lattices."""
    for S1, calls in ((7, 1), (16, 0)):
        B, T, C, big = 2, 20, 12, ((1, 2), (2, 4))
        rng = np.random.default_rng(S1)
        joint = rng.standard_normal((B, T, S1, C)).astype(np.float32)
        sym = rng.integers(4, C, (B, S1 - 1)).astype(np.int32)
        bd = np.array([[0, 0, S1 - 1, T], [0, 0, S1 - 2, T - 3]], np.int32)
        ident = np.broadcast_to(np.arange(S1, dtype=np.int32), (B, T, S1)).copy()
        per, grad = _float64_loss(joint, sym, ident, 0, big, bd, 0.05)
        x = _t(joint, dev).requires_grad_(True)
        before = ft._lib.band_multiblank_recursions
        loss = ft.rnnt_loss_multiblank(x, _t(sym, dev), 0, big, _t(bd, dev), sigma=0.05, reduction="none")
        loss.sum().backward()
        assert ft._lib.band_multiblank_recursions == before + calls, S1
        assert max_rel(_n(loss), per) <= TOL_F64 and max_rel(_n(x.grad), grad) <= TOL_F64


# -------------------------------------------------------------------------------------------------------------- memory
def test_step_allocates_less_than_one_py_lattice(ft, dev):
    """B = 1, T = 1500, S = 300, r = 5, C = 16, big blanks of 2, 4, 8 frames: forward + backward stay below the size of ONE
    py lattice, B D (S+1) T 4 bytes = 7.2 MB.  The lattice route holds px, py, float64 p and both gradients, above 20 MB; the
    band route's tensors are of the order T r D 4 bytes plus the workspace ((S+T) lanes (D+1)) and the 480 KB gradient.
    Measured on MI355X: 1 141 760 bytes."""
    B, T, S, r, C, big, blank = 1, 1500, 300, 5, 16, ((13, 2), (14, 4), (15, 8)), 0
    D = 1 + len(big)
    rng = np.random.default_rng(1500)
    s0 = np.minimum(np.arange(T) * (S + 1) // T, S + 1 - r)
    ranges = _t(np.broadcast_to((s0[:, None] + np.arange(r))[None], (B, T, r)).astype(np.int32).copy(), dev)
    sym = _t(rng.integers(1, 13, (B, S)).astype(np.int32), dev)
    logits = _t(rng.standard_normal((B, T, r, C)).astype(np.float32), dev).requires_grad_(True)
    step = lambda: ft.rnnt_loss_multiblank_pruned(logits, sym, ranges, blank, big, None, reduction="sum")
    step().backward()                            # first use: the band verdict on the ranges, any lazy initialisation
    logits.grad = None
    torch.cuda.synchronize()
    before_calls = ft._lib.band_multiblank_recursions
    torch.cuda.reset_peak_memory_stats(dev)
    resident = torch.cuda.memory_allocated(dev)
    loss = step()
    loss.backward()
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated(dev) - resident
    one_py_lattice = B * D * (S + 1) * T * 4
    print(f"band multiblank step at T={T} S={S} r={r}: {used} bytes above the resident set, one py lattice = {one_py_lattice}")
    assert ft._lib.band_multiblank_recursions == before_calls + 1
    assert np.isfinite(_n(loss)) and np.isfinite(_n(logits.grad)).all() and _n(logits.grad).any()
    assert used < one_py_lattice, (used, one_py_lattice)


# ------------------------------------------------------------------------------------------- determinism and capture
def _step_fn(ft, dev, shape, bb):
    B, T, S, C, r = shape
    logits_np, sym, ranges, bd, blank = _loss_inputs(shape)
    buf = _t(logits_np, dev)
    symt, rgt, bdt = _t(sym, dev), _t(ranges, dev), _t(bd, dev)

    def step():
        x = buf.clone().requires_grad_(True)          # the leaf is created inside the step
        loss = ft.rnnt_loss_multiblank_pruned(x, symt, rgt, blank, _big(bb, C), bdt, sigma=0.05, delay_penalty=0.1,
                                              reduction="none")
        (g,) = torch.autograd.grad(loss.sum(), (x,))
        return loss.detach(), g.detach()              # only detached results leave it
    return buf, step


def test_two_band_route_steps_are_bit_identical(ft, dev, monkeypatch):
    monkeypatch.delenv("FTR_PRUNED_ROUTE", raising=False)
    _, step = _step_fn(ft, dev, LOSS_SHAPES[2], "three")
    step()
    before = ft._lib.band_multiblank_recursions
    a = [_n(v).copy() for v in step()]
    b = [_n(v).copy() for v in step()]
    assert ft._lib.band_multiblank_recursions == before + 2
    assert np.isfinite(a[0]).all()
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()


def test_band_route_step_replays_from_a_graph_with_new_values(ft, dev, monkeypatch):
    monkeypatch.delenv("FTR_PRUNED_ROUTE", raising=False)
    buf, step = _step_fn(ft, dev, LOSS_SHAPES[0], "three")
    before = ft._lib.band_multiblank_recursions
    g, out = _capture(step)                 # the warm-up steps settle the band verdict of the ranges outside the capture
    assert ft._lib.band_multiblank_recursions == before + 4, "the captured step must be a band-route step"
    for seed in (21, 22):
        buf.copy_(torch.randn(buf.shape, generator=torch.Generator().manual_seed(seed)).to(dev) * 2)
        g.replay()
        torch.cuda.synchronize()
        got = [_n(v).copy() for v in out]
        ref = [_n(v).copy() for v in step()]
        assert np.isfinite(got[0]).all()
        for u, v in zip(got, ref):
            assert u.tobytes() == v.tobytes()
