"""The band-native TDT loss on the GPU (csrc/mi_band_tdt.hip, the band-shaped builders of csrc/tdt_logprobs.hip,
include/ftr_band_tdt.h): the recursion on band-shaped operands against the float64 restatement of tests/tdt_restatement.py
on the band scattered into full-size lattices, the two routes of rnnt_loss_tdt_pruned against the restatement and the
band-shaped builders against their lattice twins bit for bit.  The tolerance is the project's: normwise
max|d| / max|ref| <= 1e-4 (TOL_F64 of tests/test_gpu_tdt.py), helpers.max_rel asserting the same -inf pattern.

Inputs are made on the CPU.  A band is drawn around a random path of the case's own moves (so every utterance has a path
whatever the move list), as flat as that path allows: base steps 0..r where the path climbs, long flat stretches, steps
of exactly r where a token of duration >= 1 crosses them, and a ragged boundary with s_begin, t_begin > 0 in one utterance.
Every reference loss is finite, with two exceptions that are stated where they occur: the designated no-path test, and the
recursion shape (B,S,T,r) = (2,5,1,4), which cannot have a path whatever the seed: all S = 5 symbols must be emitted on
its single frame, that is rows 0..5, and a band holds 4 rows of a frame (with a boundary that shortens the climb to 4
rows, only a move list with a token of duration 1 reaches the end cell).  Whether a path exists there is decided by a
reachability count over the rectangle and the band width alone, never by the values; where none exists the reference
is -inf with zero occupancies, and the recursion must say the same."""
import functools

import numpy as np
import pytest
import torch

from band_tdt_cases import _band_around, _gather, _random_path, _scatter
from helpers import max_rel
from tdt_restatement import blank_durations_of, tdt_dp_with_grads, tdt_loss
from test_gpu_graph import _capture
from test_gpu_tdt import LOSS_DURATIONS, LOSS_SHAPES, _loss_inputs, _loss_reference

pytestmark = pytest.mark.gpu

TOL_F64 = 1e-4
NEG = float("-inf")

SHAPES = [(2, 0, 9, 1), (2, 5, 1, 4), (3, 12, 40, 4), (2, 33, 70, 5), (1, 6, 1100, 3), (2, 50, 200, 5), (2, 20, 30, 8),
          (2, 20, 30, 15)]                                     # (B, S, T, r)
MOVES = [((0,), (1,)), ((0, 1, 2, 3, 4), (1, 2, 3, 4)), ((1, 2), (1,)), ((0, 16), (3, 16)), ((0, 5, 6, 7), (1, 9))]
ONE_FRAME = (2, 5, 1, 4)     # rows 0..5 of its single frame do not fit a band of 4 rows: see the module docstring


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _n(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------- bands and operands
@functools.lru_cache(maxsize=None)
def _recursion_case(shape, moves, with_boundary):
    B, S, T, r = shape
    tok, blk = moves
    N, Ny = len(tok), len(blk)
    rng = np.random.default_rng(1000 * S + 10 * T + r + 7 * N + 3 * Ny + int(with_boundary))
    bd = np.zeros((B, 4), np.int64)
    bd[:, 2], bd[:, 3] = S, T
    if with_boundary:
        for b in range(B):                       # ragged ends; utterance 0 also begins inside the lattice
            bd[b] = [1 if (b == 0 and S >= 3) else 0, 2 if (b == 0 and T >= 6) else 0, S - (b % 2 if S >= 2 else 0),
                     T - 1 - b % 2 if T >= 3 else T]
    ranges = np.zeros((B, T, r), np.int64)
    pxb = rng.standard_normal((B, N, T, r)).astype(np.float32)
    pyb = rng.standard_normal((B, Ny, T, r)).astype(np.float32)
    pxb[rng.random(pxb.shape) < 0.02] = NEG
    pyb[rng.random(pyb.shape) < 0.02] = NEG
    has_path = True
    for b in range(B):
        sb, tb, se, te = (int(v) for v in bd[b])
        path = _random_path(rng, se - sb + 1, te - tb + 1, tok, blk, r)
        while path is None and with_boundary and te - 1 > tb + 1:      # a ragged end that the move list can land on
            te -= 1
            path = _random_path(rng, se - sb + 1, te - tb + 1, tok, blk, r)
        if path is None:
            te = int(bd[b, 3])
        bd[b, 3] = te
        has_path = has_path and path is not None
        lo = _band_around(rng, path or [], sb, tb, te, S, T, r)
        ranges[b] = lo[:, None] + np.arange(r)
        for s, t, m in path or []:               # the path's own moves stay finite
            k = sb + s - lo[tb + t]
            (pxb[b, m] if m < N else pyb[b, m - N])[tb + t, k] = rng.standard_normal()
        # the -inf rules of the builder at the band cells
        rows = ranges[b]                                                    # [T,r] lattice row of each band row
        tt = np.arange(T)[:, None]
        for i, e in enumerate(tok):
            pxb[b, i][(rows >= S) | (tt >= te) | (tt + e > te)] = NEG
        for j, d in enumerate(blk):
            pyb[b, j][np.broadcast_to(tt + d > te, rows.shape)] = NEG
    bdi = bd.astype(np.int32) if with_boundary else None
    px = _scatter(pxb, ranges, S, S, T + 1)
    py = _scatter(pyb, ranges, S, S + 1, T)
    w_ans, w_gx, w_gy = tdt_dp_with_grads(px, py, tok, blk, bdi)
    return pxb, pyb, ranges.astype(np.int32), bdi, has_path, (w_ans, _gather(w_gx, ranges), _gather(w_gy, ranges))


def _run_recursion(ft, dev, pxb, pyb, ranges, tok, blk, bd, S, weights=None):
    x, y = _t(pxb, dev).requires_grad_(True), _t(pyb, dev).requires_grad_(True)
    ans = ft.mutual_information_recursion_tdt_band(x, y, _t(ranges, dev), tok, blk, None if bd is None else _t(bd, dev), S=S)
    (ans * weights).sum().backward() if weights is not None else ans.sum().backward()
    return _n(ans), _n(x.grad), _n(y.grad)


# ---------------------------------------------------------------------------------------- recursion against restatement
@pytest.mark.parametrize("with_boundary", [False, True], ids=["full", "subrect"])
@pytest.mark.parametrize("moves", MOVES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_recursion_matches_restatement(ft, dev, shape, moves, with_boundary):
    tok, blk = moves
    pxb, pyb, ranges, bd, has_path, (w_ans, w_gx, w_gy) = _recursion_case(shape, moves, with_boundary)
    assert has_path or shape == ONE_FRAME
    if has_path:
        assert np.isfinite(w_ans).all(), "the inputs of a parity case must leave every utterance a path"
    else:
        assert (w_ans == NEG).all() and not w_gx.any() and not w_gy.any()
    ans, gx, gy = _run_recursion(ft, dev, pxb, pyb, ranges, tok, blk, bd, shape[1])
    assert gx.shape == pxb.shape and gy.shape == pyb.shape
    e = (max_rel(ans, w_ans), max_rel(gx, w_gx), max_rel(gy, w_gy))
    print(f"band tdt recursion {shape} {tok}/{blk} boundary={with_boundary}: ans {e[0]:.3g} gx_band {e[1]:.3g} gy_band {e[2]:.3g}")
    assert max(e) <= TOL_F64, e


def test_recursion_autograd_scales_by_upstream(ft, dev):
    shape, moves = (3, 12, 40, 4), ((0, 1, 2, 3, 4), (1, 2, 3, 4))
    pxb, pyb, ranges, bd, _, (w_ans, w_gx, w_gy) = _recursion_case(shape, moves, True)
    w = torch.tensor([0.5, -2.0, 3.0], device=dev)
    ans, gx, gy = _run_recursion(ft, dev, pxb, pyb, ranges, *moves, bd, shape[1], weights=w)
    assert max_rel(ans, w_ans) <= TOL_F64
    assert max_rel(gx, w_gx * _n(w)[:, None, None, None]) <= TOL_F64
    assert max_rel(gy, w_gy * _n(w)[:, None, None, None]) <= TOL_F64
    # without S the last band row stands for it (one host read): the same lattice here, the same bits
    x, y = _t(pxb, dev), _t(pyb, dev)
    a0 = ft.mutual_information_recursion_tdt_band(x, y, _t(ranges, dev), *moves, _t(bd, dev), S=shape[1])
    a1 = ft.mutual_information_recursion_tdt_band(x, y, _t(ranges, dev), *moves, _t(bd, dev))
    assert int(ranges.max()) == shape[1] and _n(a0).tobytes() == _n(a1).tobytes()


def test_recursion_value_errors(ft, dev):
    x, y = torch.zeros(1, 2, 4, 3, device=dev), torch.zeros(1, 1, 4, 3, device=dev)
    rg = torch.arange(3, dtype=torch.int32, device=dev).expand(1, 4, 3).contiguous()
    for tok, blk in (((), (1,)), ((0, 1), ()), ((1, 0), (1,)), ((0, 17), (1,)), ((0, 1), (0,)), ((0, 1), (17,)), ((0,), (1,))):
        with pytest.raises(ValueError):
            ft.mutual_information_recursion_tdt_band(x, y, rg, tok, blk, S=2)
    with pytest.raises(ValueError):
        ft.mutual_information_recursion_tdt_band(x, y, rg[:, :3], (0, 1), (1,), S=2)
    with pytest.raises(TypeError):
        ft.mutual_information_recursion_tdt_band(x.half(), y.half(), rg, (0, 1), (1,), S=2)
    wide = torch.arange(16, dtype=torch.int32, device=dev).expand(1, 4, 16).contiguous()
    with pytest.raises(ValueError):             # r = 16 is outside the band kernels
        ft.mutual_information_recursion_tdt_band(torch.zeros(1, 2, 4, 16, device=dev), torch.zeros(1, 1, 4, 16, device=dev), wide,
                                                 (0, 1), (1,), S=15)


def test_decreasing_band_is_answered_with_nan(ft, dev):
    """As ftr_mutual_information_band_f32: two cells would share a slot.  Its batch neighbour is what it is without it."""
    shape, moves = (2, 33, 70, 5), ((0, 1, 2, 3, 4), (1, 2, 3, 4))
    pxb, pyb, ranges, _, _, _ = _recursion_case(shape, moves, False)
    bad = ranges.copy()
    t = int(np.argmax(bad[1, :, 0] > 0))
    bad[1, t + 1:t + 3] = bad[1, t] - 1
    ans0, gx0, gy0 = _run_recursion(ft, dev, pxb, pyb, ranges, *moves, None, shape[1])
    ans, gx, gy = _run_recursion(ft, dev, pxb, pyb, bad, *moves, None, shape[1])
    assert np.isnan(ans[1]) and not gx[1].any() and not gy[1].any()
    assert ans[0].tobytes() == ans0[0].tobytes() and gx[0].tobytes() == gx0[0].tobytes() and gy[0].tobytes() == gy0[0].tobytes()


# ------------------------------------------------------------------------------------------------------ route vs route
def _loss_step(ft, dev, logits_np, sym, ranges, blank, durs, bd, **kw):
    logits = _t(logits_np, dev).requires_grad_(True)
    loss = ft.rnnt_loss_tdt_pruned(logits, _t(sym, dev), _t(ranges, dev), blank, durs, None if bd is None else _t(bd, dev),
                                   reduction="none", **kw)
    loss.sum().backward()
    return _n(loss), _n(logits.grad)


@pytest.mark.parametrize("durs", LOSS_DURATIONS, ids=str)
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=str)
def test_both_routes_match_the_restatement(ft, dev, monkeypatch, shape, durs):
    logits_np, sym, ranges, bd, blank = _loss_inputs(shape, len(durs))
    per, grad = _loss_reference(shape, durs, 0.1)
    assert np.isfinite(per).all()
    for route in ("band", "lattice"):
        if route == "lattice":
            monkeypatch.setenv("FTR_PRUNED_ROUTE", "lattice")
        else:
            monkeypatch.delenv("FTR_PRUNED_ROUTE", raising=False)
        before = ft._lib.band_tdt_recursions
        loss, g = _loss_step(ft, dev, logits_np, sym, ranges, blank, durs, bd, sigma=0.05, delay_penalty=0.1)
        assert ft._lib.band_tdt_recursions - before == (1 if route == "band" else 0), route     # the route that was meant
        el, eg = max_rel(loss, per), max_rel(g, grad)
        print(f"band tdt loss {shape} {durs} route={route}: loss {el:.3g} dlogits {eg:.3g}")
        assert el <= TOL_F64 and eg <= TOL_F64, (route, el, eg)


# ------------------------------------------------------------------------------------------------------------ builders
@pytest.mark.parametrize("CN", [(5, 3), (6, 5), (507, 5), (510, 2)], ids=str)      # C + N = 8, 11, 512, 512; C % 4 != 0 in all
def test_band_builders_are_bit_identical_to_the_lattice_ones(ft, dev, CN):
    _builders_are_bit_identical(ft, dev, CN, 5)


@pytest.mark.parametrize("CN", [(5, 3), (6, 5), (507, 5), (510, 2)], ids=str)
@pytest.mark.parametrize("r", [1, 2, 7, 8, 15])                  # one band row, two, and the widest bands of 8 and 16 lanes
def test_band_builders_are_bit_identical_at_every_band_width(ft, dev, CN, r):
    """The same at the other band widths (r = 5 keeps its name above)."""
    _builders_are_bit_identical(ft, dev, CN, r)


def _builders_are_bit_identical(ft, dev, CN, r):
    """px_band / py_band are the lattice builder's values at the band cells; d logits of the band gradient kernel fed the
    occupancies gathered at the band cells is that of the lattice kernel fed the same occupancies scattered (zero
    elsewhere), per-utterance scale included.  S = 9 as long as the band start has two rows to move over, r + 1 above."""
    import ctypes
    C, N = CN
    durs = {2: (0, 1), 3: (1, 2, 4), 5: (0, 1, 2, 3, 4)}[N]
    Ny = len(blank_durations_of(durs))
    B, T, S, blank = 2, 24, max(9, r + 1), 1
    assert S + 1 - r >= 2
    rng = np.random.default_rng(C + N if r == 5 else [C, N, r])
    logits = _t((rng.standard_normal((B, T, r, C + N)) * 2).astype(np.float32), dev)
    sym_np = rng.integers(0, C, (B, S)).astype(np.int32)
    sym_np[1, 0] = blank
    s0 = np.sort(rng.integers(0, S - r + 2, (B, T)), axis=1)
    ranges_np = (s0[..., None] + np.arange(r)).astype(np.int32)
    bd_np = np.array([[0, 0, S, T], [0, 0, S - 1, T - 3]], np.int32)
    sym, ranges, bd = _t(sym_np, dev), _t(ranges_np, dev), _t(bd_np, dev)
    arr = (ctypes.c_int32 * N)(*durs)
    p = lambda t: t.data_ptr()
    st = torch.cuda.current_stream(dev).cuda_stream
    f32 = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device=dev)
    lt, ld, px, py = f32(B, T, r), f32(B, T, r), f32(B, N, S, T + 1), f32(B, Ny, S + 1, T)
    bt, bl, pxb, pyb = f32(B, T, r), f32(B, T, r), f32(B, N, T, r), f32(B, Ny, T, r)
    ft._lib.call("ftr_tdt_pruned_logprobs_fwd_f32", p(logits), p(sym), p(ranges), p(bd), blank, arr, N, 0.05, 0.1, p(lt), p(ld),
                 p(px), p(py), B, T, S, C, r, st)
    ft._lib.call("ftr_tdt_pruned_band_fwd_f32", p(logits), p(sym), p(ranges), p(bd), blank, arr, N, 0.05, 0.1, p(bt), p(bl),
                 p(pxb), p(pyb), B, T, S, C, r, st)
    assert _n(bt).tobytes() == _n(lt).tobytes() and _n(bl).tobytes() == _n(ld).tobytes()
    want_x, want_y = _gather(_n(px), ranges_np), _gather(_n(py), ranges_np)
    want_x[ranges_np[:, None].repeat(N, 1) >= S] = NEG                  # row S has no symbol: no px there
    assert _n(pxb).tobytes() == want_x.tobytes() and _n(pyb).tobytes() == want_y.tobytes()
    assert np.isfinite(want_x).any() and np.isfinite(want_y).any()
    gxb_np = rng.random((B, N, T, r)).astype(np.float32)
    gyb_np = rng.random((B, Ny, T, r)).astype(np.float32)
    gx_np, gy_np = _scatter(gxb_np, ranges_np, S, S, T + 1), _scatter(gyb_np, ranges_np, S, S + 1, T)
    gx_np[~np.isfinite(gx_np)] = 0.0
    gy_np[~np.isfinite(gy_np)] = 0.0
    scale = _t(np.array([0.5, -1.5], np.float32), dev)
    gx, gy, gxb, gyb = _t(gx_np, dev), _t(gy_np, dev), _t(gxb_np, dev), _t(gyb_np, dev)     # alive until the synchronisation
    g_lat, g_band = f32(B, T, r, C + N), f32(B, T, r, C + N)
    ft._lib.call("ftr_tdt_pruned_logprobs_bwd_scaled_f32", p(logits), p(sym), p(ranges), p(bd), blank, arr, N, 0.05, 0.1, p(lt),
                 p(ld), p(gx), p(gy), p(scale), 1, 0.25, p(g_lat), B, T, S, C, r, st)
    ft._lib.call("ftr_tdt_pruned_band_bwd_scaled_f32", p(logits), p(sym), p(ranges), p(bd), blank, arr, N, 0.05, 0.1, p(bt),
                 p(bl), p(gxb), p(gyb), p(scale), 1, 0.25, p(g_band), B, T, S, C, r, st)
    torch.cuda.synchronize()
    assert _n(g_band).any() and _n(g_band).tobytes() == _n(g_lat).tobytes()


# --------------------------------------------------------------------------------------------------------- other cases
def test_band_that_never_reaches_the_end_gives_inf_and_zero_gradients(ft, dev):
    """The designated no-path case: utterance 1's band stays on rows 0..r-1 while s_end = 12, so no band cell has a move
    into the end cell.  Loss +inf, every gradient zero; utterance 0 and 2 as without it."""
    shape, durs = LOSS_SHAPES[0], LOSS_DURATIONS[1]
    logits_np, sym, ranges, bd, blank = _loss_inputs(shape, len(durs))
    stuck = ranges.copy()
    stuck[1] = np.arange(shape[4])
    assert bd[1, 2] > shape[4]
    per = tdt_loss(torch.from_numpy(logits_np).double(), sym, stuck, blank, durs, bd, 0.05, 0.0).numpy()
    assert per[1] == np.inf and np.isfinite(per[[0, 2]]).all()
    before = ft._lib.band_tdt_recursions
    loss, g = _loss_step(ft, dev, logits_np, sym, stuck, blank, durs, bd, sigma=0.05)
    assert ft._lib.band_tdt_recursions == before + 1
    assert loss[1] == np.inf and not g[1].any() and np.isfinite(g).all()
    assert max_rel(loss, per) <= TOL_F64
    loss0, g0 = _loss_step(ft, dev, logits_np, sym, ranges, blank, durs, bd, sigma=0.05)
    for b in (0, 2):
        assert loss[b].tobytes() == loss0[b].tobytes() and g[b].tobytes() == g0[b].tobytes()


def test_nan_stays_in_its_utterance(ft, dev):
    shape, durs = LOSS_SHAPES[0], LOSS_DURATIONS[1]
    logits_np, sym, ranges, bd, blank = _loss_inputs(shape, len(durs))
    poisoned = logits_np.copy()
    poisoned[1, 3, 0, 2] = np.nan
    before = ft._lib.band_tdt_recursions
    loss0, g0 = _loss_step(ft, dev, logits_np, sym, ranges, blank, durs, bd)
    loss, g = _loss_step(ft, dev, poisoned, sym, ranges, blank, durs, bd)
    assert ft._lib.band_tdt_recursions == before + 2
    assert np.isnan(loss[1])
    for b in (0, 2):
        assert loss[b].tobytes() == loss0[b].tobytes() and g[b].tobytes() == g0[b].tobytes()


def test_non_band_ranges_take_the_lattice_route(ft, dev):
    """One row of the ranges set back by one (the band start decreases there): silently the lattice route, and the
    restatement's loss and gradient all the same."""
    shape, durs = LOSS_SHAPES[1], LOSS_DURATIONS[1]
    logits_np, sym, ranges, bd, blank = _loss_inputs(shape, len(durs))
    back = ranges.copy()
    for b in range(shape[0]):
        t = next(t for t in range(5, bd[b, 3] - 1) if back[b, t, 0] == back[b, t - 1, 0] and back[b, t, 0] >= 1)
        back[b, t] -= 1
    l64 = torch.from_numpy(logits_np).double().requires_grad_(True)
    per = tdt_loss(l64, sym, back, blank, durs, bd, 0.05, 0.0)
    per.sum().backward()
    assert np.isfinite(per.detach().numpy()).all()
    before = ft._lib.band_tdt_recursions
    loss, g = _loss_step(ft, dev, logits_np, sym, back, blank, durs, bd, sigma=0.05)
    assert ft._lib.band_tdt_recursions == before
    assert max_rel(loss, per.detach().numpy()) <= TOL_F64 and max_rel(g, l64.grad.numpy()) <= TOL_F64


def test_s_range_16_takes_the_lattice_route(ft, dev):
    B, T, S, C, r, durs, blank = 2, 24, 17, 8, 16, (0, 1, 2), 0
    rng = np.random.default_rng(16)
    logits_np = (rng.standard_normal((B, T, r, C + len(durs))) * 2).astype(np.float32)
    sym = rng.integers(1, C, (B, S)).astype(np.int32)
    s0 = np.minimum(np.arange(T) * (S + 1 - r + 1) // T, S + 1 - r)
    ranges = np.broadcast_to((s0[:, None] + np.arange(r))[None], (B, T, r)).astype(np.int32).copy()
    l64 = torch.from_numpy(logits_np).double().requires_grad_(True)
    per = tdt_loss(l64, sym, ranges, blank, durs, None, 0.0, 0.0)
    per.sum().backward()
    assert np.isfinite(per.detach().numpy()).all()
    before = ft._lib.band_tdt_recursions
    loss, g = _loss_step(ft, dev, logits_np, sym, ranges, blank, durs, None)
    assert ft._lib.band_tdt_recursions == before
    assert max_rel(loss, per.detach().numpy()) <= TOL_F64 and max_rel(g, l64.grad.numpy()) <= TOL_F64


# -------------------------------------------------------------------------------------------------------------- memory
def test_step_allocates_less_than_one_px_lattice(ft, dev):
    """B = 1, T = 1500, S = 300, r = 5, C = 16, durations (0,1,2,3,4): forward + backward stay below the size of ONE px
    lattice, B N S (T+1) 4 bytes = 9.0 MB.  The lattice route holds px, py, float64 p and both gradients, more than four
    of them; the band route's tensors are of the order T r (N + Ny) 4 bytes plus the workspace ((S+T) lanes (N+Ny))."""
    B, T, S, r, C, durs, blank = 1, 1500, 300, 5, 16, (0, 1, 2, 3, 4), 0
    N = len(durs)
    rng = np.random.default_rng(1500)
    s0 = np.minimum(np.arange(T) * (S + 1) // T, S + 1 - r)
    ranges = _t(np.broadcast_to((s0[:, None] + np.arange(r))[None], (B, T, r)).astype(np.int32).copy(), dev)
    sym = _t(rng.integers(1, C, (B, S)).astype(np.int32), dev)
    logits = _t(rng.standard_normal((B, T, r, C + N)).astype(np.float32), dev).requires_grad_(True)
    step = lambda: ft.rnnt_loss_tdt_pruned(logits, sym, ranges, blank, durs, None, reduction="sum")
    step().backward()                            # first use: the band verdict on the ranges, any lazy initialisation
    logits.grad = None
    torch.cuda.synchronize()
    before_calls = ft._lib.band_tdt_recursions
    torch.cuda.reset_peak_memory_stats(dev)
    resident = torch.cuda.memory_allocated(dev)
    loss = step()
    loss.backward()
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated(dev) - resident
    one_px_lattice = B * N * S * (T + 1) * 4
    print(f"band tdt step at T={T} S={S} r={r}: {used} bytes above the resident set, one px lattice = {one_px_lattice}")
    assert ft._lib.band_tdt_recursions == before_calls + 1
    assert np.isfinite(_n(loss)) and np.isfinite(_n(logits.grad)).all() and _n(logits.grad).any()
    assert used < one_px_lattice, (used, one_px_lattice)


# ------------------------------------------------------------------------------------------- determinism and capture
def _step_fn(ft, dev, shape, durs):
    B, T, S, C, r = shape
    logits_np, sym, ranges, bd, blank = _loss_inputs(shape, len(durs))
    buf = _t(logits_np, dev)
    symt, rgt, bdt = _t(sym, dev), _t(ranges, dev), _t(bd, dev)

    def step():
        x = buf.clone().requires_grad_(True)          # the leaf is created inside the step
        loss = ft.rnnt_loss_tdt_pruned(x, symt, rgt, blank, durs, bdt, sigma=0.05, delay_penalty=0.1, reduction="none")
        (g,) = torch.autograd.grad(loss.sum(), (x,))
        return loss.detach(), g.detach()              # only detached results leave it
    return buf, step


def test_two_band_route_steps_are_bit_identical(ft, dev):
    _, step = _step_fn(ft, dev, LOSS_SHAPES[2], LOSS_DURATIONS[1])
    step()
    before = ft._lib.band_tdt_recursions
    a = [_n(v).copy() for v in step()]
    b = [_n(v).copy() for v in step()]
    assert ft._lib.band_tdt_recursions == before + 2
    assert np.isfinite(a[0]).all()
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()


def test_band_route_step_replays_from_a_graph_with_new_values(ft, dev):
    buf, step = _step_fn(ft, dev, LOSS_SHAPES[0], LOSS_DURATIONS[1])
    before = ft._lib.band_tdt_recursions
    g, out = _capture(step)                 # the warm-up steps settle the band verdict of the ranges outside the capture
    assert ft._lib.band_tdt_recursions == before + 4, "the captured step must be a band-route step"
    for seed in (21, 22):
        buf.copy_(torch.randn(buf.shape, generator=torch.Generator().manual_seed(seed)).to(dev) * 2)
        g.replay()
        torch.cuda.synchronize()
        got = [_n(v).copy() for v in out]
        ref = [_n(v).copy() for v in step()]
        assert np.isfinite(got[0]).all()
        for u, v in zip(got, ref):
            assert u.tobytes() == v.tobytes()
