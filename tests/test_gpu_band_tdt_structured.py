"""The band-native TDT route (csrc/mi_band_tdt.hip, the band builders of csrc/tdt_logprobs.hip, the band branch of
rnnt_loss_tdt_pruned) against FLOAT64 on structured, non-iid and long bands (tests/band_tdt_cases.py): a sharp planted
alignment, two regimes that no single mean fits, blank-heavy, tilted, deep (-60 per step), positive values and -inf / -1e20
holes, on shapes chosen for the kernel's code paths.  tests/test_band_tdt_cases.py shows on the CPU that every case has a
finite float64 answer, so "finite everywhere" is demanded of every case.  Every launch goes through
ft.mutual_information_recursion_tdt_band or ft.rnnt_loss_tdt_pruned.

What is asserted, all of it against float64 or against no oracle at all:

* ans: finite, rtol 1e-4 (the project's loss tolerance); occupancies per utterance: normwise max|d| / max|ref| <= 1e-4
  against float64, no float32-oracle fallback; a second launch gives the same bits; a forward-only call (operands without
  grad: the chain is launched with grid (B,1)) gives the same ans bytes.
* invariants to 1e-4, no oracle: every symbol row s_begin <= s < s_end is emitted once (its token occupancies, all N planes,
  sum to 1); the durations taken add up to the frames of the rectangle (sum over moves of duration x occupancy =
  t_end - t_begin); exact zeros for frames outside [t_begin, t_end), rows outside the rectangle and every move whose
  destination lies past t_end.
* shift (kinds sharp and holes): cx + c e_i on token plane i and c d_j on blank plane j move ans by
  (s_end - s_begin) cx + c (t_end - t_begin), rtol 3e-6 / atol 3e-5 (test_band_shift_is_invisible) plus the rounding of the
  shifted float32 operands themselves, (S_n + T_n) 2^-24 max|shifted operand| -- the maximum over the operands that can
  carry weight: the -1e20 stand-ins of `holes` are left out of it, which would make the bound vacuous -- and leave the
  occupancies within 1e-4 of the UNSHIFTED float64 ones.
* chunking: D mod TCH takes all four residues; batch mixing: degenerate, NaN and -inf utterances beside ordinary ones,
  every utterance bit for bit what a launch of its own gives.
* loss level: both routes of rnnt_loss_tdt_pruned on logits peaked on a planted path, against tdt_loss in float64; the
  ten-move list (1,2,3,4,8) among them, which also goes through the lattice recursion alone (test_ten_moves_on_the_lattice).

band_tdt_chain_kernel<LANES, M> (LANES = 8 for r <= 7, 16 for r = 8..15; M = N + Ny) and the parity tests that launch it:

    <8, 2..10>    test_every_chain_instantiation, r = 4, one move list per M (three at M = 6: Dx = Ny, Dx = 5 Ny = 1, Dx = 1 Ny = 5)
    <16, 2..10>   test_every_chain_instantiation, r = 9, the same lists
    <8, 9>        also r in {2, 6, 7} there; test_recursion_vs_float64 at (2,20,70,4) and (1,300,1500,5); test_mixed_batch
    <8, 5>        test_recursion_vs_float64 at (2,100,300,7); test_chunk_residues
    <8, 4>        test_recursion_vs_float64 at (1,120,2000,2)
    <16, 10>      test_recursion_vs_float64 at (2,100,300,8)
    <16, 7>       test_recursion_vs_float64 at (1,250,900,15)
    <16, 8>       test_recursion_vs_float64 at (1,500,700,12)

(test_invariants_without_an_oracle and test_shift_is_invisible launch what test_recursion_vs_float64 launches.)

With FTR_BAND_TDT_PARITY_OUT set, every case's figures (relative error of ans, normwise occupancy error) are written to
that file as JSON when the module is done; a run on MI355X is committed as profiles/band_tdt_structured_parity_errors.json.
"""
import json
import os

import numpy as np
import pytest
import torch

import band_tdt_cases as TC
from helpers import max_rel
from tdt_restatement import blank_durations_of, tdt_dp_with_grads, tdt_loss
from test_gpu_band_tdt import _recursion_case

pytestmark = pytest.mark.gpu

TOL_F64 = 1e-4
NEG = float("-inf")
SHIFTS = [(-37.5, 11.25), (300.0, -40.0)]
_LOG = {}


@pytest.fixture(scope="module", autouse=True)
def _write_log():
    yield
    path = os.environ.get("FTR_BAND_TDT_PARITY_OUT")
    if not path or not _LOG:
        return
    try:
        with open(path, "w") as f:
            json.dump(_LOG, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


def _log(case_id, label, e_ans, e_occ):
    _LOG.setdefault(case_id, {})[label] = dict(ans_rel_vs_f64=float(f"{e_ans:.3e}"), occupancy_normwise_vs_f64=float(f"{e_occ:.3e}"))


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _n(t):
    return t.detach().cpu().numpy()


def _run(ft, dev, pxb, pyb, ranges, tok, blk, bd, S, grads=True):
    """One call of mutual_information_recursion_tdt_band -> (ans, gx_band, gy_band) as numpy (ans alone without grads)."""
    x, y = _t(pxb, dev).requires_grad_(grads), _t(pyb, dev).requires_grad_(grads)
    ans = ft.mutual_information_recursion_tdt_band(x, y, _t(ranges, dev), tok, blk, None if bd is None else _t(bd, dev), S=S)
    if not grads:
        return _n(ans)
    ans.sum().backward()
    return _n(ans), _n(x.grad), _n(y.grad)


def _run_case(ft, dev, case, pxb=None, pyb=None, grads=True):
    return _run(ft, dev, case["pxb"] if pxb is None else pxb, case["pyb"] if pyb is None else pyb, case["ranges"], case["tok"],
                case["blk"], case["bd"], case["S"], grads)


def _norm_err(got, ref):
    """normwise max|d| / max|ref| of one utterance's array."""
    return float(np.abs(got.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def _occupancy_errors(gx, gy, gx64, gy64):
    """Per utterance: max of the normwise errors of gx_band and gy_band against float64."""
    return [max(_norm_err(gx[b], gx64[b]), _norm_err(gy[b], gy64[b])) for b in range(gx.shape[0])]


def _ans_err(ans, want):
    return float(np.max(np.abs(ans.astype(np.float64) - want) / np.abs(want)))


_GPU = {}


def _gpu_result(ft, dev, kind, shape):
    """(ans, gx, gy) of the case on the GPU, computed once for the tests that look at the same launch."""
    key = (kind, shape)
    if key not in _GPU:
        _GPU[key] = _run_case(ft, dev, TC.make_case(kind, shape))
    return _GPU[key]


# ------------------------------------------------------------------------------------------- a. recursion against float64
@pytest.mark.parametrize("shape", TC.SHAPES, ids=TC.shape_id)
@pytest.mark.parametrize("kind", TC.KINDS)
def test_recursion_vs_float64(ft, dev, kind, shape):
    case = TC.make_case(kind, shape)
    a64, gx64, gy64 = TC.reference(kind, shape)
    ans, gx, gy = _gpu_result(ft, dev, kind, shape)
    ans2, gx2, gy2 = _run_case(ft, dev, case)
    fwd = _run_case(ft, dev, case, grads=False)
    fin = bool(np.isfinite(ans).all() and np.isfinite(gx).all() and np.isfinite(gy).all())
    e_ans = _ans_err(ans, a64) if fin else float("nan")
    e_occ = _occupancy_errors(gx, gy, gx64, gy64) if fin else [float("nan")]
    _log(f"{kind}/{TC.shape_id(shape)}", "recursion", e_ans, max(e_occ))
    print(f"band tdt {kind} {TC.shape_id(shape)}: ans rel {e_ans:.3e}, occupancies per utterance {['%.3e' % e for e in e_occ]}")
    assert np.isfinite(a64).all() and np.isfinite(ans).all(), ans
    assert gx.shape == case["pxb"].shape and gy.shape == case["pyb"].shape
    np.testing.assert_allclose(ans, a64, rtol=1e-4, atol=0)
    assert np.isfinite(gx).all() and np.isfinite(gy).all()
    assert max(e_occ) <= TOL_F64, e_occ
    assert ans.tobytes() == ans2.tobytes() and gx.tobytes() == gx2.tobytes() and gy.tobytes() == gy2.tobytes()
    assert fwd.tobytes() == ans.tobytes()


# ------------------------------------------------------------------------------------------- b. invariants, no oracle
def _check_invariants(case, gx, gy):
    B, S, T, r = case["shape"]
    tok, blk = case["tok"], case["blk"]
    gx, gy = gx.astype(np.float64), gy.astype(np.float64)
    tt = np.arange(T)[:, None]
    for b in range(B):
        sb, tb, se, te = (int(v) for v in case["bd"][b])
        rows = TC.band_rows(case)[b]                                            # [T,r] lattice row of every band row
        # exact zeros: frames outside [t_begin, t_end), rows outside the rectangle (no token leaves row s_end), and moves
        # that would land past t_end
        assert not gx[b, :, :tb].any() and not gy[b, :, :tb].any() and not gx[b, :, te:].any() and not gy[b, :, te:].any()
        assert not gx[b][:, (rows < sb) | (rows >= se)].any() and not gy[b][:, (rows < sb) | (rows > se)].any()
        for i, e in enumerate(tok):
            assert not gx[b, i][np.broadcast_to(tt + e > te, rows.shape)].any()
        for j, d in enumerate(blk):
            assert not gy[b, j][np.broadcast_to(tt + d > te, rows.shape)].any()
        per_row = np.bincount(rows.ravel(), weights=gx[b].sum(axis=0).ravel(), minlength=S + 2)[sb:se]
        assert np.abs(per_row - 1.0).max() <= 1e-4, (b, float(np.abs(per_row - 1.0).max()))
        frames = float((gx[b].sum(axis=(1, 2)) * np.array(tok, np.float64)).sum() + (gy[b].sum(axis=(1, 2)) * np.array(blk, np.float64)).sum())
        assert abs(frames - (te - tb)) <= 1e-4 * (te - tb), (b, frames, te - tb)


@pytest.mark.parametrize("shape", TC.SHAPES, ids=TC.shape_id)
@pytest.mark.parametrize("kind", TC.KINDS)
def test_invariants_without_an_oracle(ft, dev, kind, shape):
    ans, gx, gy = _gpu_result(ft, dev, kind, shape)
    assert np.isfinite(ans).all() and np.isfinite(gx).all() and np.isfinite(gy).all()
    _check_invariants(TC.make_case(kind, shape), gx, gy)


# ------------------------------------------------------------------------------------------- c. shift
@pytest.mark.parametrize("shape", TC.SHAPES, ids=TC.shape_id)
@pytest.mark.parametrize("kind", ["sharp", "holes"])
def test_shift_is_invisible(ft, dev, kind, shape):
    case = TC.make_case(kind, shape)
    a64, gx64, gy64 = TC.reference(kind, shape)
    bd = case["bd"].astype(np.int64)
    steps = (bd[:, 2] - bd[:, 0] + 1) + (bd[:, 3] - bd[:, 1] + 1)                                     # S_n + T_n
    for cx, c in SHIFTS:
        pxb, pyb = TC.shifted(case, cx, c)
        ans, gx, gy = _run_case(ft, dev, case, pxb, pyb)
        assert np.isfinite(ans).all() and np.isfinite(gx).all() and np.isfinite(gy).all()
        want = a64 + TC.path_gain(case, cx, c)
        live = lambda a: np.abs(a[np.isfinite(a) & (a > -1e19)]).max()                                # not the -1e20 stand-ins
        atol = 3e-5 + steps * 2.0 ** -24 * np.array([max(live(pxb[b]), live(pyb[b])) for b in range(case["B"])])
        e_occ = _occupancy_errors(gx, gy, gx64, gy64)
        e_ans = _ans_err(ans, want)
        _log(f"{kind}/{TC.shape_id(shape)}", f"shift({cx:g},{c:g})", e_ans, max(e_occ))
        print(f"band tdt {kind} {TC.shape_id(shape)} shift ({cx}, {c}): ans rel {e_ans:.3e} (|d| {np.abs(ans - want)}, atol {atol}), "
              f"occupancies {['%.3e' % e for e in e_occ]}")
        assert (np.abs(ans.astype(np.float64) - want) <= atol + 3e-6 * np.abs(want)).all(), (ans, want, atol)
        assert max(e_occ) <= TOL_F64, ((cx, c), e_occ)


# ------------------------------------------------------------------------------------------- d. every instantiation once
MOVES_BY_M = [((0,), (1,)), ((0, 1), (1,)), ((0, 1), (1, 2)), ((0, 1, 2), (1, 2)), ((1, 2, 4), (1, 2, 4)), ((0, 1, 2, 4), (1, 2, 4)),
              ((0, 1, 3, 5), (1, 2, 4, 8)), ((0, 1, 2, 3, 4), (1, 2, 3, 4)), ((1, 2, 3, 4, 8), (1, 2, 3, 4, 8))]       # M = 2 .. 10
LOPSIDED = [((0, 1, 2, 3, 4), (1,)), ((0,), (1, 2, 3, 4, 5))]                                  # M = 6 with Dx != Ny either way
INSTANCES = ([(r, mv) for r in (4, 9) for mv in MOVES_BY_M + LOPSIDED] + [(r, MOVES_BY_M[7]) for r in (2, 6, 7)])


def test_the_move_lists_reach_every_m():
    assert [len(t) + len(k) for t, k in MOVES_BY_M] == list(range(2, 11))
    assert [(len(t), len(k)) for t, k in LOPSIDED] == [(5, 1), (1, 5)]


@pytest.mark.parametrize("r,moves", INSTANCES, ids=lambda v: str(v).replace(" ", ""))
def test_every_chain_instantiation(ft, dev, r, moves):
    shape = (3, 12, 40, r)
    tok, blk = moves
    pxb, pyb, ranges, bd, has_path, (w_ans, w_gx, w_gy) = _recursion_case(shape, moves, True)
    assert has_path and np.isfinite(w_ans).all(), "the inputs of a parity case must leave every utterance a path"
    ans, gx, gy = _run(ft, dev, pxb, pyb, ranges, tok, blk, bd, shape[1])
    fwd = _run(ft, dev, pxb, pyb, ranges, tok, blk, bd, shape[1], grads=False)
    assert np.isfinite(ans).all() and np.isfinite(gx).all() and np.isfinite(gy).all()
    e_ans, e_occ = _ans_err(ans, w_ans), _occupancy_errors(gx, gy, w_gx, w_gy)
    _log(f"iid/{shape} {tok}/{blk}".replace(" ", ""), "recursion", e_ans, max(e_occ))
    print(f"band tdt iid {shape} {tok}/{blk}: ans rel {e_ans:.3e}, occupancies per utterance {['%.3e' % e for e in e_occ]}")
    np.testing.assert_allclose(ans, w_ans, rtol=1e-4, atol=0)
    assert max(e_occ) <= TOL_F64, e_occ
    assert fwd.tobytes() == ans.tobytes()


@pytest.mark.parametrize("r", [4, 9])
def test_ten_moves_on_the_lattice(ft, dev, r):
    """mi_tdt_kernel<10>: the ten-move operands of test_every_chain_instantiation scattered into full-size lattices, through
    mutual_information_recursion_tdt, against the same float64 reference (occupancies gathered back to the band)."""
    shape, (tok, blk) = (3, 12, 40, r), MOVES_BY_M[8]
    S, T = shape[1], shape[2]
    pxb, pyb, ranges, bd, has_path, (w_ans, w_gx, w_gy) = _recursion_case(shape, (tok, blk), True)
    assert has_path and len(tok) + len(blk) == 10
    px = _t(TC._scatter(pxb, ranges, S, S, T + 1), dev).requires_grad_(True)
    py = _t(TC._scatter(pyb, ranges, S, S + 1, T), dev).requires_grad_(True)
    ans = ft.mutual_information_recursion_tdt(px, py, tok, blk, _t(bd, dev))
    ans.sum().backward()
    ans, gx, gy = _n(ans), TC._gather(_n(px.grad), ranges), TC._gather(_n(py.grad), ranges)
    assert np.isfinite(ans).all() and np.isfinite(_n(px.grad)).all() and np.isfinite(_n(py.grad)).all()
    e_ans, e_occ = _ans_err(ans, w_ans), _occupancy_errors(gx, gy, w_gx, w_gy)
    _log(f"iid/{shape} {tok}/{blk}".replace(" ", ""), "lattice recursion", e_ans, max(e_occ))
    print(f"lattice tdt iid {shape} {tok}/{blk}: ans rel {e_ans:.3e}, occupancies per utterance {['%.3e' % e for e in e_occ]}")
    np.testing.assert_allclose(ans, w_ans, rtol=1e-4, atol=0)
    assert max(e_occ) <= TOL_F64, e_occ
    assert float(_n(px.grad).sum()) == pytest.approx(float(gx.sum()), rel=1e-6)      # nothing off the band


# ------------------------------------------------------------------------------------------- e., f.: small hand-made batches
def _iid_utterance(rng, S, T, r, tok, blk, bd, lo=None):
    """(pxb [N,T,r], pyb [Ny,T,r], lo [T]) of one utterance: iid N(0,1) with 2 % -inf, a planted path of its own moves kept
    finite (when the rectangle has one and no band is given), the builder's -inf rules.  As _recursion_case."""
    N, Ny = len(tok), len(blk)
    sb, tb, se, te = bd
    pxb = rng.standard_normal((N, T, r)).astype(np.float32)
    pyb = rng.standard_normal((Ny, T, r)).astype(np.float32)
    pxb[rng.random(pxb.shape) < 0.02] = NEG
    pyb[rng.random(pyb.shape) < 0.02] = NEG
    if lo is None:
        path = TC._random_path(rng, se - sb + 1, te - tb + 1, tok, blk, r) if se >= sb and te >= tb else []
        assert path is not None
        lo = TC._band_around(rng, path, sb, tb, te, S, T, r)
        for s, t, m in path:
            (pxb[m] if m < N else pyb[m - N])[tb + t, sb + s - lo[tb + t]] = rng.standard_normal()
    rows = lo[:, None] + np.arange(r)
    tt = np.arange(T)[:, None]
    for i, e in enumerate(tok):
        pxb[i][(rows >= S) | (tt >= te) | (tt + e > te)] = NEG
    for j, d in enumerate(blk):
        pyb[j][np.broadcast_to(tt + d > te, rows.shape)] = NEG
    return pxb, pyb, lo


def _restatement(pxb, pyb, ranges, bd, tok, blk, S):
    """float64 (ans [B], gx_band, gy_band) of band operands through the scattered lattices."""
    T = pxb.shape[2]
    ans, gx, gy = tdt_dp_with_grads(TC._scatter(pxb, ranges, S, S, T + 1), TC._scatter(pyb, ranges, S, S + 1, T), tok, blk, bd)
    return ans, TC._gather(gx, ranges), TC._gather(gy, ranges)


CHUNK_MOVES = ((0, 1, 2), (1, 2))
CHUNK_CASES = [(T, T - cut) for T in (9, 10, 11, 12) for cut in (0, 1)]            # (T, t_end)


def test_the_chunk_cases_cover_every_residue():
    S = 6
    assert sorted({(S + te) % 4 for _, te in CHUNK_CASES}) == [0, 1, 2, 3] and len(CHUNK_CASES) == 8      # D = S_n - 1 + T_n - 1


@pytest.mark.parametrize("T,te", CHUNK_CASES)
def test_chunk_residues(ft, dev, T, te):
    """The chain fetches its operands four steps at a time and picks the end value at step D = S + t_end of its walk."""
    S, r = 6, 3
    tok, blk = CHUNK_MOVES
    rng = np.random.default_rng([S, T, te])
    bd = np.array([[0, 0, S, te]], np.int32)
    x, y, lo = _iid_utterance(rng, S, T, r, tok, blk, tuple(int(v) for v in bd[0]))
    pxb, pyb, ranges = x[None], y[None], (lo[None, :, None] + np.arange(r)).astype(np.int32)
    w_ans, w_gx, w_gy = _restatement(pxb, pyb, ranges, bd, tok, blk, S)
    assert np.isfinite(w_ans).all()
    ans, gx, gy = _run(ft, dev, pxb, pyb, ranges, tok, blk, bd if te < T else None, S)
    fwd = _run(ft, dev, pxb, pyb, ranges, tok, blk, bd if te < T else None, S, grads=False)
    e_ans, e_occ = _ans_err(ans, w_ans), _occupancy_errors(gx, gy, w_gx, w_gy)
    _log(f"chunk/T{T}te{te}", "recursion", e_ans, max(e_occ))
    print(f"band tdt chunk T={T} t_end={te} D%4={(S + te) % 4}: ans rel {e_ans:.3e}, occupancies {['%.3e' % e for e in e_occ]}")
    np.testing.assert_allclose(ans, w_ans, rtol=1e-4, atol=0)
    assert max(e_occ) <= TOL_F64, e_occ
    assert fwd.tobytes() == ans.tobytes()


def _mixed_batch():
    S, T, r = 12, 40, 4
    tok, blk = (0, 1, 2, 3, 4), (1, 2, 3, 4)
    rng = np.random.default_rng(1240)
    bd = np.array([[0, 0, S, T],            # ordinary
                   [8, 0, 3, T],            # inverted rectangle: ans 0, no occupancies
                   [5, 7, 5, 7],            # a single cell: ans 0, no occupancies
                   [0, 0, S, T],            # its band steps backwards inside the rectangle: NaN, no occupancies
                   [0, 0, S, T],            # its band stays on rows 0..r-1 and never reaches s_end: -inf, no occupancies
                   [1, 2, S - 1, T - 2]],   # ordinary, offset rectangle
                  np.int32)
    utts = [_iid_utterance(rng, S, T, r, tok, blk, tuple(int(v) for v in bd[b]),
                           lo=np.zeros(T, np.int64) if b == 4 else None) for b in range(6)]
    pxb, pyb = np.stack([u[0] for u in utts]), np.stack([u[1] for u in utts])
    lo = np.stack([u[2] for u in utts])
    t = int(np.argmax(lo[3] > 0))
    assert lo[3, t] > 0 and t + 3 < T
    lo[3, t + 1:t + 3] = lo[3, t] - 1
    ranges = (lo[:, :, None] + np.arange(r)).astype(np.int32)
    return S, tok, blk, pxb, pyb, ranges, bd


def test_mixed_batch(ft, dev):
    S, tok, blk, pxb, pyb, ranges, bd = _mixed_batch()
    ans, gx, gy = _run(ft, dev, pxb, pyb, ranges, tok, blk, bd, S)
    fwd = _run(ft, dev, pxb, pyb, ranges, tok, blk, bd, S, grads=False)
    assert fwd.tobytes() == ans.tobytes()
    for b in range(6):
        one = slice(b, b + 1)
        a1, gx1, gy1 = _run(ft, dev, pxb[one], pyb[one], ranges[one], tok, blk, bd[one], S)
        assert ans[one].tobytes() == a1.tobytes() and gx[one].tobytes() == gx1.tobytes() and gy[one].tobytes() == gy1.tobytes(), b
        if b == 3:                               # the documented reply to a band that is none
            assert np.isnan(ans[b]) and not gx[b].any() and not gy[b].any()
            continue
        w_ans, w_gx, w_gy = _restatement(pxb[one], pyb[one], ranges[one], bd[one], tok, blk, S)
        if b in (0, 5):
            assert np.isfinite(w_ans).all() and np.isfinite(ans[b])
            np.testing.assert_allclose(ans[one], w_ans, rtol=1e-4, atol=0)
            assert max(_occupancy_errors(gx[one], gy[one], w_gx, w_gy)) <= TOL_F64
        else:
            assert w_ans[0] == (NEG if b == 4 else 0.0) and not w_gx.any() and not w_gy.any()
            assert ans[b] == w_ans[0] and not gx[b].any() and not gy[b].any()


# ------------------------------------------------------------------------------------------- h. loss level, both routes
LOSS_B, LOSS_T, LOSS_S = 2, 48, 14
LOSS_DURS = [(0, 1, 2, 3, 4), (1, 2, 4), (1, 2, 3, 4, 8)]
_LOSS = {}


def _loss_case(r, durs, C):
    """(logits [B,T,r,C+N] float32, symbols, ranges, bd, blank, per-utterance float64 loss, float64 d logits): 2 N(0,1) with
    +12 on the planted path's token column (the symbol of a token move, the blank of a blank move) and +12 on the duration
    column of the move it takes there.  The blank is column 0 for C = 36 and the last column for C = 37.  The delay penalty
    enters the loss with either sign, so a loss can come out near 0, where a relative error says nothing: the seeds are
    such that every reference loss has |loss| >= 1 (asserted by the test).  Cached."""
    key = (r, durs, C)
    if key not in _LOSS:
        B, T, S, N = LOSS_B, LOSS_T, LOSS_S, len(durs)
        blk = blank_durations_of(durs)
        rng = np.random.default_rng([r, C, N, sum(durs), 1])
        blank = 0 if C == 36 else C - 1
        sym = (rng.integers(1, C - 1, (B, S)) if blank == C - 1 else rng.integers(1, C, (B, S))).astype(np.int32)
        bd = np.array([[0, 0, S, T], [0, 0, S - 2, T - 5]], np.int32)
        x = (2.0 * rng.standard_normal((B, T, r, C + N))).astype(np.float32)
        ranges = np.zeros((B, T, r), np.int32)
        for b in range(B):
            sb, tb, se, te = (int(v) for v in bd[b])
            path = TC._random_path(rng, se - sb + 1, te - tb + 1, durs, blk, r)
            assert path is not None
            lo = TC._band_around(rng, path, sb, tb, te, S, T, r)
            ranges[b] = lo[:, None] + np.arange(r)
            for s, t, m in path:
                k = sb + s - lo[tb + t]
                x[b, tb + t, k, sym[b, sb + s] if m < N else blank] += np.float32(12.0)
                x[b, tb + t, k, C + (m if m < N else durs.index(blk[m - N]))] += np.float32(12.0)
        l64 = torch.from_numpy(x).double().requires_grad_(True)
        per = tdt_loss(l64, sym, ranges, blank, durs, bd, 0.05, 0.1)
        per.sum().backward()
        _LOSS[key] = (x, sym, ranges, bd, blank, per.detach().numpy(), l64.grad.numpy())
    return _LOSS[key]


@pytest.mark.parametrize("route", ["band", "lattice"])
@pytest.mark.parametrize("C", [36, 37])
@pytest.mark.parametrize("durs", LOSS_DURS, ids=str)
@pytest.mark.parametrize("r", [5, 8])
def test_peaked_logits_through_both_routes(ft, dev, monkeypatch, r, durs, C, route):
    x, sym, ranges, bd, blank, per, grad = _loss_case(r, durs, C)
    assert np.isfinite(per).all() and np.isfinite(grad).all() and np.abs(per).min() >= 1.0
    if route == "lattice":
        monkeypatch.setenv("FTR_PRUNED_ROUTE", "lattice")
    else:
        monkeypatch.delenv("FTR_PRUNED_ROUTE", raising=False)
    before = ft._lib.band_tdt_recursions
    logits = _t(x, dev).requires_grad_(True)
    loss = ft.rnnt_loss_tdt_pruned(logits, _t(sym, dev), _t(ranges, dev), blank, durs, _t(bd, dev), sigma=0.05, delay_penalty=0.1,
                                   reduction="none")
    loss.sum().backward()
    assert ft._lib.band_tdt_recursions - before == (1 if route == "band" else 0), route     # the route that was meant
    loss, g = _n(loss), _n(logits.grad)
    assert np.isfinite(loss).all() and np.isfinite(g).all()
    el, eg = _ans_err(loss, per), max_rel(g, grad)
    _LOG.setdefault(f"loss/r{r} {durs} C{C}".replace(" ", ""), {})[route] = dict(loss_rel_vs_f64=float(f"{el:.3e}"),
                                                                                  dlogits_normwise_vs_f64=float(f"{eg:.3e}"))
    print(f"band tdt peaked loss r={r} {durs} C={C} route={route}: loss {el:.3e} dlogits {eg:.3e}, loss64 {per}")
    assert el <= 1e-4 and eg <= 1e-4, (route, el, eg)
    for b in range(LOSS_B):
        te = int(bd[b, 3])
        assert not grad[b, te:].any() and not g[b, te:].any()          # outside the boundary zeros stay zeros, exactly
