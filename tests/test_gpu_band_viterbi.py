"""Best-path alignment on the pruned band itself (csrc/mi_band_viterbi.hip, include/ftr_band_viterbi.h):
mutual_information_viterbi_tdt_band against the float32 restatement (tests/viterbi_tdt_restatement.py) on the band
scattered into lattices of -inf, the two routes of the three rnnt_alignment_*_pruned wrappers against each other, which
route is taken, the edge conventions, a planted path, peak memory, graph capture, the errors.  Every comparison of outputs
is == on bits: a cell is one float32 add per move and ordered selects.

The parity inputs are those of the band TDT and band multi-blank recursion tests (a band drawn around a random path of
the case's own moves, the builders' -inf rules applied), as drawn and rounded to integers so that ties decide most cells.
Every reference score is finite, with the exception those files state: shape (B,S,T,r) = (2,5,1,4), whose utterances
without a path must give score -inf and -1 everywhere."""
import functools

import numpy as np
import pytest
import torch

import band_multiblank_cases as MB
import viterbi_tdt_restatement as VT
from band_tdt_cases import _band_around, _random_path, _scatter
from test_gpu_band_tdt import MOVES as TDT_MOVES0, ONE_FRAME, SHAPES as TDT_SHAPES0, _recursion_case
from test_gpu_graph import _capture
from test_gpu_viterbi_tdt import _bits, _equal, _n, _same, _t

pytestmark = pytest.mark.gpu

NEG = np.float32(-np.inf)
ENTRY = "ftr_mutual_information_band_viterbi_f32"
# the top of 8 and of 16 lanes on top of the recursion's shapes: S + T from 10 to 1106, rows that wrap the lanes several
# times, every residue of the chunk of 4 steps, decision windows of 64 steps that turn over
TDT_SHAPES = TDT_SHAPES0 + [(1, 40, 130, 7), (1, 70, 200, 15)]
TDT_MOVES = TDT_MOVES0 + [((0,), (1, 2, 4, 8)), ((0,), (1, 2, 3, 4, 5, 6, 7, 8))]


def _run(ft, dev, pxb, pyb, ranges, tok, blk, bd, S):
    out = ft.mutual_information_viterbi_tdt_band(_t(pxb, dev), _t(pyb, dev), _t(ranges, dev), tok, blk,
                                                 None if bd is None else _t(bd, dev), S=S)
    torch.cuda.synchronize()
    assert not any(o.requires_grad for o in out)
    return tuple(_n(o) for o in out)


def _lattices(pxb, pyb, ranges, S):
    T = pxb.shape[2]
    return _scatter(pxb, ranges, S, S, T + 1), _scatter(pyb, ranges, S, S + 1, T)


def _all_minus_one(out, b):
    return all((o[b] == -1).all() for o in out[1:])


# ------------------------------------------------------------------------------------------ 1. against the restatement
@functools.lru_cache(maxsize=None)
def _tdt_expected(shape, moves, with_boundary, integer):
    pxb, pyb, ranges, bd, _, _ = _recursion_case(shape, moves, with_boundary)
    if integer:   # ties decide most cells (rint keeps -inf)
        pxb, pyb = np.rint(pxb).astype(np.float32), np.rint(pyb).astype(np.float32)
    px, py = _lattices(pxb, pyb, ranges, shape[1])
    return pxb, pyb, ranges, bd, px, py, VT.viterbi_tdt(px, py, *moves, bd)


@functools.lru_cache(maxsize=None)
def _mb_expected(shape, durations, with_boundary, integer):
    pxb, pyb, ranges, bd, _, _ = MB.recursion_case(shape, durations, with_boundary)
    pxb = pxb[:, None]
    if integer:
        pxb, pyb = np.rint(pxb).astype(np.float32), np.rint(pyb).astype(np.float32)
    px, py = _lattices(pxb, pyb, ranges, shape[1])
    return pxb, pyb, ranges, bd, px, py, VT.viterbi_tdt(px, py, (0,), durations, bd)


def _check_reference(shape, with_boundary, want):
    """The condition on the reference, before the device is looked at: a finite score everywhere, but for ONE_FRAME, which
    has no path in the full rectangle (with the ragged boundary a token of duration 1 may reach the end cell)."""
    if shape == ONE_FRAME:
        assert with_boundary or (want[0] == NEG).all()
        assert all(np.isfinite(want[0][b]) or (want[0][b] == NEG and _all_minus_one(want, b)) for b in range(shape[0]))
    else:
        assert np.isfinite(want[0]).all(), "the inputs of a parity case must leave every utterance a path"


@pytest.mark.parametrize("integer", [False, True], ids=["drawn", "rint"])
@pytest.mark.parametrize("with_boundary", [False, True], ids=["full", "subrect"])
@pytest.mark.parametrize("moves", TDT_MOVES, ids=str)
@pytest.mark.parametrize("shape", TDT_SHAPES, ids=str)
def test_bit_exact_against_restatement_tdt(ft, dev, shape, moves, with_boundary, integer):
    pxb, pyb, ranges, bd, px, py, want = _tdt_expected(shape, moves, with_boundary, integer)
    _check_reference(shape, with_boundary, want)
    got = _run(ft, dev, pxb, pyb, ranges, *moves, bd, shape[1])
    _same(got, want, (shape, moves, with_boundary, integer))
    if moves == ((0,), (1,)):
        score, frames = ft.mutual_information_viterbi(_t(px[:, 0], dev), _t(py[:, 0], dev), None if bd is None else _t(bd, dev))
        assert np.array_equal(_bits(_n(score)), _bits(got[0])) and np.array_equal(_n(frames), got[1])


@pytest.mark.parametrize("integer", [False, True], ids=["drawn", "rint"])
@pytest.mark.parametrize("with_boundary", [False, True], ids=["full", "subrect"])
@pytest.mark.parametrize("durations", MB.RECURSION_DURATIONS, ids=str)
@pytest.mark.parametrize("shape", MB.RECURSION_SHAPES, ids=str)
def test_bit_exact_against_restatement_big_blanks(ft, dev, shape, durations, with_boundary, integer):
    """Blanks above 16 frames, (1, 32) and (1, 2, 4, 8, 16, 17, 31, 32) -- nine moves -- among them; no 1 in (2, 3)."""
    pxb, pyb, ranges, bd, px, py, want = _mb_expected(shape, durations, with_boundary, integer)
    _check_reference(shape, with_boundary, want)
    got = _run(ft, dev, pxb, pyb, ranges, (0,), durations, bd, shape[1])
    _same(got, want, (shape, durations, with_boundary, integer))
    if durations == (1,):
        score, frames = ft.mutual_information_viterbi(_t(px[:, 0], dev), _t(py[:, 0], dev), None if bd is None else _t(bd, dev))
        assert np.array_equal(_bits(_n(score)), _bits(got[0])) and np.array_equal(_n(frames), got[1])


# ------------------------------------------------------------------------------------------ 2. / 3. wrappers and routes
def _pruned_inputs(ft, dev, width, termination_symbol, sym_lo, sym_hi, r):
    """The sizes of test_gpu_viterbi_tdt._pruned_inputs, at a band width of choice."""
    torch.manual_seed(3)
    B, T, S, C = 2, 40, 12, 16
    am = torch.randn(B, T, C, device=dev); lm = torch.randn(B, S + 1, C, device=dev)
    sym = torch.randint(sym_lo, sym_hi, (B, S), device=dev, dtype=torch.int32)
    bd = torch.tensor([[0, 0, S, T], [0, 0, S - 3, T - 6]], dtype=torch.int32, device=dev)
    _, (gx, gy) = ft.rnnt_loss_simple(lm, am, sym, termination_symbol, bd, reduction="none", calc_gradients=True)
    ranges = ft.get_rnnt_prune_ranges(gx, gy, bd, r)
    return torch.randn(B, T, r, width, device=dev), sym, ranges, bd


def _spy(ft, monkeypatch):
    names, real = [], ft._lib.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(ft._lib, "call", call)
    return names


def _wrapper(ft, dev, which, r):
    """(the call, the same answer from the builder's lattices) of one wrapper."""
    C = 16
    if which == "tdt":
        durs = (0, 1, 2, 3, 4)
        logits, sym, ranges, bd = _pruned_inputs(ft, dev, C + len(durs), C - 1, 0, C - 1, r)
        return (lambda rg=ranges, **kw: ft.rnnt_alignment_tdt_pruned(logits, sym, rg, C - 1, durs, bd, **kw),
                lambda rg=ranges: ft.mutual_information_viterbi_tdt(*ft.get_rnnt_logprobs_tdt_pruned(logits, sym, rg, C - 1, durs, bd),
                                                                    durs, (1, 2, 3, 4), bd), ranges)
    if which == "multiblank":
        big = ((13, 2), (14, 4), (15, 8))
        logits, sym, ranges, bd = _pruned_inputs(ft, dev, C, 0, 1, 13, r)

        def lattice(rg=ranges):
            px, py = ft.get_rnnt_logprobs_multiblank_pruned(logits, sym, rg, 0, big, bd)
            return ft.mutual_information_viterbi_tdt(px.unsqueeze(1), py, (0,), (1, 2, 4, 8), bd)
        return lambda rg=ranges, **kw: ft.rnnt_alignment_multiblank_pruned(logits, sym, rg, 0, big, bd, **kw), lattice, ranges
    logits, sym, ranges, bd = _pruned_inputs(ft, dev, C, C - 1, 0, C - 1, r)
    if which == "bf16":
        logits = logits.bfloat16()
    return (lambda rg=ranges, **kw: ft.rnnt_alignment_pruned(logits, sym, rg, C - 1, bd, **kw),
            lambda rg=ranges, **kw: ft.mutual_information_viterbi(*ft.get_rnnt_logprobs_pruned(logits, sym, rg, C - 1, bd, **kw), bd), ranges)


@pytest.mark.parametrize("r", [5, 8])
@pytest.mark.parametrize("which", ["tdt", "multiblank", "regular", "bf16"])
def test_both_routes_of_the_wrappers_are_bit_identical(ft, dev, monkeypatch, which, r):
    run, lattice, _ = _wrapper(ft, dev, which, r)
    names = _spy(ft, monkeypatch)
    band = run()
    assert names.count(ENTRY) == 1 and not any("viterbi" in n for n in names if n != ENTRY), names
    assert np.isfinite(_n(band[0])).all() and not any(o.requires_grad for o in band)
    del names[:]
    monkeypatch.setenv("FTR_PRUNED_ROUTE", "lattice")
    lat = run()
    assert ENTRY not in names and sum("viterbi" in n for n in names) == 1, names
    _equal(band, lat)
    _equal(band, lattice())


def test_other_inputs_take_the_lattice_route(ft, dev, monkeypatch):
    """Non-band ranges, s_range = 16 and rnnt_type = "modified": the answer of viterbi(builder lattices), as before, and
    the band kernel is not the one that ran."""
    names = _spy(ft, monkeypatch)
    for which in ("tdt", "multiblank", "regular"):
        run, lattice, ranges = _wrapper(ft, dev, which, 5)
        back = ranges.clone()
        rg = _n(ranges)
        for b in range(rg.shape[0]):        # one row set back by one: the band start decreases there
            t = next(t for t in range(5, 30) if rg[b, t, 0] == rg[b, t - 1, 0] and rg[b, t, 0] >= 1)
            back[b, t] -= 1
        del names[:]
        got = run(back)
        assert ENTRY not in names, (which, names)
        _equal(got, lattice(back))
    run, lattice, _ = _wrapper(ft, dev, "regular", 5)
    del names[:]
    _equal(run(rnnt_type="modified"), lattice(rnnt_type="modified"))
    assert ENTRY not in names
    B, T, S, C, r = 2, 24, 17, 8, 16
    torch.manual_seed(16)
    s0 = np.minimum(np.arange(T) * (S + 1 - r + 1) // T, S + 1 - r)
    ranges = _t(np.broadcast_to((s0[:, None] + np.arange(r))[None], (B, T, r)).astype(np.int32).copy(), dev)
    sym = torch.randint(1, C, (B, S), device=dev, dtype=torch.int32)
    logits = torch.randn(B, T, r, C, device=dev)
    del names[:]
    got = ft.rnnt_alignment_pruned(logits, sym, ranges, 0)
    assert ENTRY not in names and np.isfinite(_n(got[0])).all()
    _equal(got, ft.mutual_information_viterbi(*ft.get_rnnt_logprobs_pruned(logits, sym, ranges, 0, None)))
    got = ft.rnnt_alignment_tdt_pruned(torch.randn(B, T, r, C + 2, device=dev), sym, ranges, 0, (0, 1))
    assert ENTRY not in names and np.isfinite(_n(got[0])).all()


# ------------------------------------------------------------------------------------------------------------ 4. edges
def _ramp_case(B, S, T, r, tok, blk, seed):
    """A band that climbs evenly from row 0 to row S, iid operands with the builders' -inf rules."""
    rng = np.random.default_rng(seed)
    s0 = np.minimum(np.arange(T) * (S + 1) // T, S + 1 - r)
    ranges = np.broadcast_to((s0[:, None] + np.arange(r))[None], (B, T, r)).astype(np.int32).copy()
    pxb = rng.standard_normal((B, len(tok), T, r)).astype(np.float32)
    pyb = rng.standard_normal((B, len(blk), T, r)).astype(np.float32)
    return pxb, pyb, ranges


def _builder_rules(pxb, pyb, ranges, bd, tok, blk, S):
    tt = np.arange(pxb.shape[2])[:, None]
    for b in range(pxb.shape[0]):
        te = int(bd[b, 3])
        for i, e in enumerate(tok):
            pxb[b, i][(ranges[b] >= S) | (tt >= te) | (tt + e > te)] = NEG
        for j, d in enumerate(blk):
            pyb[b, j][np.broadcast_to(tt + d > te, ranges[b].shape)] = NEG


def test_edges_in_one_batch(ft, dev):
    """No path; a NaN on a cell from which blank-1 moves reach the end; a band start that decreases; an inverted
    rectangle; S_n = T_n = 1; and plain neighbours with and without a sub-rectangle: each utterance is, bit for bit,
    what a launch of its own gives.  Then S = 0."""
    tok, blk = (0, 1), (1, 2)
    B, S, T, r = 7, 33, 70, 5
    pxb, pyb, ranges = _ramp_case(B, S, T, r, tok, blk, 4)
    bd = np.array([[0, 0, S, T], [0, 0, S, T], [0, 0, S, T], [0, 0, S, T], [9, 4, 3, 30], [5, 10, 5, 10], [2, 3, S - 4, T - 9]], np.int32)
    _builder_rules(pxb, pyb, ranges, bd, tok, blk, S)
    pxb[1, :, 20:46] = NEG                       # no token move out of frames 20..45, whose first and last bands share no row
    assert ranges[2, T - 3, r - 1] == S
    pyb[2, 0, T - 3, r - 1] = np.nan             # the blank of one frame out of (S, T - 3)
    t = next(t for t in range(10, T) if ranges[3, t, 0] == ranges[3, t - 1, 0] and ranges[3, t, 0] >= 1)
    ranges[3, t] -= 1
    got = _run(ft, dev, pxb, pyb, ranges, tok, blk, bd, S)
    score = got[0]
    assert np.isfinite(score[[0, 6]]).all() and score[1] == NEG and np.isnan(score[2]) and np.isnan(score[3])
    assert score[4] == 0 and score[5] == 0 and _bits(score[4]) == 0 and _bits(score[5]) == 0
    for b in (1, 2, 3, 4, 5):
        assert _all_minus_one(got, b), b
    for b in range(B):
        own = _run(ft, dev, pxb[b:b + 1], pyb[b:b + 1], ranges[b:b + 1], tok, blk, bd[b:b + 1], S)
        assert _bits(own[0][0]) == _bits(score[b]), b
        assert all(np.array_equal(o[0], g[b]) for o, g in zip(own[1:], got[1:])), b
    ok = [0, 1, 4, 5, 6]                         # without NaN and with a band: the restatement on the scattered lattices
    px, py = _lattices(pxb[ok], pyb[ok], ranges[ok], S)
    _same(tuple(g[ok] for g in got), VT.viterbi_tdt(px, py, tok, blk, bd[ok]))
    # S = 0: one row, blanks only
    pxb0, pyb0, ranges0 = _ramp_case(2, 0, 9, 1, tok, blk, 5)
    bd0 = np.array([[0, 0, 0, 9], [0, 1, 0, 8]], np.int32)
    _builder_rules(pxb0, pyb0, ranges0, bd0, tok, blk, 0)
    got0 = _run(ft, dev, pxb0, pyb0, ranges0, tok, blk, bd0, 0)
    assert got0[1].shape == (2, 0) and got0[2].shape == (2, 0) and np.isfinite(got0[0]).all()
    _same(got0, VT.viterbi_tdt(*_lattices(pxb0, pyb0, ranges0, 0), tok, blk, bd0))


# ----------------------------------------------------------------------------------------------------- 5. planted path
def test_recovers_a_planted_path(ft, dev):
    """One path of random moves at -0.1 (token) / -0.05 (blank) per move, every other operand at N(-10, 0.5): a deviation
    trades at most five planted moves (>= -0.5) for a move below -7."""
    tok, blk = (0, 1, 2, 3, 4), (1, 2, 3, 4)
    B, S, T, r = 2, 70, 300, 5
    rng = np.random.default_rng(5)
    pxb = (0.5 * rng.standard_normal((B, len(tok), T, r)) - 10.0).astype(np.float32)
    pyb = (0.5 * rng.standard_normal((B, len(blk), T, r)) - 10.0).astype(np.float32)
    ranges = np.zeros((B, T, r), np.int32)
    frames = np.zeros((B, S), np.int32); durs = np.zeros((B, S), np.int32); steps = np.zeros((B, T), np.int32)
    for b in range(B):
        path = _random_path(rng, S + 1, T + 1, tok, blk, r)
        lo = _band_around(rng, path, 0, 0, T, S, T, r)
        ranges[b] = lo[:, None] + np.arange(r)
        for s, t, m in path:
            if m < len(tok):
                pxb[b, m, t, s - lo[t]] = -0.1
                frames[b, s], durs[b, s] = t, tok[m]
            else:
                pyb[b, m - len(tok), t, s - lo[t]] = -0.05
                steps[b, t] = blk[m - len(tok)]
    _builder_rules(pxb, pyb, ranges, np.array([[0, 0, S, T]] * B), tok, blk, S)
    got = _run(ft, dev, pxb, pyb, ranges, tok, blk, None, S)
    assert np.array_equal(got[1], frames) and np.array_equal(got[2], durs) and np.array_equal(got[3], steps)
    _same(got, VT.viterbi_tdt(*_lattices(pxb, pyb, ranges, S), tok, blk, None))


# ------------------------------------------------------------------------------------------------------------ 6. memory
def test_alignment_allocates_less_than_one_px_lattice(ft, dev, monkeypatch):
    """B = 1, T = 1500, S = 300, r = 5, C = 16, durations (0,1,2,3,4): rnnt_alignment_tdt_pruned stays below the size of ONE
    px plane set, N S (T+1) 4 bytes = 9.0 MB.  The lattice route allocates that set itself, and py and the decision
    workspace on top of it."""
    B, T, S, r, C, durs, blank = 1, 1500, 300, 5, 16, (0, 1, 2, 3, 4), 0
    N = len(durs)
    rng = np.random.default_rng(1500)
    s0 = np.minimum(np.arange(T) * (S + 1) // T, S + 1 - r)
    ranges = _t(np.broadcast_to((s0[:, None] + np.arange(r))[None], (B, T, r)).astype(np.int32).copy(), dev)
    sym = _t(rng.integers(1, C, (B, S)).astype(np.int32), dev)
    logits = _t(rng.standard_normal((B, T, r, C + N)).astype(np.float32), dev)
    step = lambda: ft.rnnt_alignment_tdt_pruned(logits, sym, ranges, blank, durs)
    first = step()                               # first use: the band verdict on the ranges, any lazy initialisation
    torch.cuda.synchronize()
    names = _spy(ft, monkeypatch)
    torch.cuda.reset_peak_memory_stats(dev)
    resident = torch.cuda.memory_allocated(dev)
    out = step()
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated(dev) - resident
    one_px_plane_set = B * N * S * (T + 1) * 4
    print(f"band alignment at T={T} S={S} r={r}: {used} bytes above the resident set, one px plane set = {one_px_plane_set}")
    assert names.count(ENTRY) == 1
    assert np.isfinite(_n(out[0])).all() and (_n(out[1]) >= 0).all()
    _equal(out, first)
    assert used < one_px_plane_set, (used, one_px_plane_set)


# ------------------------------------------------------------------------------------------- 7. capture, repeatability
def test_graph_capture_and_repeatability(ft, dev, monkeypatch):
    """Captured once, replayed with new logits written in place: each replay equals an eager run (one builder launch and
    one alignment launch, no memset / memcpy nodes).  Two eager runs are bit-identical."""
    durs, C, r = (0, 1, 2, 3, 4), 16, 5
    logits, sym, ranges, bd = _pruned_inputs(ft, dev, C + len(durs), C - 1, 0, C - 1, r)
    step = lambda: ft.rnnt_alignment_tdt_pruned(logits, sym, ranges, C - 1, durs, bd)
    g, out = _capture(step)
    names = _spy(ft, monkeypatch)
    for i in range(2):
        logits.copy_(torch.randn_like(logits))
        g.replay()
        torch.cuda.synchronize()
        e1, e2 = step(), step()
        torch.cuda.synchronize()
        _equal(out, e1)
        _equal(e1, e2)
    assert names.count(ENTRY) == 4
    assert np.isfinite(_n(e1[0])).all()


# ------------------------------------------------------------------------------------------------------------ 8. errors
def test_value_errors(ft, dev):
    f = ft.mutual_information_viterbi_tdt_band
    x, y = torch.zeros(1, 2, 4, 3, device=dev), torch.zeros(1, 1, 4, 3, device=dev)
    rg = torch.arange(3, dtype=torch.int32, device=dev).expand(1, 4, 3).contiguous()
    assert f(x, y, rg, (0, 1), (1,), S=2)[1].shape == (1, 2)
    for tok, blk in (((), (1,)), ((0, 1), ()), ((1, 0), (1,)), ((0, 17), (1,)), ((0, 1), (0,)), ((0, 1), (33,)), ((0,), (1,)),
                     ((0, 1), (1, 2))):                   # the duration lists, and lists that do not match the planes
        with pytest.raises(ValueError):
            f(x, y, rg, tok, blk, S=2)
    with pytest.raises(ValueError):                      # ten moves
        f(torch.zeros(1, 5, 4, 3, device=dev), torch.zeros(1, 5, 4, 3, device=dev), rg, (0, 1, 2, 3, 4), (1, 2, 3, 4, 5), S=2)
    for bad in (lambda: f(x, y, rg[:, :3], (0, 1), (1,), S=2), lambda: f(x[0], y[0], rg, (0, 1), (1,), S=2),
                lambda: f(x, y, rg, (0, 1), (1,), torch.zeros(2, 4, dtype=torch.int32, device=dev), S=2),
                lambda: f(x, y, rg, (0, 1), (1,), S=-1)):   # shapes
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        f(x.half(), y.half(), rg, (0, 1), (1,), S=2)
    wide = torch.arange(16, dtype=torch.int32, device=dev).expand(1, 4, 16).contiguous()
    with pytest.raises(ValueError):             # r = 16 is outside the band kernels
        f(torch.zeros(1, 2, 4, 16, device=dev), torch.zeros(1, 1, 4, 16, device=dev), wide, (0, 1), (1,), S=15)
    for bad in (lambda: f(x, y.cpu(), rg, (0, 1), (1,), S=2), lambda: f(x.cpu(), y.cpu(), rg.cpu(), (0, 1), (1,), S=2)):
        with pytest.raises(RuntimeError):       # an operand that is not on the GPU: as mutual_information_recursion_tdt_band raises it
            bad()
    # an int64 boundary and strided views are taken as they are
    a = f(x, y, rg, (0, 1), (1,), torch.tensor([[0, 0, 2, 4]], device=dev), S=2)
    bx = torch.zeros(1, 2, 4, 6, device=dev)
    b = f(bx[..., ::2], y, rg, (0, 1), (1,), torch.tensor([[0, 0, 2, 4]], dtype=torch.int32, device=dev), S=2)
    _equal(a, b)
