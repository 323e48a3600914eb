"""Best-path alignment over the TDT / multi-blank lattice, CPU side: the float32 restatement
(tests/viterbi_tdt_restatement.py) against brute-force enumeration of every path and against the ordinary restatement
(tests/viterbi_restatement.py) for the moves (0,) / (1,), its tie rule on a hand-built lattice, the exported surface, and
the error paths of the C entry that need no device."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import viterbi_restatement as VR
import viterbi_tdt_restatement as VT

NEG = np.float32(-np.inf)
MOVE_SETS = [((0,), (1, 2)), ((0, 1, 2), (1, 2)), ((1, 2), (1,)), ((0, 3), (2,))]


def _bits(x):
    return np.asarray(x, np.float32).view(np.int32)


def _operands(rng, B, S, T, tok, blk, integer):
    if integer:
        px = rng.integers(-3, 1, (B, len(tok), S, T + 1)).astype(np.float32)
        py = rng.integers(-3, 1, (B, len(blk), S + 1, T)).astype(np.float32)
    else:
        px = rng.standard_normal((B, len(tok), S, T + 1)).astype(np.float32)
        py = rng.standard_normal((B, len(blk), S + 1, T)).astype(np.float32)
    return px, py


def _boundary(S, T):
    sb, tb = min(1, S), min(1, T)
    return np.array([[0, 0, S, T], [sb, tb, S, T], [sb, min(2, T), max(S - 1, sb), T]], np.int32)


@pytest.mark.parametrize("integer", [False, True], ids=["normal", "ties"])
@pytest.mark.parametrize("moves", MOVE_SETS, ids=str)
def test_restatement_matches_brute_force_and_replays(moves, integer):
    """Every S <= 3, T <= 5 (lattices without any path included): the score is the brute-force maximum bit for bit, and
    re-summing the operands along the returned path gives the score bits wherever it is finite."""
    tok, blk = moves
    rng = np.random.default_rng(31 + 5 * len(tok) + blk[-1] + integer)
    finite = 0
    for S in range(0, 4):
        for T in range(0, 6):
            px, py = _operands(rng, 3, S, T, tok, blk, integer)
            for bd in (None, _boundary(S, T)):
                score, frames, durs, steps = VT.viterbi_tdt(px, py, tok, blk, bd)
                want = VT.brute_force(px, py, tok, blk, bd)
                assert np.array_equal(_bits(score), _bits(want)), (S, T, score, want)
                again = VT.replay(px, py, tok, blk, bd, frames, durs, steps)
                for b in range(3):
                    if np.isfinite(score[b]):
                        finite += 1
                        assert _bits(again[b]) == _bits(score[b]), (S, T, b, again[b], score[b])
                        assert set(durs[b][durs[b] >= 0]) <= set(tok) and set(steps[b][steps[b] > 0]) <= set(blk)
                    else:
                        assert score[b] == NEG and (frames[b] == -1).all() and (durs[b] == -1).all() and (steps[b] == -1).all()
    assert finite > 20


@pytest.mark.parametrize("integer", [False, True], ids=["normal", "ties"])
def test_restatement_0_1_is_the_ordinary_restatement(integer):
    rng = np.random.default_rng(7 + integer)
    for S, T in [(0, 4), (3, 0), (1, 1), (3, 5), (7, 12), (12, 7)]:
        px, py = _operands(rng, 3, S, T, (0,), (1,), integer)
        for bd in (None, _boundary(S, T)):
            score, frames, durs, steps = VT.viterbi_tdt(px, py, (0,), (1,), bd)
            o_score, o_frames = VR.viterbi(px[:, 0], py[:, 0], bd)
            assert np.array_equal(_bits(score), _bits(o_score)) and np.array_equal(frames, o_frames)
            assert np.array_equal(durs, np.where(frames >= 0, 0, -1))
            assert set(np.unique(steps)) <= {-1, 0, 1}
            for b in range(3):
                sb, tb, se, te = VT._bounds(bd, b, S, T)
                if se >= sb and te >= tb:
                    assert set(steps[b, tb:te]) <= {0, 1} and (steps[b, :tb] == -1).all() and (steps[b, te:] == -1).all()


def test_restatement_ties_go_to_the_lowest_index_move():
    """S = 1, T = 2, token durations (0, 1), blank durations (1, 2), every operand 0 but the ones set below.  The cell
    (1,2) is reached with the sum -1 by token e=0 from (0,2), by token e=1 from (0,1) and by the blanks from (1,1) and
    (1,0): the token of duration 0 (move 0) must be reported.  With that move at -inf the token of duration 1 (move 1)
    ties with the blank of duration 1 (move 2) and wins; with both tokens into (1,2) at -inf the blank of duration 1
    beats the blank of duration 2."""
    tok, blk = (0, 1), (1, 2)
    px = np.zeros((1, 2, 1, 3), np.float32); py = np.zeros((1, 2, 2, 2), np.float32)
    py[0, :, 0, :] = -0.5        # row 0: p[0,1] = -0.5, p[0,2] = -0.5 (blank 2) or -1 (two blanks): -0.5
    px[0, 0, 0, 2] = -0.5        # token e=0 from (0,2): -0.5 - 0.5 = -1
    px[0, 1, 0, 1] = -0.5        # token e=1 from (0,1): -0.5 - 0.5 = -1
    px[0, 0, 0, 0] = -1.0; px[0, 0, 0, 1] = -0.5; px[0, 1, 0, 0] = -1.0     # p[1,0] = -1, p[1,1] = -1 (tie: token e=0)
    # blanks into (1,2): from (1,1) = -1 + 0, from (1,0) = -1 + 0
    score, frames, durs, steps = VT.viterbi_tdt(px, py, tok, blk)
    assert score[0] == -1.0 and frames.tolist() == [[2]] and durs.tolist() == [[0]] and steps.tolist() == [[2, 0]]
    px[0, 0, 0, 2] = NEG
    score, frames, durs, steps = VT.viterbi_tdt(px, py, tok, blk)
    assert score[0] == -1.0 and frames.tolist() == [[1]] and durs.tolist() == [[1]] and steps.tolist() == [[1, 0]]
    px[0, 1, 0, 1] = NEG
    score, frames, durs, steps = VT.viterbi_tdt(px, py, tok, blk)
    # (1,2) from (1,1) by blank 1; (1,1) from (0,1) by token e=0 (-0.5 - 0.5) tying token e=1 from (0,0) (-1): move 0
    assert score[0] == -1.0 and frames.tolist() == [[1]] and durs.tolist() == [[0]] and steps.tolist() == [[1, 1]]


def test_restatement_edges():
    tok, blk = (0, 2), (1, 3)
    px = np.zeros((3, 2, 3, 6), np.float32); py = np.zeros((3, 2, 4, 5), np.float32)
    bd = np.array([[1, 2, 1, 2], [2, 3, 1, 1], [0, 0, 3, 5]], np.int32)      # empty, inverted, full
    px[2] = NEG                                                               # no path
    score, frames, durs, steps = VT.viterbi_tdt(px, py, tok, blk, bd)
    assert score.tolist() == [0.0, 0.0, -np.inf]
    assert (frames == -1).all() and (durs == -1).all() and (steps == -1).all()
    px[2] = 0; px[2, 1, 1, 2] = np.nan
    score, frames, durs, steps = VT.viterbi_tdt(px, py, tok, blk, bd)
    assert np.isnan(score[2]) and (frames[2] == -1).all() and (durs[2] == -1).all() and (steps[2] == -1).all()


SYMBOLS = ("ftr_mutual_information_viterbi_tdt_workspace_bytes", "ftr_mutual_information_viterbi_tdt_f32")


def test_viterbi_tdt_surface_is_exported(ft):
    handle = ctypes.CDLL(ft._lib.LIB_PATH)
    for n in SYMBOLS:
        assert hasattr(handle, n) and n in ft._lib.EXPORTED_SYMBOLS, n
    L = ft._lib.lib()
    assert L.ftr_abi_version() == 133 and ft.__version__ == "1.2"
    assert L.ftr_mutual_information_viterbi_tdt_workspace_bytes(2, 3, 4) > 0
    assert L.ftr_mutual_information_viterbi_tdt_workspace_bytes(-1, 3, 4) == 0
    # half a byte per cell of the skewed 64-row blocks plus the strip carry: below one byte per lattice cell on a
    # lattice that is not tiny
    B, S, T = 4, 1023, 4000
    assert L.ftr_mutual_information_viterbi_tdt_workspace_bytes(B, S, T) <= B * (S + 1) * (T + 1)
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(ft.mutual_information_viterbi_tdt) == ["px", "py", "token_durations", "blank_durations", "boundary"]
    assert sig(ft.rnnt_alignment_tdt_pruned) == ["logits", "symbols", "ranges", "termination_symbol", "durations", "boundary",
                                                 "sigma"]
    assert sig(ft.rnnt_alignment_multiblank_pruned) == ["logits", "symbols", "ranges", "termination_symbol", "big_blanks",
                                                        "boundary", "sigma"]
    for f in (ft.rnnt_alignment_tdt_pruned, ft.rnnt_alignment_multiblank_pruned):
        p = inspect.signature(f).parameters
        assert p["boundary"].default is None and p["sigma"].default == 0.0


def _arr(vals):
    return (ctypes.c_int32 * max(len(vals), 1))(*vals)


def _call(L, tok, blk, ws_bytes=0, ws=None, out=None):
    """B=1 S=2 T=4 with null device pointers: only argument validation can answer (FTR_ERR_INVALID_ARG = 0)."""
    return L.ftr_mutual_information_viterbi_tdt_f32(out, out, None, _arr(tok), len(tok), _arr(blk), len(blk), ws, ws_bytes,
                                                    out, out, out, out, 1, 2, 4, None)


def test_viterbi_tdt_argument_validation_without_device(ft):
    L = ft._lib.lib()
    err = lambda: L.ftr_last_error()
    for tok in ((2, 1), (0, 0), (17,), (-1,), ()):                         # unsorted, repeated, above 16, negative, empty
        assert _call(L, tok, (1,)) == 0 and b"token_durations" in err(), (tok, err())
    for blk in ((3, 2), (1, 1), (0,), (0, 1), (33,), (1, 33), ()):          # unsorted, repeated, 0, above 32, empty
        assert _call(L, (0,), blk) == 0 and b"blank_durations" in err(), (blk, err())
    assert _call(L, (0, 1, 2, 3, 4), (1, 2, 3, 4, 5)) == 0 and b"Dx + Dy" in err()       # 10 moves
    # valid lists (a blank of 32 and nine moves among them) get as far as the workspace check
    need = L.ftr_mutual_information_viterbi_tdt_workspace_bytes(1, 2, 4)
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    for tok, blk in (((0,), (1, 32)), ((0, 1, 2, 3, 4), (1, 2, 3, 4)), ((0, 16), (3, 16)), ((1, 2), (1,)), ((0,), (1,))):
        assert _call(L, tok, blk, need - 1, a, a) == 0
        assert b"durations" not in err() and b"too small" in err(), err()
        assert _call(L, tok, blk, need, None, a) == 0 and b"null" in err(), err()
    assert L.ftr_mutual_information_viterbi_tdt_f32(None, None, None, _arr((0,)), 1, _arr((1,)), 1, None, 0, None, None, None,
                                                    None, -1, 2, 4, None) == 0 and b"negative" in err()
    assert L.ftr_mutual_information_viterbi_tdt_f32(None, None, None, _arr((0,)), 1, _arr((1,)), 1, None, 0, None, None, None,
                                                    None, 0, 2, 4, None) == 1                      # B == 0
    # the loss keeps its own limit: a blank above 16 is this entry's alone
    assert L.ftr_mutual_information_tdt_fwd_f32(None, None, None, _arr((0,)), 1, _arr((1, 17)), 2, None, 0, None, 1, 2, 4,
                                                None) == 0 and b"blank_durations" in err()


def test_viterbi_tdt_python_validation(ft):
    """Raised before anything touches a device; CPU tensors are refused, there is no CPU fallback."""
    px, py = torch.zeros(1, 1, 2, 5), torch.zeros(1, 2, 3, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ft.mutual_information_viterbi_tdt(px, py, (0,), (1, 32))
    logits = torch.zeros(1, 4, 2, 8)
    sym = torch.zeros(1, 2, dtype=torch.int32)
    ranges = torch.zeros(1, 4, 2, dtype=torch.int32) + torch.arange(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ft.rnnt_alignment_tdt_pruned(logits, sym, ranges, 4, (0, 1, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ft.rnnt_alignment_multiblank_pruned(logits, sym, ranges, 7, ((5, 2), (6, 4)))
    from tf_fast_rnnt.mutual_information import _check_tdt_moves
    assert _check_tdt_moves((0,), (1, 32), blank_hi=32) == ((0,), (1, 32))
    with pytest.raises(ValueError, match="blank_durations"):
        _check_tdt_moves((0,), (1, 33), blank_hi=32)
    with pytest.raises(ValueError, match="blank_durations"):
        _check_tdt_moves((0,), (1, 17))                        # the loss keeps 16
