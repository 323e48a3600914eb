"""Best-path alignment over the TDT / multi-blank lattice on the device (csrc/mi_viterbi_tdt.hip): bit-exact against the
float32 restatement (tests/viterbi_tdt_restatement.py) in all four outputs, against mutual_information_viterbi for the
moves (0,) / (1,), properties that do not depend on the restatement, the edge conventions, the two pruned wrappers, views,
graph capture.  Every comparison is exact: a cell is one float32 add per move and ordered selects."""
import functools

import numpy as np
import pytest
import torch

import viterbi_tdt_restatement as VT
from test_gpu_graph import _capture
from test_gpu_tdt import _lattice

pytestmark = pytest.mark.gpu

NEG = np.float32(-np.inf)
# rows 64 and 65 (the wave boundary), a full strip of 256 rows and the strip carry (S + 1 = 257, 301, 1101), S + 1 = 129,
# and the chunk boundary at T = 8, 9
SHAPES = [(2, 0, 9), (2, 5, 1), (3, 12, 40), (2, 63, 9), (2, 64, 33), (2, 128, 17), (1, 256, 8), (1, 300, 25), (1, 1100, 6),
          (2, 50, 200)]
MOVES = [((0,), (1,)), ((0,), (1, 2, 4, 8)), ((0,), (1, 32)), ((0, 1, 2, 3, 4), (1, 2, 3, 4)), ((1, 2), (1,)),
         ((0, 16), (3, 16)), ((0, 5, 6, 7), (1, 9))]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _n(t):
    return t.detach().cpu().numpy()


def _bits(x):
    return np.asarray(x, np.float32).view(np.int32)


def _fit(moves, T):
    """T <= 9: the durations of each list that fit into T frames (the shortest one stays when none does: a move that
    never fits is a valid description, it is simply never taken)."""
    if T > 9:
        return moves
    return tuple(tuple(d for d in m if d <= T) or m[:1] for m in moves)


def _run(ft, dev, px, py, tok, blk, bd):
    out = ft.mutual_information_viterbi_tdt(_t(px, dev), _t(py, dev), tok, blk, None if bd is None else _t(bd, dev))
    torch.cuda.synchronize()
    return tuple(_n(o) for o in out)


def _same(got, want, what=""):
    assert np.array_equal(_bits(got[0]), _bits(want[0])), (what, got[0], want[0])
    for name, g, w in zip(("frames", "durations", "blank_steps"), got[1:], want[1:]):
        assert g.dtype == np.int32 and g.shape == w.shape, (what, name)
        for b in range(g.shape[0]):
            assert np.array_equal(g[b], w[b]), (what, name, b, np.nonzero(g[b] != w[b])[0][:10])


@functools.lru_cache(maxsize=None)
def _case(shape, moves, with_boundary, integer):
    """The lattice of test_gpu_tdt.py (standard normal, 2 % -inf, thinned on tall lattices; the sub-rectangle boundary of
    that file) and the restatement's answer, computed once."""
    B, S, T = shape
    tok, blk = moves
    px, py, bd = _lattice(B, S, T, len(tok), len(blk), 17 * S + T + len(tok) + 3 * len(blk), with_boundary)
    if integer:   # ties decide most cells (rint keeps -inf)
        px, py = np.rint(px).astype(np.float32), np.rint(py).astype(np.float32)
    return px, py, bd, VT.viterbi_tdt(px, py, tok, blk, bd)


@pytest.mark.parametrize("with_boundary", [False, True], ids=["full", "subrect"])
@pytest.mark.parametrize("moves", MOVES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_bit_exact_against_restatement(ft, dev, shape, moves, with_boundary):
    moves = _fit(moves, shape[2])
    tok, blk = moves
    for integer in (False, True):
        px, py, bd, want = _case(shape, moves, with_boundary, integer)
        if 0 in tok and 1 in blk:
            assert np.isfinite(want[0]).any(), "the inputs of a case must leave some utterance a path"
        got = _run(ft, dev, px, py, tok, blk, bd)
        _same(got, want, (shape, moves, with_boundary, integer))
        if tok == (0,) and blk == (1,):   # the ordinary lattice: the ordinary kernel's score and frames, on the GPU
            o_score, o_frames = ft.mutual_information_viterbi(_t(px[:, 0], dev), _t(py[:, 0], dev),
                                                              None if bd is None else _t(bd, dev))
            assert np.array_equal(_bits(_n(o_score)), _bits(got[0])) and np.array_equal(_n(o_frames), got[1])
            assert np.array_equal(got[2], np.where(got[1] >= 0, 0, -1)) and set(np.unique(got[3])) <= {-1, 0, 1}


@pytest.mark.parametrize("moves", [((0,), (1, 2, 4, 8)), ((0, 1, 2, 3, 4), (1, 2, 3, 4)), ((0, 5, 6, 7), (1, 9))], ids=str)
def test_properties_of_the_result_alone(ft, dev, moves):
    """The outputs describe a path whose float32 left-to-right sum is the score; the score is at most the log-sum over
    all paths (float32 rounding of `ans` allowed: 1e-4 relative, the project's parity rule); a token move starts no
    earlier than the one before it ended; two runs are bit-identical; the outputs are detached."""
    tok, blk = moves
    B, S, T = 3, 150, 260
    rng = np.random.default_rng(23)
    px = (rng.standard_normal((B, len(tok), S, T + 1)) - 1).astype(np.float32)
    py = (rng.standard_normal((B, len(blk), S + 1, T)) - 1).astype(np.float32)
    bd = np.array([[0, 0, S, T], [3, 5, S - 20, T - 31], [0, 0, S, T - 1]], np.int32)
    tpx, tpy, tbd = _t(px, dev), _t(py, dev), _t(bd, dev)
    out1 = ft.mutual_information_viterbi_tdt(tpx, tpy, tok, blk, tbd)
    out2 = ft.mutual_information_viterbi_tdt(tpx.clone().requires_grad_(True), tpy, tok, blk, tbd)
    assert not any(o.requires_grad for o in out2)
    assert torch.equal(out1[0].view(torch.int32), out2[0].view(torch.int32))
    assert all(torch.equal(a, b) for a, b in zip(out1[1:], out2[1:]))
    score, frames, durs, steps = (_n(o) for o in out1)
    assert np.isfinite(score).all()
    again = VT.replay(px, py, tok, blk, bd, frames, durs, steps)
    assert np.array_equal(_bits(again), _bits(score)), (again, score)
    ans = _n(ft.mutual_information_recursion_tdt(tpx, tpy, tok, blk, tbd))
    assert (score <= ans + 1e-4 * np.abs(ans)).all(), (score, ans)
    for b in range(B):
        sb, tb, se, te = bd[b]
        f, d = frames[b, sb:se], durs[b, sb:se]
        assert set(d) <= set(tok) and (f >= tb).all() and (f + d <= te).all()
        assert (f[1:] >= f[:-1] + d[:-1]).all() and (np.diff(f + d) >= 0).all()
        assert (frames[b, :sb] == -1).all() and (frames[b, se:] == -1).all() and (durs[b, se:] == -1).all()
        assert set(steps[b, tb:te]) <= {0, *blk} and (steps[b, :tb] == -1).all() and (steps[b, te:] == -1).all()


def test_edges_in_one_batch(ft, dev):
    """No path: score -inf and all -1.  A NaN confined to one utterance: score NaN and all -1 there, the neighbours
    bit-identical to a run without it.  An inverted rectangle: score 0 and all -1.  S = 0."""
    tok, blk = (0, 2), (1, 3)
    B, S, T = 5, 70, 40
    px, py, _ = _lattice(B, S, T, 2, 2, 3, False)
    bd = np.array([[0, 0, S, T], [0, 0, S, T], [1, 2, S - 3, T - 1], [9, 4, 3, 30], [2, 0, S, T - 5]], np.int32)
    base = _run(ft, dev, px, py, tok, blk, bd)
    assert np.isfinite(base[0][[0, 1, 2, 4]]).all()
    px2, py2 = px.copy(), py.copy()
    px2[1, :, 30] = NEG                       # no token move out of row 30
    py2[2, 1, 40, 17] = np.nan                # inside utterance 2's rectangle
    py2[4, 0, 1, 3] = np.nan                  # row 1 lies below utterance 4's s_begin: no effect
    got = _run(ft, dev, px2, py2, tok, blk, bd)
    _same(got, VT.viterbi_tdt(px2, py2, tok, blk, bd))
    score, frames, durs, steps = got
    assert score[1] == NEG and np.isnan(score[2]) and score[3] == 0
    for b in (1, 2, 3):
        assert (frames[b] == -1).all() and (durs[b] == -1).all() and (steps[b] == -1).all()
    for b in (0, 4):
        assert _bits(score[b]) == _bits(base[0][b])
        assert all(np.array_equal(g[b], w[b]) for g, w in zip(got[1:], base[1:]))
    px0 = np.zeros((2, 2, 0, T + 1), np.float32)
    py0 = np.random.default_rng(1).standard_normal((2, 2, 1, T)).astype(np.float32)
    got0 = _run(ft, dev, px0, py0, tok, blk, None)
    assert got0[1].shape == (2, 0) and got0[2].shape == (2, 0)
    _same(got0, VT.viterbi_tdt(px0, py0, tok, blk, None))
    assert np.array_equal(_bits(VT.replay(px0, py0, tok, blk, None, *got0[1:])), _bits(got0[0]))


def test_recovers_a_planted_alignment(ft, dev):
    """One path with random token durations and blank steps at -0.1 / -0.05 per move, every other operand at
    N(-10, 0.5): a deviation trades at most five planted moves (>= -0.5) for a move below -7."""
    tok, blk = (0, 1, 2, 3, 4), (1, 2, 3, 4)
    B, S, T = 2, 70, 300
    rng = np.random.default_rng(5)
    px = (0.5 * rng.standard_normal((B, len(tok), S, T + 1)) - 10.0).astype(np.float32)
    py = (0.5 * rng.standard_normal((B, len(blk), S + 1, T)) - 10.0).astype(np.float32)
    frames = np.zeros((B, S), np.int32); durs = np.zeros((B, S), np.int32); steps = np.zeros((B, T), np.int32)
    for b in range(B):
        e = rng.integers(0, 5, S)
        rest, d = T - int(e.sum()), []
        while rest > 0:
            d.append(int(rng.integers(1, min(4, rest) + 1)))
            rest -= d[-1]
        order = rng.permutation(np.array([0] * S + [1] * len(d)))
        s = t = i = 0
        for is_blank in order:
            if is_blank:
                py[b, blk.index(d[i]), s, t] = -0.05
                steps[b, t] = d[i]
                t += d[i]; i += 1
            else:
                px[b, tok.index(e[s]), s, t] = -0.1
                frames[b, s], durs[b, s] = t, e[s]
                t += e[s]; s += 1
        assert s == S and t == T
    got = _run(ft, dev, px, py, tok, blk, None)
    _same(got, VT.viterbi_tdt(px, py, tok, blk, None))
    assert np.array_equal(got[1], frames) and np.array_equal(got[2], durs) and np.array_equal(got[3], steps)


def _pruned_inputs(ft, dev, width, termination_symbol, sym_lo, sym_hi):
    torch.manual_seed(3)
    B, T, S, C, r = 2, 40, 12, 16, 5
    am = torch.randn(B, T, C, device=dev); lm = torch.randn(B, S + 1, C, device=dev)
    sym = torch.randint(sym_lo, sym_hi, (B, S), device=dev, dtype=torch.int32)
    bd = torch.tensor([[0, 0, S, T], [0, 0, S - 3, T - 6]], dtype=torch.int32, device=dev)
    _, (gx, gy) = ft.rnnt_loss_simple(lm, am, sym, termination_symbol, bd, reduction="none", calc_gradients=True)
    ranges = ft.get_rnnt_prune_ranges(gx, gy, bd, r)
    logits = torch.randn(B, T, r, width, device=dev, requires_grad=True)
    joint = torch.randn(B, T, S + 1, width, device=dev)
    ident = torch.arange(S + 1, device=dev, dtype=torch.int32).expand(B, T, S + 1).contiguous()
    return logits, joint, sym, ranges, ident, bd


def _equal(a, b):
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))


def _in_band(out, ranges, bd, r):
    score, frames = _n(out[0]), _n(out[1])
    rg, bdn = _n(ranges), _n(bd)
    assert np.isfinite(score).all()
    for b in range(frames.shape[0]):
        for s in range(bdn[b, 2]):
            t = frames[b, s]
            assert 0 <= t < bdn[b, 3] and rg[b, t, 0] <= s < rg[b, t, 0] + r, (b, s, t, rg[b, t])
        assert (frames[b, bdn[b, 2]:] == -1).all()


def test_rnnt_alignment_tdt_pruned(ft, dev):
    durs, C, r = (0, 1, 2, 3, 4), 16, 5
    logits, joint, sym, ranges, ident, bd = _pruned_inputs(ft, dev, C + len(durs), C - 1, 0, C - 1)
    out = ft.rnnt_alignment_tdt_pruned(logits, sym, ranges, C - 1, durs, bd)
    assert not any(o.requires_grad for o in out) and out[2].shape == sym.shape and out[3].shape == (2, 40)
    px, py = ft.get_rnnt_logprobs_tdt_pruned(logits, sym, ranges, C - 1, durs, bd)
    _equal(out, ft.mutual_information_viterbi_tdt(px, py, durs, (1, 2, 3, 4), bd))
    _in_band(out, ranges, bd, r)
    assert set(np.unique(_n(out[2]))) <= {-1, *durs}
    _equal(ft.rnnt_alignment_tdt_pruned(joint, sym, ident, C - 1, durs, bd, sigma=0.05),
           ft.mutual_information_viterbi_tdt(*ft.get_rnnt_logprobs_tdt_joint(joint, sym, C - 1, durs, bd, sigma=0.05), durs,
                                             (1, 2, 3, 4), bd))
    with pytest.raises(ValueError):
        ft.rnnt_alignment_tdt_pruned(logits, sym, ranges, C - 1, (0, 1, 17), bd)


def test_rnnt_alignment_multiblank_pruned(ft, dev):
    big, C, r = ((13, 2), (14, 4), (15, 8)), 16, 5
    logits, joint, sym, ranges, ident, bd = _pruned_inputs(ft, dev, C, 0, 1, 13)
    out = ft.rnnt_alignment_multiblank_pruned(logits, sym, ranges, 0, big, bd)
    assert not any(o.requires_grad for o in out)
    px, py = ft.get_rnnt_logprobs_multiblank_pruned(logits, sym, ranges, 0, big, bd)
    _equal(out, ft.mutual_information_viterbi_tdt(px.unsqueeze(1), py, (0,), (1, 2, 4, 8), bd))
    _in_band(out, ranges, bd, r)
    assert np.array_equal(_n(out[2]), np.where(_n(out[1]) >= 0, 0, -1))      # a symbol stays on its frame
    assert set(np.unique(_n(out[3]))) <= {-1, 0, 1, 2, 4, 8}
    jpx, jpy = ft.get_rnnt_logprobs_multiblank_joint(joint, sym, 0, big, bd)
    _equal(ft.rnnt_alignment_multiblank_pruned(joint, sym, ident, 0, big, bd),
           ft.mutual_information_viterbi_tdt(jpx.unsqueeze(1), jpy, (0,), (1, 2, 4, 8), bd))
    # a big blank of 32 frames: beyond the loss's recursion, within the alignment's
    out32 = ft.rnnt_alignment_multiblank_pruned(joint, sym, ident, 0, ((13, 2), (14, 32)), bd)
    jpx, jpy = ft.get_rnnt_logprobs_multiblank_joint(joint, sym, 0, ((13, 2), (14, 32)), bd)
    _same(tuple(_n(o) for o in out32), VT.viterbi_tdt(_n(jpx)[:, None], _n(jpy), (0,), (1, 2, 32), _n(bd)))


def test_views_and_int64_boundary(ft, dev):
    """Strided and offset views of px / py and an int64 boundary give the bits of contiguous int32 inputs."""
    moves = ((0, 1, 2, 3, 4), (1, 2, 3, 4))
    px, py, bd, want = _case((3, 12, 40), moves, True, False)
    B, S, T = 3, 12, 40
    bx = torch.full((B, 5, S + 3, 2 * (T + 1) + 5), 7.0, device=dev)
    by = torch.full((B + 1, 4, S + 1, T + 4), 7.0, device=dev)
    vx = bx[:, :, 2:S + 2, 3:3 + 2 * (T + 1):2]
    vy = by[1:, :, :, 1:T + 1]
    vx.copy_(_t(px, dev)); vy.copy_(_t(py, dev))
    assert not vx.is_contiguous() and not vy.is_contiguous() and vx.storage_offset() > 0 and vy.storage_offset() > 0
    got = ft.mutual_information_viterbi_tdt(vx, vy, *moves, _t(bd, dev).to(torch.int64))
    _same(tuple(_n(o) for o in got), want)


def test_graph_capture_and_repeatability(ft, dev):
    """Captured once, replayed with new operand values written in place: each replay equals an eager run (kernels only,
    no memset / memcpy nodes; the duration lists are launch arguments).  Two eager runs are bit-identical."""
    tok, blk = (0, 1, 2, 3, 4), (1, 2, 3, 4)
    B, S, T = 2, 300, 120
    torch.manual_seed(4)
    px = torch.randn(B, len(tok), S, T + 1, device=dev); py = torch.randn(B, len(blk), S + 1, T, device=dev)
    bd = torch.tensor([[0, 0, S, T], [2, 1, S - 30, T - 7]], dtype=torch.int32, device=dev)
    g, out = _capture(lambda: ft.mutual_information_viterbi_tdt(px, py, tok, blk, bd))
    for i in range(2):
        px.copy_(torch.randn_like(px)); py.copy_(torch.randn_like(py))
        g.replay()
        torch.cuda.synchronize()
        e1 = ft.mutual_information_viterbi_tdt(px, py, tok, blk, bd)
        e2 = ft.mutual_information_viterbi_tdt(px, py, tok, blk, bd)
        torch.cuda.synchronize()
        _equal(out, e1)
        _equal(e1, e2)
    _same(tuple(_n(o) for o in e1), VT.viterbi_tdt(_n(px), _n(py), tok, blk, _n(bd)))
