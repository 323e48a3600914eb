"""Float32 numpy restatement of the best-path alignment over the TDT / multi-blank lattice
(tf_fast_rnnt.mutual_information_viterbi_tdt, csrc/mi_viterbi_tdt.hip).

Moves m = 0..M-1: the token moves in list order, then the blank moves in list order.  For a cell (s,t) other than
(s_begin,t_begin)

    cand[m] = p[src_m] + op_m[src_m]          one float32 add; src_m = (s-1, t-e_i) for a token move, (s, t-d_j) for a
                                              blank move; -inf when src_m lies outside the boundary rectangle
    best, move = cand[M-1], M-1
    for m = M-2 .. 0:
        take = (cand[m] != cand[m]) or (cand[m] >= best)
        if take: best, move = cand[m], m
    p[s,t] = best

with p[s_begin,t_begin] = 0 and score = p[s_end,t_end]: a NaN propagates, a tie goes to the lowest-index move.  Vectorised
along the anti-diagonals s + t = k (every source lies on a strictly earlier diagonal, also for duration 0); every value is
one add per move and ordered selects, so any order that respects the dependencies gives the same bits.  Boundaries are
clamped into the lattice as the kernels do."""
import numpy as np

NEG = np.float32(-np.inf)


def _bounds(boundary, b, S, T):
    if boundary is None:
        return 0, 0, S, T
    sb, tb, se, te = (int(v) for v in boundary[b])
    return max(sb, 0), max(tb, 0), min(se, S), min(te, T)


def _shapes(px, py, tok, blk):
    px = np.asarray(px, np.float32); py = np.asarray(py, np.float32)
    B, Dx, S, T1 = px.shape
    T = py.shape[3]
    assert T1 == T + 1 and py.shape == (B, len(blk), S + 1, T) and Dx == len(tok), (px.shape, py.shape, tok, blk)
    return px, py, B, S, T


def _forward(px_b, py_b, tok, blk, sb, tb, Sn, Tn):
    """p [Sn,Tn] and the chosen move index [Sn,Tn] of one utterance (relative coordinates)."""
    M = len(tok) + len(blk)
    p = np.full((Sn, Tn), NEG, np.float32)
    mv = np.zeros((Sn, Tn), np.int8)
    p[0, 0] = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(1, Sn + Tn - 1):
            r = np.arange(max(0, k - Tn + 1), min(Sn - 1, k) + 1)
            t = k - r
            cand = np.full((M, r.size), NEG, np.float32)
            for i, e in enumerate(tok):
                m = (r >= 1) & (t >= e)
                cand[i, m] = p[r[m] - 1, t[m] - e] + px_b[i, sb + r[m] - 1, tb + t[m] - e]
            for j, d in enumerate(blk):
                m = t >= d
                cand[len(tok) + j, m] = p[r[m], t[m] - d] + py_b[j, sb + r[m], tb + t[m] - d]
            best = cand[M - 1].copy()
            move = np.full(r.size, M - 1, np.int8)
            for m_ in range(M - 2, -1, -1):
                c = cand[m_]
                take = (c != c) | (c >= best)
                best = np.where(take, c, best)
                move = np.where(take, np.int8(m_), move)
            p[r, t] = best
            mv[r, t] = move
    return p, mv


def viterbi_tdt(px, py, token_durations, blank_durations, boundary=None):
    """px [B,Dx,S,T+1], py [B,Dy,S+1,T] float32; boundary int [B,4] or None.  Returns (score [B] float32, frames [B,S],
    durations [B,S], blank_steps [B,T], all int32) with the conventions of mutual_information_viterbi_tdt."""
    tok = tuple(int(d) for d in token_durations); blk = tuple(int(d) for d in blank_durations)
    px, py, B, S, T = _shapes(px, py, tok, blk)
    score = np.zeros(B, np.float32)
    frames = np.full((B, S), -1, np.int32)
    durations = np.full((B, S), -1, np.int32)
    blank_steps = np.full((B, T), -1, np.int32)
    for b in range(B):
        sb, tb, se, te = _bounds(boundary, b, S, T)
        Sn, Tn = se - sb + 1, te - tb + 1
        if Sn <= 0 or Tn <= 0:
            continue
        p, mv = _forward(px[b], py[b], tok, blk, sb, tb, Sn, Tn)
        sc = p[Sn - 1, Tn - 1]
        score[b] = sc
        if sc != sc or sc == NEG:
            continue
        blank_steps[b, tb:te] = 0
        r, t = Sn - 1, Tn - 1
        while r > 0 or t > 0:
            m = int(mv[r, t])
            if m < len(tok):
                t -= tok[m]; r -= 1
                frames[b, sb + r] = tb + t
                durations[b, sb + r] = tok[m]
            else:
                d = blk[m - len(tok)]
                t -= d
                blank_steps[b, tb + t] = d
            assert r >= 0 and t >= 0
    return score, frames, durations, blank_steps


def brute_force(px, py, token_durations, blank_durations, boundary=None):
    """The maximum over every path of its operands summed left to right in float32 (-inf when there is no path, 0 for an
    inverted rectangle).  Score only: which of several equal paths wins is the recursion's tie rule, not a property of
    the set of paths."""
    tok = tuple(int(d) for d in token_durations); blk = tuple(int(d) for d in blank_durations)
    px, py, B, S, T = _shapes(px, py, tok, blk)
    score = np.zeros(B, np.float32)
    for b in range(B):
        sb, tb, se, te = _bounds(boundary, b, S, T)
        if se < sb or te < tb:
            continue
        best = [NEG, False]

        def walk(s, t, acc):
            if s == se and t == te:
                if acc != acc:
                    best[1] = True
                elif acc > best[0]:
                    best[0] = acc
                return
            for j, d in enumerate(blk):
                if t + d <= te:
                    walk(s, t + d, np.float32(acc + py[b, j, s, t]))
            if s < se:
                for i, e in enumerate(tok):
                    if t + e <= te:
                        walk(s + 1, t + e, np.float32(acc + px[b, i, s, t]))

        with np.errstate(invalid="ignore", over="ignore"):
            walk(sb, tb, np.float32(0))
        assert not best[1], "brute_force is for NaN-free operands"
        score[b] = best[0]
    return score


def replay(px, py, token_durations, blank_durations, boundary, frames, durations, blank_steps):
    """Walks the returned path of every utterance from (s_begin,t_begin): at (s,t) the token move when frames[s] == t,
    else the blank move blank_steps[t].  Asserts that it arrives at (s_end,t_end) and returns the float32 left-to-right
    sums [B] (NaN for an utterance without a path, whose outputs are all -1)."""
    tok = tuple(int(d) for d in token_durations); blk = tuple(int(d) for d in blank_durations)
    px, py, B, S, T = _shapes(px, py, tok, blk)
    out = np.full(B, np.nan, np.float32)
    for b in range(B):
        sb, tb, se, te = _bounds(boundary, b, S, T)
        if se < sb or te < tb:
            continue
        if (se > sb and frames[b, sb] < 0) or (te > tb and blank_steps[b, tb] < 0):
            continue
        acc, s, t = np.float32(0), sb, tb
        with np.errstate(invalid="ignore", over="ignore"):
            while s < se or t < te:
                if s < se and frames[b, s] == t:
                    e = int(durations[b, s])
                    acc = np.float32(acc + px[b, tok.index(e), s, t]); s += 1; t += e
                else:
                    assert t < te, (b, s, t)
                    d = int(blank_steps[b, t])
                    assert d > 0, (b, s, t, d)
                    acc = np.float32(acc + py[b, blk.index(d), s, t]); t += d
                assert s <= se and t <= te, (b, s, t)
        out[b] = acc
    return out
