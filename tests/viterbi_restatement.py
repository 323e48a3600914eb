"""Float32 numpy restatement of the best-path (Viterbi) alignment (tf_fast_rnnt.mutual_information_viterbi).

The recursion of mutual_information_recursion with LogAdd replaced by a select:

    a = p[s-1, t+off] + px[s-1, t+off]   (off = 0 regular, -1 modified; -inf where the recursion's guards say so)
    c = p[s, t-1] + py[s, t-1]
    take_px = (a != a) | (a >= c)
    p[s, t] = where(take_px, a, c)

Vectorised along anti-diagonals (regular) and along columns (modified); every value is one float32 add and one
select, so the result is bit-identical to any other order that respects the dependencies.  Boundaries are clamped
into the lattice as the kernels do."""
import numpy as np

NEG = np.float32(-np.inf)


def _bounds(boundary, b, S, T):
    if boundary is None:
        return 0, 0, S, T
    sb, tb, se, te = (int(v) for v in boundary[b])
    return max(sb, 0), max(tb, 0), min(se, S), min(te, T)


def _forward(x, y, Sn, Tn, modified):
    """x = px[sb:se, tb+off...] as [Sn-1, Tn] (column t holds the px operand of column t, NaN-free padding unused),
    y = py[sb:se+1, tb:te] as [Sn, Tn-1].  Returns p [Sn, Tn] and the take_px decisions [Sn, Tn]."""
    p = np.full((Sn, Tn), NEG, np.float32)
    d = np.zeros((Sn, Tn), bool)
    p[0, 0] = 0
    with np.errstate(invalid="ignore", over="ignore"):
        if modified:
            # column t from column t-1: a = p[r-1, t-1] + px[r-1, t-1]; c = p[r, t-1] + py[r, t-1]
            for t in range(1, Tn):
                a = np.full(Sn, NEG, np.float32)
                a[1:] = p[:-1, t - 1] + x[:, t]
                c = p[:, t - 1] + y[:, t - 1]
                tp = (a != a) | (a >= c)
                p[:, t] = np.where(tp, a, c)
                d[:, t] = tp
            d[1:, 0] = True                     # a = c = -inf at t = 0: the select takes a
        else:
            for k in range(1, Sn + Tn - 1):     # anti-diagonal r + t = k
                r = np.arange(max(0, k - Tn + 1), min(Sn - 1, k) + 1)
                t = k - r
                a = np.full(r.shape, NEG, np.float32)
                m = r >= 1
                a[m] = p[r[m] - 1, t[m]] + x[r[m] - 1, t[m]]
                c = np.full(r.shape, NEG, np.float32)
                m = t >= 1
                c[m] = p[r[m], t[m] - 1] + y[r[m], t[m] - 1]
                tp = (a != a) | (a >= c)
                p[r, t] = np.where(tp, a, c)
                d[r, t] = tp
    return p, d


def viterbi(px, py, boundary=None):
    """px [B,S,T+1] (regular) or [B,S,T] (modified), py [B,S+1,T] float32; boundary int [B,4] or None.
    Returns (score [B] float32, frames [B,S] int32) with the conventions of mutual_information_viterbi."""
    px = np.asarray(px, np.float32); py = np.asarray(py, np.float32)
    B, S, T1 = px.shape
    T = py.shape[2]
    modified = T1 == T
    off = -1 if modified else 0
    score = np.zeros(B, np.float32)
    frames = np.full((B, S), -1, np.int32)
    for b in range(B):
        sb, tb, se, te = _bounds(boundary, b, S, T)
        Sn, Tn = se - sb + 1, te - tb + 1
        if Sn <= 0 or Tn <= 0:
            continue
        # px operand of relative cell (r, t) (r >= 1): px[sb + r - 1, tb + t + off]; x[r-1, t]
        x = np.full((max(Sn - 1, 0), Tn), NEG, np.float32)
        for t in range(Tn):
            col = tb + t + off
            if 0 <= col < T1 and Sn > 1 and t + off >= 0:
                x[:, t] = px[b, sb:se, col]
        y = py[b, sb:se + 1, tb:te] if Tn > 1 else np.zeros((Sn, 0), np.float32)
        p, d = _forward(x, y, Sn, Tn, modified)
        sc = p[Sn - 1, Tn - 1]
        score[b] = sc
        if sc != sc or sc == NEG:
            continue
        r, t = Sn - 1, Tn - 1
        while r > 0:
            if d[r, t]:
                t = t + off
                frames[b, sb + r - 1] = tb + t
                r -= 1
            else:
                t -= 1
    return score, frames


def brute_force(px, py, boundary=None):
    """Every monotone path, summed left to right in float32; the maximum and the frames of the maximising path."""
    px = np.asarray(px, np.float32); py = np.asarray(py, np.float32)
    B, S, T1 = px.shape
    T = py.shape[2]
    modified = T1 == T
    score = np.zeros(B, np.float32)
    frames = np.full((B, S), -1, np.int32)
    for b in range(B):
        sb, tb, se, te = _bounds(boundary, b, S, T)
        best = [NEG, None]

        def walk(s, t, acc, fr):
            if s == se and t == te:
                if best[1] is None or acc > best[0]:
                    best[0], best[1] = acc, list(fr)
                return
            if t < te:                                       # py move
                walk(s, t + 1, np.float32(acc + py[b, s, t]), fr)
            if s < se and (not modified or t < te):          # px move out of row s at frame t
                walk(s + 1, t + 1 if modified else t, np.float32(acc + px[b, s, t]), fr + [t])

        with np.errstate(invalid="ignore", over="ignore"):
            walk(sb, tb, np.float32(0), [])
        score[b] = best[0] if best[1] is not None else NEG
        if best[1] is not None and best[0] != NEG:
            frames[b, sb:se] = best[1]
    return score, frames
