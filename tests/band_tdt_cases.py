"""Band-shaped inputs for the band-native TDT recursion (csrc/mi_band_tdt.hip) and their float64 reference.  CPU only:
numpy, torch and tests/tdt_restatement.py.

Two things live here.

* The path, band and band <-> lattice helpers that tests/test_gpu_band_tdt.py has always used (`_random_path`,
  `_band_around`, `_scatter`, `_gather`): band element (b, plane, t, k) is lattice cell (ranges[b,t,k], t).

* STRUCTURED cases, the TDT counterpart of tests/band_cases.py: a planted path of the case's own moves, a band drawn
  around it, and value kinds that are not iid around one mean (`make_case`), with the float64 restatement on the band
  scattered into full-size lattices, occupancies gathered back to the band, as the reference (`reference`, once per case).

Geometry of a case.  A shape is (B, S, T, r) with one move list (token durations / blank durations, MOVES_OF).  Utterance 0
has the full rectangle; in B = 2 shapes utterance 1 has boundary (2, 5, S - 3, T - 7).  The planted path is `_random_path`
over the rectangle with the case's moves, the band `_band_around` it; both depend on the shape alone, so the seven kinds of
a shape share them.  Off-path values have the means and deviations of band_cases._values, on all N token planes and all Ny
blank planes; `sharp` puts -0.1 on the path's own token entries and -0.05 on its blank entries (an entry is (move plane,
frame, band row)); `holes` knocks out 10 % of the off-path entries, -1e20 in utterance 0 and -inf in the others.  Then the
builder's -inf rules are applied as `_recursion_case` of test_gpu_band_tdt.py applies them (no token out of row S or out of
a frame >= t_end, no move that lands past t_end)."""
import numpy as np

from band_cases import _values
from tdt_restatement import tdt_dp_with_grads

NEG = float("-inf")

KINDS = ["sharp", "two_regime", "blank_heavy", "tilted", "deep", "positive", "holes"]

# (B, S, T, r), its (token durations, blank durations), and what it is there for (M = N + Ny moves; 8 lanes for r <= 7,
# 16 above; lane = lattice row mod lanes)
CASES = [
    ((2, 20, 70, 4), ((0, 1, 2, 3, 4), (1, 2, 3, 4))),          # short base case, M = 9
    ((2, 100, 300, 8), ((1, 2, 3, 4, 8), (1, 2, 3, 4, 8))),     # M = 10, 16 lanes wrapped 6 times, no zero duration
    ((2, 100, 300, 7), ((0, 1, 2), (1, 2))),                    # M = 5, lanes = r + 1 = 8
    ((1, 250, 900, 15), ((0, 1, 2, 4), (1, 2, 4))),             # M = 7, lanes = r + 1 = 16, long
    ((1, 300, 1500, 5), ((0, 1, 2, 3, 4), (1, 2, 3, 4))),       # the shape of the memory test, with parity
    ((1, 120, 2000, 2), ((0, 16), (3, 16))),                    # ring of 32 steps, r = 2, the longest walk
    ((1, 500, 700, 12), ((0, 1, 3, 5), (1, 2, 4, 8))),          # M = 8, S comparable to T
]
SHAPES = [shape for shape, _ in CASES]
MOVES_OF = dict(CASES)


def shape_id(shape):
    B, S, T, r = shape
    tok, blk = MOVES_OF[shape]
    return f"B{B}S{S}T{T}r{r}_M{len(tok) + len(blk)}"


# ------------------------------------------------------------------------------------------------- bands and operands
def _random_path(rng, Sn, Tn, tok, blk, r):
    """A random path (0,0) -> (Sn-1,Tn-1) of the rectangle as [(s, t, move)] that climbs at most r - 1 rows inside one
    frame (the rows it visits at a frame must fit one band of r rows); None when there is none."""
    # reach[s,t,c]: the end can be reached from (s,t) after c climbs inside frame t
    reach = np.zeros((Sn + 1, Tn + 17, r + 1), bool)
    reach[Sn - 1, Tn - 1, :r] = True
    zero = 0 in tok
    for t in range(Tn - 2, -1, -1):             # sources are frames before the last column
        for s in range(Sn - 1, -1, -1):
            on = any(reach[s + 1, t + e, 0] for e in tok if e > 0) or any(reach[s, t + d, 0] for d in blk)
            for c in range(r - 1, -1, -1):
                reach[s, t, c] = on or (zero and c < r - 1 and reach[s + 1, t, c + 1])
    if not reach[0, 0, 0]:
        return None
    moves = [(1, e) for e in tok] + [(0, d) for d in blk]
    s, t, c, path = 0, 0, 0, []
    while (s, t) != (Sn - 1, Tn - 1):
        ok = [m for m, (ds, d) in enumerate(moves) if reach[s + ds, t + d, c + 1 if (ds == 1 and d == 0) else 0]
              and not (ds == 1 and d == 0 and c >= r - 1)]
        m = ok[rng.integers(len(ok))]
        path.append((s, t, m))
        ds, d = moves[m]
        c = c + 1 if (ds == 1 and d == 0) else 0
        s, t = s + ds, t + d
    return path


def _band_around(rng, path, sb, tb, te, S, T, r):
    """lo[t], non-decreasing, 0 <= lo <= S + 1 - r, holding every source cell of the path; flat wherever it may be."""
    lo_min = np.zeros(T, np.int64)               # frame t: lo >= (highest row visited) - r + 1
    lo_max = np.full(T, S + 1 - r, np.int64)     #          lo <= lowest row visited
    for s, t, _ in path:
        lo_min[tb + t] = max(lo_min[tb + t], sb + s - r + 1)
        lo_max[tb + t] = min(lo_max[tb + t], sb + s)
    for t in range(T - 2, -1, -1):               # a later frame's ceiling holds for the earlier ones (monotone)
        lo_max[t] = min(lo_max[t], lo_max[t + 1])
    lo = np.zeros(T, np.int64)
    prev = 0
    for t in range(T):
        lb, ub = max(prev, lo_min[t]), lo_max[t]
        assert lb <= ub
        if rng.random() < 0.25 and tb <= t < te:       # now and then a step the path does not ask for: 1..r rows, r itself
            lb = min(ub, lb + (r if rng.random() < 0.3 else rng.integers(1, r + 1)))      # among them
        lo[t] = prev = lb
    return lo


def _scatter(band, ranges, S, rows, cols):
    """band [B,P,T,r] -> lattice [B,P,rows,cols], -inf outside the band (band rows beyond the lattice are dropped)"""
    B, P, T, r = band.shape
    out = np.full((B, P, rows, cols), NEG, band.dtype)
    for b in range(B):
        for t in range(T):
            for k in range(r):
                s = int(ranges[b, t, k])
                if 0 <= s < rows:
                    out[b, :, s, t] = band[b, :, t, k]
    return out


def _gather(lat, ranges):
    """lattice [B,P,rows,cols] -> band [B,P,T,r], 0 for band rows beyond the lattice"""
    B, T, r = ranges.shape
    out = np.zeros((B, lat.shape[1], T, r), lat.dtype)
    for b in range(B):
        for t in range(T):
            for k in range(r):
                s = int(ranges[b, t, k])
                if 0 <= s < lat.shape[2] and t < lat.shape[3]:
                    out[b, :, t, k] = lat[b, :, s, t]
    return out


# --------------------------------------------------------------------------------------------------- structured cases
_GEOMETRY = {}


def _geometry(shape):
    """(bd [B,4] int64, paths: per utterance [(s, t, move)] relative to (s_begin, t_begin), lo [B,T]) of a shape."""
    if shape not in _GEOMETRY:
        B, S, T, r = shape
        tok, blk = MOVES_OF[shape]
        rng = np.random.default_rng([B, S, T, r, len(tok), len(blk)])
        bd = np.zeros((B, 4), np.int64)
        bd[:, 2], bd[:, 3] = S, T
        if B > 1:
            bd[1] = (2, 5, S - 3, T - 7)
        paths, lo = [], np.zeros((B, T), np.int64)
        for b in range(B):
            sb, tb, se, te = (int(v) for v in bd[b])
            path = _random_path(rng, se - sb + 1, te - tb + 1, tok, blk, r)
            assert path is not None, f"{shape}: the move list {tok}/{blk} has no path through utterance {b}'s rectangle"
            paths.append(path)
            lo[b] = _band_around(rng, path, sb, tb, te, S, T, r)
        _GEOMETRY[shape] = (bd, paths, lo)
    return _GEOMETRY[shape]


_CASES = {}


def make_case(kind, shape):
    """dict(pxb [B,N,T,r], pyb [B,Ny,T,r] float32 with the builder's -inf applied; ranges [B,T,r] int32; bd [B,4] int32;
    on_x, on_y: the planted paths' own entries; paths; lo [B,T]; tok, blk; B, S, T, r).  Seeded by (kind, shape), cached,
    never to be modified by a caller."""
    key = (kind, shape)
    if key in _CASES:
        return _CASES[key]
    B, S, T, r = shape
    tok, blk = MOVES_OF[shape]
    N, Ny = len(tok), len(blk)
    bd, paths, lo = _geometry(shape)
    rng = np.random.default_rng([KINDS.index(kind), B, S, T, r])
    planes = [_values(kind, rng, B, T, r) for _ in range(max(N, Ny))]        # (token plane, blank plane) pairs
    pxb = np.stack([planes[i][0] for i in range(N)], axis=1)
    pyb = np.stack([planes[j][1] for j in range(Ny)], axis=1)
    on_x, on_y = np.zeros(pxb.shape, bool), np.zeros(pyb.shape, bool)
    for b in range(B):
        sb, tb = int(bd[b, 0]), int(bd[b, 1])
        for s, t, m in paths[b]:
            k = sb + s - lo[b, tb + t]
            (on_x[b, m] if m < N else on_y[b, m - N])[tb + t, k] = True
    if kind == "sharp":
        pxb[on_x] = np.float32(-0.1)
        pyb[on_y] = np.float32(-0.05)
    if kind == "holes":                                     # 10 % of the off-path entries; the planted path survives
        for arr, on in ((pxb, on_x), (pyb, on_y)):
            hole = (rng.random(arr.shape) < 0.1) & ~on
            arr[0][hole[0]] = np.float32(-1.0e20)           # utterance 0: huge finite stand-ins for -inf
            arr[1:][hole[1:]] = NEG
    ranges = lo[:, :, None] + np.arange(r)
    for b in range(B):                                      # the -inf rules of the builder at the band cells
        te = int(bd[b, 3])
        rows = ranges[b]
        tt = np.arange(T)[:, None]
        for i, e in enumerate(tok):
            pxb[b, i][(rows >= S) | (tt >= te) | (tt + e > te)] = NEG
        for j, d in enumerate(blk):
            pyb[b, j][np.broadcast_to(tt + d > te, rows.shape)] = NEG
    case = dict(kind=kind, shape=shape, B=B, S=S, T=T, r=r, tok=tok, blk=blk, pxb=pxb, pyb=pyb, ranges=ranges.astype(np.int32),
                bd=bd.astype(np.int32), on_x=on_x, on_y=on_y, paths=paths, lo=lo)
    _CASES[key] = case
    return case


_REFS = {}


def _reference(kind, shape):
    key = (kind, shape)
    if key not in _REFS:
        c = make_case(kind, shape)
        S, T = c["S"], c["T"]
        px = _scatter(c["pxb"], c["ranges"], S, S, T + 1)
        py = _scatter(c["pyb"], c["ranges"], S, S + 1, T)
        a64, gx, gy = tdt_dp_with_grads(px, py, c["tok"], c["blk"], c["bd"])
        _REFS[key] = (a64, _gather(gx, c["ranges"]), _gather(gy, c["ranges"]), gx.sum(axis=(1, 2, 3)), gy.sum(axis=(1, 2, 3)))
    return _REFS[key]


def reference(kind, shape):
    """(ans64 [B], gx64 [B,N,T,r], gy64 [B,Ny,T,r]): tdt_dp_with_grads on the scattered lattices, the occupancies gathered
    back to the band.  Computed once per (kind, shape), never to be modified by a caller."""
    return _reference(kind, shape)[:3]


def lattice_totals(kind, shape):
    """(sum of px_grad [B], sum of py_grad [B]) over the whole lattices, before the gather."""
    return _reference(kind, shape)[3:]


def shifted(case, cx, c):
    """The band operands with cx + c e_i added to every finite entry of token plane i and c d_j to every finite entry of
    blank plane j (float32, as a caller would): every complete path gains (s_end - s_begin) cx + c (t_end - t_begin)."""
    pxb, pyb = case["pxb"].copy(), case["pyb"].copy()
    for i, e in enumerate(case["tok"]):
        pxb[:, i] = np.where(np.isfinite(pxb[:, i]), pxb[:, i] + np.float32(cx + c * e), pxb[:, i])
    for j, d in enumerate(case["blk"]):
        pyb[:, j] = np.where(np.isfinite(pyb[:, j]), pyb[:, j] + np.float32(c * d), pyb[:, j])
    return pxb, pyb


def path_gain(case, cx, c):
    """What `shifted` adds to every utterance's ans, [B] float64."""
    bd = case["bd"].astype(np.float64)
    return (bd[:, 2] - bd[:, 0]) * cx + c * (bd[:, 3] - bd[:, 1])


def band_rows(case):
    """[B,T,r] lattice row of every band row."""
    return case["ranges"].astype(np.int64)
