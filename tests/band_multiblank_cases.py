"""Band-shaped inputs for the band-native multi-blank recursion (the multi-blank domain of csrc/mi_band_tdt.hip) and their
float64 reference.  CPU only: numpy, torch and tests/multiblank_restatement.py.

The multi-blank lattice has one symbol move of duration 0 and D blank moves of durations up to 32.  The band <-> lattice
helpers and the band drawer are those of tests/band_tdt_cases.py (`_band_around`, `_scatter`, `_gather`); the path planter is
this file's own, because that file's table is sized for durations up to 16 (`Tn + 17`) and a blank of duration 32 runs off
it.  A path entry is (s, t, move) relative to (s_begin, t_begin), move 0 being the symbol and move 1 + j blank j.  Band
element (b, t, k) of px_band [B,T,r] and (b, j, t, k) of py_band [B,D,T,r] is lattice cell (ranges[b,t,k], t).

* `recursion_case(shape, durations, with_boundary)`: iid N(0,1) operands with 2 % -inf, a planted path that stays finite,
  the builder's -inf rules, and the restatement's (ans, gx_band, gy_band).  Whether a path exists is decided by the planter
  alone (reachability over the rectangle, the move list and the band width), never by the values.
* STRUCTURED cases, the counterpart of tests/band_tdt_cases.py: `make_case(kind, shape)` with the value kinds of
  band_cases._values on the shapes of CASES, `reference(kind, shape)` once per case.  Utterance 0 has the full rectangle; in
  B = 2 shapes utterance 1 has boundary (2, 5, S - 3, T - 7)."""
import functools

import numpy as np

from band_cases import _values
from band_tdt_cases import KINDS, _band_around, _gather, _scatter          # noqa: F401  (re-exported for the tests)
from multiblank_restatement import multiblank_dp_with_grads

NEG = float("-inf")

# (B, S, T, r) and its blank durations (M = D + 1 moves; 8 lanes for r <= 7, 16 above; ring depth 64 at duration 32)
CASES = [
    ((2, 20, 70, 4), (1, 2, 4, 8)),                         # short base case, M = 5
    ((2, 100, 300, 8), (1, 2, 4, 8, 16, 17, 31, 32)),       # M = 9, 16 lanes, ring of 64 steps wrapped six times
    ((1, 300, 1500, 5), (1, 2, 4, 8)),                      # the shape of the memory test, with parity
    ((1, 120, 2000, 2), (1, 32)),                           # ring of 64 steps, r = 2, the longest walk
]
SHAPES = [shape for shape, _ in CASES]
DURATIONS_OF = dict(CASES)


def shape_id(shape):
    B, S, T, r = shape
    return f"B{B}S{S}T{T}r{r}_D{len(DURATIONS_OF[shape])}max{DURATIONS_OF[shape][-1]}"


# the iid parity cases of recursion_case: (B, S, T, r), and the duration lists -- one blank; the usual set; beyond TDT's 16
# (ring of 32 steps); ring of 64 steps, which wraps once S + T > 64; no 1; D = 8 (M = 9), the second with ring 64
RECURSION_SHAPES = [(2, 0, 9, 1), (2, 5, 1, 4), (3, 12, 40, 4), (2, 33, 70, 5), (1, 6, 1100, 3), (2, 50, 200, 5), (2, 20, 100, 8),
                    (2, 20, 100, 15)]
RECURSION_DURATIONS = [(1,), (1, 2, 4, 8), (1, 17), (1, 32), (2, 3), (1, 2, 3, 4, 5, 6, 7, 8), (1, 2, 4, 8, 16, 17, 31, 32)]
ONE_FRAME = (2, 5, 1, 4)     # rows 0..5 of its single frame do not fit a band of 4 rows: no path whatever the values


def random_path(rng, Sn, Tn, durations, r):
    """A random path (0,0) -> (Sn-1,Tn-1) of the rectangle as [(s, t, move)] that climbs at most r - 1 rows inside one
    frame (the rows it visits at a frame must fit one band of r rows); None when there is none.  The table is wide enough
    for the longest blank (32 frames past the last column)."""
    pad = max(durations) + 1
    reach = np.zeros((Sn + 1, Tn + pad, r + 1), bool)       # reach[s,t,c]: the end is reachable from (s,t) after c climbs at t
    reach[Sn - 1, Tn - 1, :r] = True
    for t in range(Tn - 2, -1, -1):
        for s in range(Sn - 1, -1, -1):
            on = any(reach[s, t + d, 0] for d in durations)
            for c in range(r - 1, -1, -1):
                reach[s, t, c] = on or (c < r - 1 and reach[s + 1, t, c + 1])
    if not reach[0, 0, 0]:
        return None
    s, t, c, path = 0, 0, 0, []
    while (s, t) != (Sn - 1, Tn - 1):
        ok = [0] if (c < r - 1 and reach[s + 1, t, c + 1]) else []
        ok += [1 + j for j, d in enumerate(durations) if reach[s, t + d, 0]]
        m = ok[rng.integers(len(ok))]
        path.append((s, t, m))
        if m == 0:
            s, c = s + 1, c + 1
        else:
            t, c = t + durations[m - 1], 0
    return path


def apply_builder_rules(pxb, pyb, ranges, bd, durations, S):
    """The -inf rules of the builder at the band cells, in place: no symbol out of row S or out of a frame >= t_end, no
    blank that lands past t_end."""
    B, T, r = pxb.shape
    tt = np.arange(T)[:, None]
    for b in range(B):
        te = int(bd[b, 3])
        rows = ranges[b]
        pxb[b][(rows >= S) | (tt >= te)] = NEG
        for j, d in enumerate(durations):
            pyb[b, j][np.broadcast_to(tt + d > te, rows.shape)] = NEG


def restatement(pxb, pyb, ranges, bd, durations, S):
    """(ans [B], gx_band [B,T,r], gy_band [B,D,T,r]) float64: multiblank_dp_with_grads on the band scattered into full-size
    lattices of -inf, the occupancies gathered back to the band."""
    T = pxb.shape[1]
    px = _scatter(pxb[:, None], ranges, S, S, T + 1)[:, 0]
    py = _scatter(pyb, ranges, S, S + 1, T)
    ans, gx, gy = multiblank_dp_with_grads(px, py, durations, bd)
    return ans, _gather(gx[:, None], ranges)[:, 0], _gather(gy, ranges), gx.sum(axis=(1, 2)), gy.sum(axis=(1, 2, 3))


@functools.lru_cache(maxsize=None)
def recursion_case(shape, durations, with_boundary):
    """(pxb, pyb, ranges int32, bd int32 | None, has_path, (ans64, gx64, gy64)); cached, never to be modified by a caller."""
    B, S, T, r = shape
    D = len(durations)
    rng = np.random.default_rng([S, T, r, D, sum(durations), int(with_boundary)])
    bd = np.zeros((B, 4), np.int64)
    bd[:, 2], bd[:, 3] = S, T
    if with_boundary:
        for b in range(B):                       # ragged ends; utterance 0 also begins inside the lattice
            bd[b] = [1 if (b == 0 and S >= 3) else 0, 2 if (b == 0 and T >= 6) else 0, S - (b % 2 if S >= 2 else 0),
                     T - 1 - b % 2 if T >= 3 else T]
    ranges = np.zeros((B, T, r), np.int64)
    pxb = rng.standard_normal((B, T, r)).astype(np.float32)
    pyb = rng.standard_normal((B, D, T, r)).astype(np.float32)
    pxb[rng.random(pxb.shape) < 0.02] = NEG
    pyb[rng.random(pyb.shape) < 0.02] = NEG
    has_path = True
    for b in range(B):
        sb, tb, se, te = (int(v) for v in bd[b])
        path = random_path(rng, se - sb + 1, te - tb + 1, durations, r)
        while path is None and with_boundary and te - 1 > tb + 1:      # a ragged end that the move list can land on
            te -= 1
            path = random_path(rng, se - sb + 1, te - tb + 1, durations, r)
        if path is None:
            te = int(bd[b, 3])
        bd[b, 3] = te
        has_path = has_path and path is not None
        lo = _band_around(rng, path or [], sb, tb, te, S, T, r)
        ranges[b] = lo[:, None] + np.arange(r)
        for s, t, m in path or []:               # the path's own moves stay finite
            k = sb + s - lo[tb + t]
            (pxb[b] if m == 0 else pyb[b, m - 1])[tb + t, k] = rng.standard_normal()
    apply_builder_rules(pxb, pyb, ranges, bd, durations, S)
    bdi = bd.astype(np.int32) if with_boundary else None
    return pxb, pyb, ranges.astype(np.int32), bdi, has_path, restatement(pxb, pyb, ranges, bdi, durations, S)[:3]


# --------------------------------------------------------------------------------------------------- structured cases
@functools.lru_cache(maxsize=None)
def _geometry(shape):
    """(bd [B,4] int64, paths per utterance, lo [B,T]) of a shape: the seven kinds of a shape share them."""
    B, S, T, r = shape
    durations = DURATIONS_OF[shape]
    rng = np.random.default_rng([B, S, T, r, len(durations), durations[-1]])
    bd = np.zeros((B, 4), np.int64)
    bd[:, 2], bd[:, 3] = S, T
    if B > 1:
        bd[1] = (2, 5, S - 3, T - 7)
    paths, lo = [], np.zeros((B, T), np.int64)
    for b in range(B):
        sb, tb, se, te = (int(v) for v in bd[b])
        path = random_path(rng, se - sb + 1, te - tb + 1, durations, r)
        assert path is not None, f"{shape}: the durations {durations} have no path through utterance {b}'s rectangle"
        paths.append(path)
        lo[b] = _band_around(rng, path, sb, tb, te, S, T, r)
    return bd, paths, lo


@functools.lru_cache(maxsize=None)
def make_case(kind, shape):
    """dict(pxb [B,T,r], pyb [B,D,T,r] float32 with the builder's -inf applied; ranges [B,T,r] int32; bd [B,4] int32; on_x,
    on_y: the planted paths' own entries; paths; lo [B,T]; durations; B, S, T, r).  Off-path values have the means and
    deviations of band_cases._values on the symbol plane and on all D blank planes; `sharp` puts -0.1 on the path's symbol
    entries and -0.05 on its blank entries; `holes` knocks out 10 % of the off-path entries, -1e20 in utterance 0 and -inf in
    the others.  Seeded by (kind, shape), cached, never to be modified by a caller."""
    B, S, T, r = shape
    durations = DURATIONS_OF[shape]
    D = len(durations)
    bd, paths, lo = _geometry(shape)
    rng = np.random.default_rng([KINDS.index(kind), B, S, T, r, 32])
    planes = [_values(kind, rng, B, T, r) for _ in range(D)]
    pxb = planes[0][0]
    pyb = np.stack([planes[j][1] for j in range(D)], axis=1)
    on_x, on_y = np.zeros(pxb.shape, bool), np.zeros(pyb.shape, bool)
    for b in range(B):
        sb, tb = int(bd[b, 0]), int(bd[b, 1])
        for s, t, m in paths[b]:
            k = sb + s - lo[b, tb + t]
            (on_x[b] if m == 0 else on_y[b, m - 1])[tb + t, k] = True
    if kind == "sharp":
        pxb[on_x] = np.float32(-0.1)
        pyb[on_y] = np.float32(-0.05)
    if kind == "holes":                                     # 10 % of the off-path entries; the planted path survives
        for arr, on in ((pxb, on_x), (pyb, on_y)):
            hole = (rng.random(arr.shape) < 0.1) & ~on
            arr[0][hole[0]] = np.float32(-1.0e20)           # utterance 0: huge finite stand-ins for -inf
            arr[1:][hole[1:]] = NEG
    ranges = lo[:, :, None] + np.arange(r)
    apply_builder_rules(pxb, pyb, ranges, bd, durations, S)
    return dict(kind=kind, shape=shape, B=B, S=S, T=T, r=r, durations=durations, pxb=pxb, pyb=pyb,
                ranges=ranges.astype(np.int32), bd=bd.astype(np.int32), on_x=on_x, on_y=on_y, paths=paths, lo=lo)


@functools.lru_cache(maxsize=None)
def _reference(kind, shape):
    c = make_case(kind, shape)
    return restatement(c["pxb"], c["pyb"], c["ranges"], c["bd"], c["durations"], c["S"])


def reference(kind, shape):
    """(ans64 [B], gx64 [B,T,r], gy64 [B,D,T,r]); computed once per (kind, shape), never to be modified by a caller."""
    return _reference(kind, shape)[:3]


def lattice_totals(kind, shape):
    """(sum of px_grad [B], sum of py_grad [B]) over the whole lattices, before the gather."""
    return _reference(kind, shape)[3:]
