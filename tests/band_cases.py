"""Band-shaped inputs for the band recursion kernels (csrc/mi_band.hip, csrc/mi_band_seg.hip) and their float64 reference.

Two things live here.

* The band <-> lattice maps the edge-case test of test_gpu_mi.py has always used (`band_to_lattice`, `lattice_to_band`):
  band cell (t, k) is lattice cell (s, t) with s = s0[t] + k.

* STRUCTURED cases: a planted alignment, monotone contiguous ranges that follow it, and value kinds that are not iid around
  one mean -- what a trained model, a badly scaled one or a masked one hands the kernels (`make_case`), with the float64
  oracle on the expanded lattice collapsed back to the band as the reference (`reference`, computed once per case).

Geometry of a case.  Every utterance gets an alignment over the whole lattice, (0,0) -> (S,T): one emitting frame per symbol
around the diagonal with a jitter of +-3 frames, non-decreasing for the regular type and strictly increasing for the modified
one.  The ranges are s0[t] = clip(e(t) - r // 2, 0, max(S + 1 - r, 0)) with e(t) = symbols emitted before frame t.  Inside
frame t the regular path occupies rows e(t) .. e(t+1), which must all lie in [s0[t], s0[t] + r - 1]: the alignment therefore
emits at most r - 1 - r // 2 symbols per frame (and the band start then steps by at most r - 1).  In B = 2 cases utterance
1 gets begin / end offsets: frames [t_begin, t_end) cut out of the middle, and (s_begin, s_end) the rows where the planted
path crosses those columns -- offsets inside the band that keep the planted path a complete path of the rectangle.
"""
import numpy as np

KINDS = ["sharp", "two_regime", "blank_heavy", "tilted", "deep", "positive", "holes"]

# (B, T, S, r, modified) and the code path each one is there for
SHAPES = [
    (2, 70, 20, 4, False),       # one renormalisation + a scalar tail per half-walk; segments K = 2
    (2, 300, 100, 8, False),     # 16-lane chains
    (2, 300, 100, 7, True),      # 8 lanes with the r+1-th cell of the modified end
    (1, 700, 150, 5, False),     # ~13 renormalisations
    (1, 900, 250, 12, False),    # S + T >= 1100: segments by default; the chain is the 16-lane streaming kernel
    (1, 2200, 500, 5, False),    # 8-lane streaming; K = 32, L > 64
    (1, 1500, 700, 10, True),    # modified type on the long route
]
SEG_FROM = 1100                  # S + T from which the library takes the segmented route, and below which the LDS chain fits


def shape_id(shape):
    B, T, S, r, mod = shape
    return f"{'short' if S + T < SEG_FROM else 'long'}_B{B}T{T}S{S}r{r}{'mod' if mod else 'reg'}"


# ------------------------------------------------------------------------------------------- band <-> lattice
def band_to_lattice(pxb, pyb, s0, bd, S, modified):
    """Expand band arrays [B,T,r] on band starts s0[B,T] to the lattices (px [B,S,T1], py [B,S+1,T]) they stand for, -inf
    outside the band.  pxb / pyb are modified IN PLACE where the band builder writes -inf: s >= S (px), s > S (py) and, for
    the regular type, column t_end."""
    B, T, r = pxb.shape
    T1 = T if modified else T + 1
    px = np.full((B, S, T1), -np.inf, np.float32); py = np.full((B, S + 1, T), -np.inf, np.float32)
    for b in range(B):
        for t in range(T):
            for k in range(r):
                s = s0[b, t] + k
                if s < S: px[b, s, t] = pxb[b, t, k]
                if s <= S: py[b, s, t] = pyb[b, t, k]
                if s >= S: pxb[b, t, k] = -np.inf                     # what the band builder writes there
                if s > S: pyb[b, t, k] = -np.inf
    if not modified:                                                   # fix_for_boundary (rnnt_loss.py:28-61): no symbol in column t_end
        for b in range(B):
            te = int(bd[b, 3])
            if te < T: px[b, :, te] = -np.inf; pxb[b, te, :] = -np.inf
    return px, py


def lattice_to_band(lgx, lgy, s0, r):
    """Collapse lattice-shaped arrays (lgx [B,S,T1], lgy [B,S+1,T]) to the band: [B,T,r], zero where the band has no cell."""
    B, S, T1 = lgx.shape
    T = lgy.shape[2]
    egx = np.zeros((B, T, r), lgx.dtype); egy = np.zeros((B, T, r), lgy.dtype)
    for b in range(B):
        for t in range(T):
            for k in range(r):
                s = s0[b, t] + k
                if s < S and t < T1: egx[b, t, k] = lgx[b, s, t]
                if s <= S: egy[b, t, k] = lgy[b, s, t]
    return egx, egy


# ------------------------------------------------------------------------------------------- structured cases
def planted_alignment(rng, T, S, r, modified):
    """Emitting frame of each of the S symbols on the T frames: around the diagonal, jitter +-3, sorted, at most
    m = r - 1 - r // 2 symbols per frame (regular; see the module docstring) / one per frame (modified)."""
    m = 1 if modified else max(r - 1 - r // 2, 1)
    assert S <= m * T
    ts = np.round((np.arange(S) + 0.5) * T / max(S, 1)).astype(np.int64) + rng.integers(-3, 4, S)
    ts = np.sort(np.clip(ts, 0, T - 1))
    for i in range(m, S):                                  # at most m per frame, pushing later symbols on ...
        ts[i] = max(ts[i], ts[i - m] + 1)
    for i in range(S - 1, -1, -1):                         # ... and back inside the T frames
        ts[i] = min(ts[i], T - 1 - (S - 1 - i) // m)
    return ts


def emitted_before(ts, T):
    """e[t], t = 0 .. T: symbols whose emitting frame is < t -- the row on which the planted path enters column t."""
    return np.searchsorted(ts, np.arange(T + 1), side="left").astype(np.int64)


def path_band_cells(ts, s0, T, modified):
    """The planted path's transitions as band coordinates: (t, k) of its px entries and (t, k) of its py entries."""
    e = emitted_before(ts, T)
    xs = [(int(t), int(s - s0[t])) for s, t in enumerate(ts)]
    if modified:
        emits = np.zeros(T, bool); emits[ts] = True
        ys = [(t, int(e[t] - s0[t])) for t in range(T) if not emits[t]]
    else:
        ys = [(t, int(e[t + 1] - s0[t])) for t in range(T)]          # the blank of frame t is taken after its symbols
    return xs, ys


def _values(kind, rng, B, T, r):
    n = lambda mean, std: (mean + std * rng.standard_normal((B, T, r))).astype(np.float32)
    if kind == "sharp":
        return n(-10.0, 1.0), n(-3.0, 1.0)
    if kind == "two_regime":                                # one mean fits neither half
        px, py = n(-1.0, 1.0), n(-1.0, 1.0)
        px[:, T // 2:] -= np.float32(14.0); py[:, T // 2:] -= np.float32(14.0)
        return px, py
    if kind == "blank_heavy":
        return n(-8.0, 0.5), n(-0.1, 0.05)
    if kind == "tilted":
        return n(-2.0, 1.0), n(-9.0, 1.0)
    if kind == "deep":
        return n(-60.0, 5.0), n(-60.0, 5.0)
    if kind == "positive":                                  # the op takes any reals
        return n(4.0, 1.0), n(2.0, 1.0)
    if kind == "holes":
        return n(-1.0, 1.0), n(-1.0, 1.0)
    raise ValueError(kind)


_CASES = {}


def make_case(kind, shape):
    """dict(pxb, pyb [B,T,r] float32 with the builder's -inf applied; ranges [B,T,r] int32; s0 [B,T]; bd [B,4] int32;
    px, py: the lattices they expand to; ts: per-utterance emitting frames; B, T, S, r, modified).  Seeded by (kind, shape),
    cached, never to be modified by a caller."""
    key = (kind, shape)
    if key in _CASES:
        return _CASES[key]
    B, T, S, r, modified = shape
    rng = np.random.default_rng([KINDS.index(kind), B, T, S, r, int(modified)])
    ts = [planted_alignment(rng, T, S, r, modified) for _ in range(B)]
    s0 = np.zeros((B, T), np.int64)
    for b in range(B):
        e = emitted_before(ts[b], T)
        s0[b] = np.maximum.accumulate(np.clip(e[:T] - r // 2, 0, max(S + 1 - r, 0)))
    ranges = (s0[:, :, None] + np.arange(r)[None, None, :]).astype(np.int32)
    bd = np.zeros((B, 4), np.int32); bd[:, 2] = S; bd[:, 3] = T
    if B > 1:                                               # utterance 1: offsets inside the band, on the planted path
        e = emitted_before(ts[1], T)
        tb = int(rng.integers(0, max(T // 3, 1))); te = int(rng.integers(max(tb + 1, (2 * T) // 3), T + 1))
        bd[1] = (e[tb], tb, e[te], te)
    pxb, pyb = _values(kind, rng, B, T, r)
    on_x = np.zeros((B, T, r), bool); on_y = np.zeros((B, T, r), bool)
    for b in range(B):
        xs, ys = path_band_cells(ts[b], s0[b], T, modified)
        for t, k in xs: on_x[b, t, k] = True
        for t, k in ys: on_y[b, t, k] = True
    if kind == "sharp":
        pxb[on_x] = np.float32(-0.1); pyb[on_y] = np.float32(-0.05)
    if kind == "holes":                                     # 10 % of the off-path entries; the planted path survives
        for arr, on in ((pxb, on_x), (pyb, on_y)):
            hole = (rng.random((B, T, r)) < 0.1) & ~on
            arr[0][hole[0]] = np.float32(-1.0e20)           # utterance 0: huge finite stand-ins for -inf
            arr[1:][hole[1:]] = -np.inf
    px, py = band_to_lattice(pxb, pyb, s0, bd, S, modified)
    case = dict(kind=kind, shape=shape, B=B, T=T, S=S, r=r, modified=modified, pxb=pxb, pyb=pyb, ranges=ranges, s0=s0, bd=bd,
                px=px, py=py, ts=ts, on_x=on_x, on_y=on_y)
    _CASES[key] = case
    return case


_REFS = {}


def reference(oracle, kind, shape):
    """(ans64 [B], gx64, gy64 [B,T,r]): the float64 oracle on the expanded lattice, occupancies collapsed to the band.
    Computed once per (kind, shape)."""
    key = (kind, shape)
    if key not in _REFS:
        c = make_case(kind, shape)
        a64, (gx64, gy64) = oracle.mutual_information_recursion(c["px"], c["py"], c["bd"], True, np.float64)
        egx, egy = lattice_to_band(gx64, gy64, c["s0"], c["r"])
        _REFS[key] = (a64, egx, egy)
    return _REFS[key]


def shifted(case, cx, cy):
    """The band arrays with cx added to every finite px entry and cy to every finite py entry (float32, as a caller would)."""
    pxb = np.where(np.isfinite(case["pxb"]), case["pxb"] + np.float32(cx), case["pxb"]).astype(np.float32)
    pyb = np.where(np.isfinite(case["pyb"]), case["pyb"] + np.float32(cy), case["pyb"]).astype(np.float32)
    return pxb, pyb


def step_counts(case):
    """(n_x, n_y) per utterance: px and py steps of a complete path (test_operand_shift_is_invisible)."""
    bd = case["bd"]
    nx = (bd[:, 2] - bd[:, 0]).astype(np.float64)
    ny = (bd[:, 3] - bd[:, 1]).astype(np.float64) - (nx if case["modified"] else 0.0)
    return nx, ny
