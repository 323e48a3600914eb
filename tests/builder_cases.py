"""Trained-model-shaped am / lm for the simple and the smoothed px / py builders (get_rnnt_logprobs, get_rnnt_logprobs_smoothed:
csrc/simple_logprobs.hip, csrc/simple_fused.hip, the library GEMMs and the torch glue of _smoothed_forward) and their
FLOAT64 references.  CPU only, seeded, cached; a caller never modifies what it gets.

Geometry of a case.  Every utterance has a boundary (0, 0, s_end, t_end), utterance 0 full size, utterance 1 ragged (for
T % 4 == 0 its t_end is no multiple of 4: the 16-byte sweeps of the backward kernels end inside a quad).  Inside it a
monotone alignment is planted (band_cases.planted_alignment): at most 2 symbols per frame for the regular type, one for the
modified / constrained types (`strict` cases; where S > T the full-size utterance of a strict case keeps t_end = T and
takes s_end = T - 4, because the modified lattice has no path with more symbols than frames -- the builders still compute
all S + 1 rows).  Then

    am[b,t,:] = 2 N(0,1) + margin on the column the path emits at frame t (its first symbol there, blank if it emits none
                or the frame lies past t_end),
    lm[b,s,:] = 2 N(0,1) + margin on target(symbols[b,s]), target(blank) for s = S,

with target(c) = c (the networks AGREE) or (c + 7) mod (C - 1) (they CONFLICT: the normaliser product is about e^-margin).
blank = C - 1; three columns per case are kept free of symbols (the `masked` kind masks them).

Kinds: see KINDS below.  SOUND kinds have a normaliser product that stays a normal float32 on every cell, so the reference's
`W = g / (prod + tiny)` arithmetic has a gradient; `subnormal` and `zero` do not (the float32 restatement returns NaN there),
and only their forward is pinned.

References: tests/torch_restatements.py in float64 on the float32 inputs, `tiny` added in float64 as written there;
gradients by autograd of (px wx).sum() + (py wy).sum() over the finite cells with (a) seeded N(0,1) weights and (b) minus
the float64 occupancies of the float64 px / py, which makes them d loss / d am and d loss / d lm of the sum-reduced loss.
"""
import numpy as np
import torch

import band_cases as BC
import torch_restatements as R

TINY = 1.401298464324817e-45            # the smallest float32 subnormal, rnnt_loss._TINY
F32_MIN_NORMAL = 2.0 ** -126
KINDS = ["agree12", "conflict25", "wide", "offset", "masked", "subnormal", "zero"]
SOUND = ["agree12", "conflict25", "wide", "offset", "masked"]
UNSOUND = ["subnormal", "zero"]
# (B, T, S, C) and the code path each one is there for
SHAPES = [
    (2, 72, 33, 36),       # C % 4 == 0, no multiple of the 32 staged columns; a full 64-frame tile + a ragged one; t_end % 4 != 0
    (2, 130, 20, 37),      # odd C: library GEMM and the scalar row paths only
    (1, 68, 70, 304),      # C > kTTnarrowAbove (300): 16-frame tiles; S + 1 = 71 rows: two symbol tiles at the forced block count 4
    (2, 40, 33, 12),       # small vocabulary, 32-frame tiles
]
TYPES = ["regular", "modified", "constrained"]
SCALES = [(0.1, 0.2), (0.25, 0.0), (0.0, 0.0)]       # (lm_only_scale, am_only_scale) of the smoothed builder
BUILDERS = [None] + SCALES                          # None: the simple builder
BWD_BUILDERS = [None, (0.1, 0.2), (0.25, 0.0)]      # the backward is pinned for these (the second has the 1e-20 stand-in)
WIDE_INTERVAL = (1e-36, 1e-32)                      # smallest float64 product over the valid cells of a `wide` case


def shape_id(shape):
    return "B%dT%dS%dC%d" % shape


def builder_id(builder):
    return "simple" if builder is None else "smoothed_%g_%g" % builder


def low_cut(C):
    """Products from here up keep >= 10 bits when float32 accumulates C subnormal terms: the cells a bound is asserted on."""
    return 2.0 ** 10 * C * TINY


# ------------------------------------------------------------------------------------------- cases
def products64(am, lm):
    """sum_c lm_probs am_probs [B,S+1,T] in float64 on the float32 inputs (torch_restatements._normalizers without the log)."""
    a = am.astype(np.float64); l = lm.astype(np.float64)
    ap = np.exp(a - a.max(axis=2, keepdims=True)); lp = np.exp(l - l.max(axis=2, keepdims=True))
    return np.matmul(lp, ap.transpose(0, 2, 1))


def products32(am, lm):
    """The same op by op in float32 (torch on the CPU keeps subnormals)."""
    _, _, _, ap, lp = R._normalizers(torch.from_numpy(lm), torch.from_numpy(am))
    return torch.matmul(lp, ap.transpose(1, 2)).numpy()


_CASES = {}


def make_case(kind, shape, strict):
    """dict(am [B,T,C], lm [B,S+1,C] float32; symbols [B,S], boundary [B,4] int32; blank; ts: emitting frames per utterance;
    valid [B,S+1,T] bool: the cells inside the boundary; margin; masked_lm / masked_am: columns that are -inf)."""
    key = (kind, shape, bool(strict))
    if key in _CASES:
        return _CASES[key]
    B, T, S, C = shape
    blank = C - 1
    rng = np.random.default_rng([KINDS.index(kind), B, T, S, C, int(strict)])
    free = np.sort(rng.choice(C - 1, 3, replace=False))                    # no symbol uses these columns
    allowed = np.setdiff1d(np.arange(C - 1), free)
    symbols = rng.choice(allowed, (B, S)).astype(np.int32)
    bd = np.zeros((B, 4), np.int32)
    bd[0, 2] = min(S, T - 4) if strict else S
    bd[0, 3] = T
    for b in range(1, B):
        te = int(rng.integers((T + 1) // 2, T))
        if te % 4 == 0:
            te += 1
        hi = min(S, te - 2) if strict else S
        bd[b, 2] = int(rng.integers(hi // 2, hi + 1)); bd[b, 3] = te
    ts = [BC.planted_alignment(rng, int(bd[b, 3]), int(bd[b, 2]), 6, bool(strict)) for b in range(B)]     # r = 6: <= 2 per frame
    conflict = kind in ("conflict25", "wide", "subnormal", "zero")
    sym_ext = np.concatenate((symbols, np.full((B, 1), blank, np.int32)), axis=1).astype(np.int64)
    col_lm = (sym_ext + 7) % (C - 1) if conflict else sym_ext
    col_am = np.full((B, T), blank, np.int64)
    for b in range(B):
        for s in range(len(ts[b]) - 1, -1, -1):                            # the first symbol of a frame wins
            col_am[b, ts[b][s]] = symbols[b, s]
    na = 2.0 * rng.standard_normal((B, T, C)); nl = 2.0 * rng.standard_normal((B, S + 1, C))
    valid = np.zeros((B, S + 1, T), bool)
    for b in range(B):
        valid[b, :bd[b, 2] + 1, :bd[b, 3]] = True

    def build(margin):
        am = na.copy(); lm = nl.copy()
        np.put_along_axis(am, col_am[:, :, None], np.take_along_axis(am, col_am[:, :, None], 2) + margin, 2)
        np.put_along_axis(lm, col_lm[:, :, None], np.take_along_axis(lm, col_lm[:, :, None], 2) + margin, 2)
        return am.astype(np.float32), lm.astype(np.float32)

    masked_lm = masked_am = None
    if kind in ("agree12", "masked"):
        margin = 12.0
    elif kind == "conflict25":
        margin = 25.0
    elif kind == "zero":
        margin = 120.0
    elif kind == "offset":
        margin = 0.0
    elif kind == "wide":        # the first margin (steps of 1/4) at which the smallest product is <= 1e-34, the middle of the interval
        margin = next(m for m in np.arange(55.0, 95.0, 0.25) if products64(*build(m))[valid].min() <= 1e-34)
    elif kind == "subnormal":   # the margin (steps of 1/4) with the largest share of valid cells in [2^10 C tiny, 2^-126)
        def share(m):
            p = products64(*build(m))[valid]
            return float(np.mean((p >= low_cut(C)) & (p < F32_MIN_NORMAL)))
        margin = max(np.arange(80.0, 100.0, 0.25), key=share)
    am, lm = build(margin)
    if kind == "offset":
        am = (am + rng.uniform(-300.0, 300.0, (B, T, 1))).astype(np.float32)
        lm = (lm + rng.uniform(-400.0, 400.0, (B, S + 1, 1))).astype(np.float32)
    if kind == "masked":
        masked_lm = free; masked_am = free[:1]
        lm[:, :, masked_lm] = -np.inf
        am[:, :, masked_am] = -np.inf
        for b in range(B):          # the acoustic model wants what the prediction network forbids
            frames = rng.choice(int(bd[b, 3]), 4, replace=False)
            am[b, frames, free[1 + (frames % 2)]] += np.float32(12.0)
    case = dict(kind=kind, shape=shape, strict=bool(strict), B=B, T=T, S=S, C=C, blank=blank, am=am, lm=lm, symbols=symbols,
                boundary=bd, ts=ts, valid=valid, margin=float(margin), masked_lm=masked_lm, masked_am=masked_am, free=free)
    _CASES[key] = case
    return case


def path_nodes(case, b, rnnt_type):
    """(s, t) of every lattice node the planted path of utterance b visits, t < t_end."""
    ts = case["ts"][b]; te = int(case["boundary"][b, 3])
    e = BC.emitted_before(ts, te)
    if rnnt_type == "regular":
        return [(s, t) for t in range(te) for s in range(int(e[t]), int(e[t + 1]) + 1)]
    return [(int(e[t]), t) for t in range(te)]


# ------------------------------------------------------------------------------------------- float64 (and float32) restatement
def _builder_torch(case, builder, rnnt_type, dtype):
    """(px, py, am, lm) of the restatement in `dtype`; am / lm are leaves that require grad."""
    am = torch.from_numpy(case["am"]).to(dtype).requires_grad_(True)
    lm = torch.from_numpy(case["lm"]).to(dtype).requires_grad_(True)
    sym = torch.from_numpy(case["symbols"]); bd = torch.from_numpy(case["boundary"])
    if builder is None:
        px, py = R.get_rnnt_logprobs_torch(lm, am, sym, case["blank"], rnnt_type, bd)
    else:
        px, py = R.get_rnnt_logprobs_smoothed_torch(lm, am, sym, case["blank"], builder[0], builder[1], bd, rnnt_type)
    return px, py, am, lm


def weighted_grads(px, py, am, lm, wx, wy):
    """d / d (am, lm) of (px wx).sum() + (py wy).sum() over the finite cells of px, as numpy arrays."""
    finite = torch.isfinite(px.detach())
    obj = (torch.where(finite, px, torch.zeros_like(px)) * wx.to(px.dtype)).sum() + (py * wy.to(py.dtype)).sum()
    gam, glm = torch.autograd.grad(obj, (am, lm), retain_graph=True)
    return gam.numpy(), glm.numpy()


def random_weights(case, rnnt_type):
    """Weight set (a): seeded N(0,1) on every cell of px and py, as the builder tests of test_gpu_pipeline.py."""
    B, T, S = case["B"], case["T"], case["S"]
    g = torch.Generator(device="cpu").manual_seed(3)
    wx = torch.randn((B, S, T + 1 if rnnt_type == "regular" else T), generator=g)
    wy = torch.randn((B, S + 1, T), generator=g)
    return wx, wy


def boundary_weights(case, rnnt_type):
    """Weight set (a) with zeros outside every utterance's boundary: an upstream gradient that, like a loss's, leaves the
    padding alone."""
    wx, wy = random_weights(case, rnnt_type)
    for b in range(case["B"]):
        se, te = int(case["boundary"][b, 2]), int(case["boundary"][b, 3])
        wx[b, se:] = 0.0; wx[b, :, te:] = 0.0
        wy[b, se + 1:] = 0.0; wy[b, :, te:] = 0.0
    return wx, wy


_REFS = {}


def reference(oracle, kind, shape, rnnt_type, builder):
    """The float64 reference of one (case, type, builder), computed once:
    px, py [numpy float64]; prod64, nrm64 [B,S+1,T]: the normaliser product and the simple normaliser; occ = (gx64, gy64): the
    float64 occupancies of the float64 px / py; and, on the sound kinds, grads = {"a" | "b": (d am, d lm)} with
    weights = {"a" | "b": (wx, wy)} as float32 tensors (what a GPU test multiplies its own px / py with)."""
    key = (kind, shape, rnnt_type, builder)
    if key in _REFS:
        return _REFS[key]
    case = make_case(kind, shape, rnnt_type != "regular")
    px, py, am, lm = _builder_torch(case, builder, rnnt_type, torch.float64)
    px64 = px.detach().numpy(); py64 = py.detach().numpy()
    prod64 = products64(case["am"], case["lm"])
    a = case["am"].astype(np.float64); l = case["lm"].astype(np.float64)
    nrm64 = np.log(prod64 + TINY) + l.max(axis=2)[:, :, None] + a.max(axis=2)[:, None, :]
    gx64 = gy64 = None
    ans64 = oracle.mutual_information_recursion(px64, py64, case["boundary"], False, np.float64)
    ref = dict(case=case, px=px64, py=py64, prod64=prod64, nrm64=nrm64, ans64=ans64)
    if kind in SOUND:
        _, (gx64, gy64) = oracle.mutual_information_recursion(px64, py64, case["boundary"], True, np.float64)
        wa = random_weights(case, rnnt_type)
        wb = (torch.from_numpy(-np.where(np.isfinite(px64), gx64, 0.0)), torch.from_numpy(-gy64))
        ref["occ"] = (gx64, gy64)
        ref["weights"] = {"a": wa, "b": tuple(w.float() for w in wb)}
        # the float32 weights are what both sides use: the reference differentiates the SAME objective the GPU test does
        ref["grads"] = {k: weighted_grads(px, py, am, lm, *ref["weights"][k]) for k in ("a", "b")}
    _REFS[key] = ref
    return ref


def float32_grads(case, builder, rnnt_type, weights):
    """The float32 op-by-op restatement's gradients for one weight set (the float32 floor of test_builder_cases.py)."""
    px, py, am, lm = _builder_torch(case, builder, rnnt_type, torch.float32)
    return weighted_grads(px, py, am, lm, *weights)


def loss64(oracle, ref, rnnt_type, delay_penalty):
    """The float64 loss per utterance: the float64 recursion on the float64 px / py plus the penalty (rnnt_loss.py:305-321)."""
    case = ref["case"]
    px = ref["px"]
    if delay_penalty > 0.0:
        B, S, T0 = px.shape
        offset = (case["boundary"][:, 3].astype(np.float64) - 1) / 2
        px = px + (offset.reshape(B, 1, 1) - np.arange(T0, dtype=np.float64).reshape(1, 1, T0)) * delay_penalty
    return -oracle.mutual_information_recursion(px, ref["py"], case["boundary"], False, np.float64)


# ------------------------------------------------------------------------------------------- the forward bound
K_ROUND = 4.0
# |v - v64| <= 2e-5 + 1e-5 |v64| + K_ROUND 2^-24 (|a| + |l| + |lm_max| + |am_max| + |nrm64|): the project's px / py tolerance
# (test_native_simple_builder_forward_backward) plus the float32 rounding of sums of large offsets; a, l: the gathered am /
# lm entries; the same formula for px and py of every type.  test_builder_cases.py holds the float32 oracle to HALF of it.
# Measured worst ratio of the oracle's error to the bound with K_ROUND = 4, over all cases, builders and types: 0.27
# (`offset`, px of the constrained type; 0.18 `offset` otherwise, 0.13 `wide`, 0.11 the other kinds).


def forward_bounds(ref, rnnt_type, subnormal_term):
    """(bx [B,S,T1], by [B,S+1,T], low [B,S+1,T], lowx [B,S,T1] bool): the elementwise bound for px and py of this reference
    and the cells of py / px whose product is below low_cut(C) (only with `subnormal_term`: then the bound also gets
    2 C tiny / prod64, the rounding of C subnormal terms relative to the product, and means nothing on the `low` cells)."""
    case = ref["case"]
    B, T, S, C, blank = case["B"], case["T"], case["S"], case["C"], case["blank"]
    am = case["am"].astype(np.float64); lm = case["lm"].astype(np.float64)
    sym = case["symbols"].astype(np.int64)
    amx = np.abs(am.max(axis=2))[:, None, :]; lmx = np.abs(lm.max(axis=2))[:, :, None]
    common = lmx + amx + np.abs(ref["nrm64"])                                                         # [B,S+1,T]
    a_y = np.abs(am[:, :, blank])[:, None, :]; l_y = np.abs(lm[:, :, blank])[:, :, None]
    a_x = np.abs(np.take_along_axis(am.transpose(0, 2, 1), sym[:, :, None], axis=1)) if S else np.zeros((B, 0, T))   # [B,S,T]
    l_x = np.abs(np.take_along_axis(lm[:, :S, :], sym[:, :, None], axis=2))                           # [B,S,1]
    u = K_ROUND * 2.0 ** -24
    extra = np.zeros_like(common); low = np.zeros(common.shape, bool)
    if subnormal_term:
        low = ref["prod64"] < low_cut(C)
        extra = np.where(low, 0.0, 2.0 * C * TINY / np.maximum(ref["prod64"], low_cut(C)))
    py64 = ref["py"]; px64 = ref["px"]
    by = 2e-5 + 1e-5 * np.abs(py64) + u * (a_y + l_y + common) + extra
    # px, every type, the same formula on |px64| (constrained: px64 = px' + py[1:] is one value with one bound; the float32
    # oracle's constrained px reaches 0.27 of it).  Column T of the regular type is -inf and has no bound.
    bx = np.full(px64.shape, np.inf)
    fin = np.isfinite(px64[:, :, :T])
    bx[:, :, :T] = 2e-5 + 1e-5 * np.abs(np.where(fin, px64[:, :, :T], 0.0)) + u * (a_x + l_x + common[:, :S, :]) + extra[:, :S, :]
    lowx = np.zeros(px64.shape, bool); lowx[:, :, :T] = low[:, :S, :]
    if rnnt_type == "constrained":       # a cell is below the cut if either of its two normalisers is
        lowx[:, :, :T] |= low[:, 1:, :]
    return bx, by, low, lowx


def bound_ratio(got, want, bound, skip=None):
    """max |got - want| / bound over the finite cells of `want` that `skip` does not cover (0.0 if there are none)."""
    sel = np.isfinite(want) if skip is None else np.isfinite(want) & ~skip
    if not sel.any():
        return 0.0
    return float((np.abs(got.astype(np.float64)[sel] - want[sel]) / bound[sel]).max())


def norm_err(got, ref):
    """normwise max|d| / max|ref| of one utterance's array."""
    return float(np.abs(got.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))
