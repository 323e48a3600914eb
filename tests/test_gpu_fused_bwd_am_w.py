"""The fused d am kernel with W as an operand (ftr_*_logprobs_fused_bwd_am_w_f32, csrc/simple_fused.hip) and its column tilings.

d am of the simple and of the smoothed builder for FIXED upstream gradients g_px, g_py (random, zero outside every
utterance's boundary as occupancies are, and NON-zero in the column t_end of a regular lattice, which the backward has to
mask), through four routes: the W-operand entry (what `_simple_backward` / `_smoothed_backward` call on the fused route),
the product-operand entry it derives from, the library route (FTR_BUILDER_BWD=library: library GEMM + epilogue kernel) and
the float64 torch restatement of the builder (tests/torch_restatements.py) under autograd.  Per utterance, normwise
max|d - ref| / max|ref| <= 1e-4 (TOL_F64, the project's bound) between the W-operand entry and each of the other three;
exactly 0 in every frame from t_end on; two launches bit-identical.  The shapes are the smallest at which a mechanism can go
wrong: one partial column group, a group plus a sliver, a partial last group at C = 500 under the 128-column tiling, four
full groups; frame counts that are multiples of 4 but of no frame tile; S = 1.  The library GEMMs keep rocBLAS' own kernel
(FTR_GEMM_TUNE=off): nothing here times anything."""
import itertools

import numpy as np
import pytest
import torch

import torch_restatements as R
from helpers import synthetic

pytestmark = pytest.mark.gpu

TOL_F64 = 1e-4          # the project's bound: gradients within 1e-4 normwise
_KNOBS = ("FTR_FUSED_BWD_CT", "FTR_BUILDER_BWD", "FTR_BUILDER_GEMM")
BUILDERS = (None, (0.1, 0.2), (0.25, 0.0))   # simple, smoothed (lm_only_scale, am_only_scale)


@pytest.fixture(autouse=True)
def _knobs(monkeypatch):
    monkeypatch.setenv("FTR_GEMM_TUNE", "off")
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)


def _rl():
    """The module tf_fast_rnnt.rnnt_loss (the package attribute of that name is the function it exports)."""
    import importlib
    return importlib.import_module("tf_fast_rnnt.rnnt_loss")


def _upstream(rng, p, modified):
    """g_px [B,S,T1], g_py [B,S+1,T]: positive inside the boundary, 0 outside; the masked column t_end of a regular lattice
    carries values the kernels must not use."""
    B, T, S = p["B"], p["T"], p["S"]
    T1 = T if modified else T + 1
    gpx = np.zeros((B, S, T1), np.float32); gpy = np.zeros((B, S + 1, T), np.float32)
    for b in range(B):
        se, te = int(p["boundary"][b, 2]), int(p["boundary"][b, 3])
        gpx[b, :se, :te] = rng.random((se, te), dtype=np.float32) + 0.05
        gpy[b, :se + 1, :te] = rng.random((se + 1, te), dtype=np.float32) + 0.05
        if not modified:
            gpx[b, :se, te] = 3.0
    return gpx, gpy


def _ref64(p, rnnt_type, smooth, gpx, gpy, factor):
    """d am of sum_b factor[b] * (sum g_px px + sum g_py py) by autograd over the float64 restatement of the builder."""
    lm = torch.tensor(p["lm"], dtype=torch.float64)
    am = torch.tensor(p["am"], dtype=torch.float64, requires_grad=True)
    sym = torch.tensor(p["symbols"]); bnd = torch.tensor(p["boundary"])
    blank = p["termination_symbol"]
    if smooth is None:
        px, py = R.get_rnnt_logprobs_torch(lm, am, sym, blank, rnnt_type, bnd)
    else:
        px, py = R.get_rnnt_logprobs_smoothed_torch(lm, am, sym, blank, smooth[0], smooth[1], boundary=bnd, rnnt_type=rnnt_type)
    px = torch.where(torch.isfinite(px), px, torch.zeros_like(px))
    per_utt = (px * torch.tensor(gpx, dtype=torch.float64)).sum((1, 2)) + (py * torch.tensor(gpy, dtype=torch.float64)).sum((1, 2))
    (per_utt * torch.tensor(factor, dtype=torch.float64)).sum().backward()
    return am.grad.numpy()


class _Native:
    """One forward of the native builder; d am through each route for the same upstream gradients."""

    def __init__(self, dev, p, modified, smooth, gpx, gpy, scale, stride, mul):
        RL = _rl()
        self.RL, self.dev, self.smooth, self.modified = RL, dev, smooth, modified
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        lm, am, sym, bnd = t(p["lm"]), t(p["am"]), t(p["symbols"]), t(p["boundary"])
        blank = p["termination_symbol"]
        if smooth is None:
            _, _, self.saved, self.meta = RL._simple_forward(lm, am, sym, blank, bnd, modified, 0.0)
        else:
            _, _, self.saved, self.meta = RL._smoothed_forward(lm, am, sym, blank, bnd, modified, smooth[0], smooth[1], None, 0.0)
        self.gpx, self.gpy = t(gpx), t(gpy)
        self.scale = None if scale is None else t(scale)
        self.stride, self.mul = stride, mul

    def route(self, monkeypatch, route, ct=None):
        """d am [B,T,C] as numpy through _simple_backward / _smoothed_backward on FTR_BUILDER_BWD=route."""
        monkeypatch.setenv("FTR_BUILDER_BWD", route)
        if ct is None:
            monkeypatch.delenv("FTR_FUSED_BWD_CT", raising=False)
        else:
            monkeypatch.setenv("FTR_FUSED_BWD_CT", str(ct))
        back = self.RL._simple_backward if self.smooth is None else self.RL._smoothed_backward
        _, d_am = back(self.saved, self.meta, self.gpx, self.gpy, self.scale, self.stride, self.mul)
        return d_am.cpu().numpy()

    def product_entry(self):
        """The entry that forms W on the fly from g_px, g_py and the product."""
        from tf_fast_rnnt import _lib
        p = lambda x: None if x is None else x.data_ptr()
        st = torch.cuda.current_stream(self.dev).cuda_stream
        if self.smooth is None:
            am_probs, lm_probs, prod, sym, bnd = self.saved
            blank, modified = self.meta
            B, T, C = am_probs.shape; S = lm_probs.shape[1] - 1
            d_am = torch.empty_like(am_probs)
            _lib.call("ftr_simple_logprobs_fused_bwd_am_f32", p(self.gpx), p(self.gpy), p(self.scale), self.stride, self.mul,
                      p(prod), p(lm_probs), p(am_probs), p(sym), p(bnd), blank, p(d_am), B, T, S, C, modified, st)
        else:
            am_probs, lm_probs, prod, sym, bnd, inv, u, am_dot = self.saved
            blank, modified, cs, ls, a_s, count, group = self.meta
            B, T, C = am_probs.shape; S = lm_probs.shape[1] - 1
            d_am = torch.empty_like(am_probs); Rv = torch.empty((B, T), dtype=torch.float32, device=self.dev)
            _lib.call("ftr_smoothed_logprobs_fused_bwd_am_f32", p(self.gpx), p(self.gpy), p(self.scale), self.stride, self.mul,
                      p(prod), p(lm_probs), p(am_probs), p(sym), p(bnd), blank, cs, cs + a_s, p(u), p(am_dot), a_s, p(Rv),
                      p(d_am), B, T, S, C, modified, st)
        return d_am.cpu().numpy()


def _per_utt(got, ref):
    return [float(np.abs(got[b].astype(np.float64) - ref[b]).max() / max(np.abs(ref[b]).max(), 1e-30)) for b in range(ref.shape[0])]


def _check_shape(ft, dev, monkeypatch, p, ct, tag, builders=BUILDERS, types=("regular", "modified")):
    from tf_fast_rnnt import _lib
    B, T, S, C = p["B"], p["T"], p["S"], p["C"]
    assert _lib.lib().ftr_simple_logprobs_fused_bwd_supported(T, C), tag
    failures = []
    for k, (rnnt_type, smooth) in enumerate(itertools.product(types, builders)):
        modified = rnnt_type == "modified"
        rng = np.random.default_rng(1000 * T + 10 * S + k)
        gpx, gpy = _upstream(rng, p, modified)
        if k % 2 == 0:      # per-utterance scale with stride 1 (reduction "none") ...
            scale, stride, mul = np.linspace(0.5, 1.5, B).astype(np.float32), 1, -1.0
            factor = scale.astype(np.float64) * mul
        else:               # ... and a scalar factor alone (reduction "mean")
            scale, stride, mul = None, 0, -1.0 / B
            factor = np.full((B,), mul, np.float64)
        nat = _Native(dev, p, int(modified), smooth, gpx, gpy, scale, stride, mul)
        w1 = nat.route(monkeypatch, "fused", ct)
        w2 = nat.route(monkeypatch, "fused", ct)
        lib = nat.route(monkeypatch, "library")
        old = nat.product_entry()
        ref = _ref64(p, rnnt_type, smooth, gpx, gpy, factor)
        label = f"{tag} {rnnt_type} {'simple' if smooth is None else smooth}"
        assert np.isfinite(w1).all(), label
        assert np.array_equal(w1.view(np.int32), w2.view(np.int32)), f"{label}: two launches differ"
        for b in range(B):
            te = int(p["boundary"][b, 3])
            assert not w1[b, te:].any(), f"{label}: d am of utterance {b} is not 0 from t_end = {te} on"
        for name, other in (("library route", lib), ("product-operand entry", old), ("float64", ref)):
            e = _per_utt(w1, other.astype(np.float64))
            if not max(e) <= TOL_F64:
                failures.append((label, name, e))
    assert not failures, failures


def _problem(B, T, S, C, symbols=None):
    p = synthetic(7 * T + S + C, B, T, S, C, ragged=True)      # utterance 0 is full, the others end early
    if symbols is not None:
        p["symbols"] = symbols(np.random.default_rng(S + C), (B, S)).astype(np.int32)
    return p


# C = 36: one partial group; 260: a full 256-column group plus a sliver; 500 under its own (128-column) tiling: the last of
# four groups partial; 1024: four full groups.
@pytest.mark.parametrize("C,ct", [(36, None), (260, None), (500, 128), (1024, None)])
def test_column_groups(ft, dev, monkeypatch, C, ct):
    for T, S in itertools.product((68, 72, 100, 132), (1, 33, 70)):
        _check_shape(ft, dev, monkeypatch, _problem(2, T, S, C), ct, f"C={C} T={T} S={S}")


# Every tiling the launcher can choose, forced, on shapes with a partial last frame tile (100 = 64 + 36, 132 = 2 * 64 + 4)
# and a tile list that is no multiple of the device's workgroup slots (any list this short).
@pytest.mark.parametrize("ct", [128, 256])
@pytest.mark.parametrize("cfg", [(2, 100, 33, 500), (3, 132, 70, 260)])
def test_every_tiling_forced(ft, dev, monkeypatch, ct, cfg):
    from tf_fast_rnnt import _lib
    B, T, S, C = cfg
    assert _lib.lib().ftr_simple_logprobs_fused_bwd_am_w_columns(B, T, C) in (128, 256)
    monkeypatch.setenv("FTR_FUSED_BWD_CT", str(ct))
    assert _lib.lib().ftr_simple_logprobs_fused_bwd_am_w_columns(B, T, C) == ct
    _check_shape(ft, dev, monkeypatch, _problem(B, T, S, C), ct, f"ct={ct} {cfg}")


# The scatter pass walks, per workgroup, the list of the rows whose symbol lies in its columns, in stages of CT / 2 rows; the
# list is built 256 rows at a time.  C = 520 is five 128-column groups or three 256-column ones.
_PLACEMENTS = {
    "one_group": lambda rng, shape: rng.integers(130, 250, shape),          # inside [128, 256): one group holds every row,
    "every_symbol_equal": lambda rng, shape: np.full(shape, 7),             # every other group an empty list
    "spread": lambda rng, shape: rng.integers(0, 519, shape),
}


@pytest.mark.parametrize("ct", [128, 256])
@pytest.mark.parametrize("placement", sorted(_PLACEMENTS))
def test_symbol_placement(ft, dev, monkeypatch, placement, ct):
    # S = 330: a list built in two 256-row batches and staged in three (256 columns) or six (128) stages where one group
    # holds every row; S = 33: a single partial stage
    for S in (33, 330):
        p = _problem(2, 68, S, 520, _PLACEMENTS[placement])
        _check_shape(ft, dev, monkeypatch, p, ct, f"{placement} ct={ct} S={S}", builders=(None, (0.1, 0.2)))


def test_auto_route_is_what_the_docstring_says(ft, monkeypatch):
    """`auto` (the default) against the table in _use_fused_builder_bwd's docstring; no device, no timing."""
    RL = _rl()
    monkeypatch.delenv("FTR_BUILDER_BWD", raising=False)
    for (B, T, S, C), fused in RL._FUSED_BWD_MEASURED.items():
        assert RL._use_fused_builder_bwd(T, C, B) is fused, (B, T, S, C)
    assert not RL._use_fused_builder_bwd(1001, 500, 32)       # T % 4 != 0: outside the kernel's domain
    assert not RL._use_fused_builder_bwd(1000, 498, 32)       # C % 4 != 0
    monkeypatch.setenv("FTR_BUILDER_BWD", "library")
    assert not RL._use_fused_builder_bwd(2000, 1024, 32)
    monkeypatch.setenv("FTR_BUILDER_BWD", "fused")
    assert RL._use_fused_builder_bwd(1000, 256, 8) and not RL._use_fused_builder_bwd(1001, 256, 8)


def test_fused_route_allocates_no_btc_scratch(ft, dev, monkeypatch):
    """The library route's `damp` [B,T,C] does not exist on the fused route: peak allocation of the backward."""
    B, T, S, C = 2, 132, 33, 1024
    p = _problem(B, T, S, C)
    gpx, gpy = _upstream(np.random.default_rng(5), p, False)
    nat = _Native(dev, p, 0, None, gpx, gpy, None, 0, 1.0)
    peak = {}
    for route in ("library", "fused", "library", "fused"):
        torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        nat.route(monkeypatch, route)
        torch.cuda.synchronize()
        peak[route] = torch.cuda.max_memory_allocated(dev) - base
    assert peak["library"] - peak["fused"] >= 4 * B * T * C, peak
