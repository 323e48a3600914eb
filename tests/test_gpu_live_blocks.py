"""The builder's backward on the live part of the lattice (include/ftr_live.h): the W kernel's table of live frame intervals
and the fused d am kernel that walks only the row chunks the table reaches.

Away from the paths that carry probability the occupancies g_px, g_py are exact zeros, and W with them; skipping a block of
exact zeros removes additions of exact zeros and nothing else, so d am with the table compares EQUAL under `==` with d am
under FTR_BWD_LIVE=dense (every interval [0, T)).  `==` on floats: +0 and -0 compare equal, which is what is claimed -- a sum
of skipped (-0) terms may come out as +0.  Shapes: B = 2, T = 132 (two 64-frame tiles and a 4-frame one), S = 37 (two 16-row
chunks and a 6-row one), C = 20 (one partial column group) and C = 260 (a 256-column group that owns no blank and a sliver
that does; three groups of 128).  Inputs are N(0,1) times 8: peaked enough that, on the CPU oracle, 4 - 8 of an utterance's
nine 16-row x 64-frame blocks hold a non-zero occupancy (regular and modified, full and ragged boundary).  Every test first
asserts on the GPU's own px_grad / py_grad that every utterance has at least one dead and one live block."""
import numpy as np
import pytest
import torch

from helpers import synthetic

pytestmark = pytest.mark.gpu

B, T, S = 2, 132, 37
INPUT_SCALE = 8.0
SMOOTH = (0.1, 0.2)     # lm_only_scale, am_only_scale
_KNOBS = ("FTR_BWD_LIVE", "FTR_FUSED_BWD_CT", "FTR_BUILDER_BWD", "FTR_BUILDER_GEMM")


@pytest.fixture(autouse=True)
def _knobs(monkeypatch):
    monkeypatch.setenv("FTR_GEMM_TUNE", "off")
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)


def _rl():
    import importlib
    return importlib.import_module("tf_fast_rnnt.rnnt_loss")


def _problem(C, ragged=True, T=T):
    p = synthetic(11 * T + S + C, B, T, S, C, ragged=ragged)      # utterance 0 is full, utterance 1 ends early when ragged
    p["am"] = p["am"] * np.float32(INPUT_SCALE); p["lm"] = p["lm"] * np.float32(INPUT_SCALE)
    return p


def _loss(ft, dev, p, rnnt_type, smooth, am, lm):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    kw = dict(lm=lm, am=am, symbols=t(p["symbols"]), termination_symbol=p["termination_symbol"], boundary=t(p["boundary"]),
              rnnt_type=rnnt_type, reduction="none", calc_gradients=True)
    if smooth is None:
        return ft.rnnt_loss_simple(**kw)
    return ft.rnnt_loss_smoothed(lm_only_scale=smooth[0], am_only_scale=smooth[1], **kw)


def _grads(ft, dev, monkeypatch, p, rnnt_type, smooth, weights, dense, ct=None):
    """d am, d lm of sum_b weights[b] * loss[b] and the occupancies, with the live table (dense = False) or with every
    interval [0, T) (dense = True)."""
    if dense:
        monkeypatch.setenv("FTR_BWD_LIVE", "dense")
    else:
        monkeypatch.delenv("FTR_BWD_LIVE", raising=False)
    if ct is None:
        monkeypatch.delenv("FTR_FUSED_BWD_CT", raising=False)
    else:
        monkeypatch.setenv("FTR_FUSED_BWD_CT", str(ct))
    am = torch.from_numpy(p["am"]).to(dev).requires_grad_(True)
    lm = torch.from_numpy(p["lm"]).to(dev).requires_grad_(True)
    loss, (gx, gy) = _loss(ft, dev, p, rnnt_type, smooth, am, lm)
    (loss * torch.tensor(weights, dtype=torch.float32, device=dev)).sum().backward()
    return am.grad.cpu().numpy(), lm.grad.cpu().numpy(), gx.cpu().numpy(), gy.cpu().numpy()


def _live_cells(gx, gy, boundary, modified):
    """[B, S+1, T] bool: cells with a non-zero (or NaN) occupancy; the column t_end of a regular g_px is masked."""
    x = np.zeros_like(gy)
    x[:, :S, :] = gx[:, :, :gy.shape[2]]
    if not modified:
        for b in range(gy.shape[0]):
            te = int(boundary[b, 3])
            if te < gy.shape[2]:
                x[b, :, te] = 0.0
    return (x != 0) | (gy != 0)


def _assert_dead_and_live_blocks(gx, gy, boundary, modified, tag):
    live = _live_cells(gx, gy, boundary, modified)
    Tn = gy.shape[2]
    ns, nt = (S + 1 + 15) // 16, (Tn + 63) // 64
    pad = np.zeros((gy.shape[0], ns * 16, nt * 64), bool)
    pad[:, :S + 1, :Tn] = live
    blk = pad.reshape(gy.shape[0], ns, 16, nt, 64).any(axis=(2, 4))
    for b in range(gy.shape[0]):
        n = int(blk[b].sum())
        assert 1 <= n <= ns * nt - 1, f"{tag}: utterance {b} has {n} live 16x64 blocks of {ns * nt}: the test would pass vacuously"


CASES = [  # C, rnnt_type, smooth, column tiling
    (20, "regular", None, None), (20, "modified", SMOOTH, None),
    (260, "regular", None, 128), (260, "regular", None, 256), (260, "modified", None, 128), (260, "modified", None, 256),
    (260, "regular", SMOOTH, 128), (260, "regular", SMOOTH, 256), (260, "modified", SMOOTH, 128), (260, "modified", SMOOTH, 256),
]


@pytest.mark.parametrize("C,rnnt_type,smooth,ct", CASES)
def test_skipping_is_exact(ft, dev, monkeypatch, C, rnnt_type, smooth, ct):
    """d am (and d lm, which reads the same W) with the table == with every interval dense: ragged boundary, a reduction with
    per-utterance scales, and upstream scale 0 (every row dead: exact zeros)."""
    p = _problem(C, ragged=True)
    tag = f"C={C} {rnnt_type} {smooth} ct={ct}"
    for weights in ((0.5, 1.5), (0.0, 0.0)):
        a_live, l_live, gx, gy = _grads(ft, dev, monkeypatch, p, rnnt_type, smooth, weights, False, ct)
        a_dense, l_dense, gx2, gy2 = _grads(ft, dev, monkeypatch, p, rnnt_type, smooth, weights, True, ct)
        _assert_dead_and_live_blocks(gx, gy, p["boundary"], rnnt_type == "modified", tag)
        assert np.array_equal(gx, gx2) and np.array_equal(gy, gy2), tag
        assert np.isfinite(a_dense).all() and np.isfinite(l_dense).all(), tag
        assert np.array_equal(a_live, a_dense), f"{tag} weights {weights}: d am differs in {(a_live != a_dense).sum()} elements"   # ==: +0 equals -0
        assert np.array_equal(l_live, l_dense), f"{tag} weights {weights}: d lm differs"
        if weights == (0.0, 0.0):
            assert not a_live.any() and not a_dense.any(), tag
        else:
            assert a_live.any(), tag


@pytest.mark.parametrize("C,ct", [(20, None), (260, 128), (260, 256)])
def test_full_boundary_and_unit_scale(ft, dev, monkeypatch, C, ct):
    p = _problem(C, ragged=False)
    for rnnt_type in ("regular", "modified"):
        a_live, l_live, gx, gy = _grads(ft, dev, monkeypatch, p, rnnt_type, None, (1.0, 1.0), False, ct)
        a_dense, l_dense, _, _ = _grads(ft, dev, monkeypatch, p, rnnt_type, None, (1.0, 1.0), True, ct)
        _assert_dead_and_live_blocks(gx, gy, p["boundary"], rnnt_type == "modified", f"C={C} {rnnt_type}")
        assert np.isfinite(a_dense).all()
        assert np.array_equal(a_live, a_dense) and np.array_equal(l_live, l_dense), (C, ct, rnnt_type)


@pytest.mark.parametrize("C,smooth", [(20, None), (260, None), (260, SMOOTH)])
def test_nan_behaves_as_before(ft, dev, monkeypatch, C, smooth):
    """One NaN in am: d am and d lm have NaN in exactly the same places with the table as without, and equal numbers
    elsewhere.  (The dead / live precondition is asserted on the same inputs without the NaN: the NaN makes its utterance's
    occupancies NaN, hence live, everywhere.)"""
    p = _problem(C, ragged=True)
    _, _, gx, gy = _grads(ft, dev, monkeypatch, p, "regular", smooth, (1.0, 1.0), False)
    _assert_dead_and_live_blocks(gx, gy, p["boundary"], False, f"C={C}")
    for b, t, c in ((1, 40, 3), (0, 70, C - 1)):
        q = dict(p); q["am"] = p["am"].copy(); q["am"][b, t, c] = np.nan
        a_live, l_live, _, _ = _grads(ft, dev, monkeypatch, q, "regular", smooth, (0.5, 1.5), False)
        a_dense, l_dense, _, _ = _grads(ft, dev, monkeypatch, q, "regular", smooth, (0.5, 1.5), True)
        assert np.isnan(a_dense).any(), "the NaN did not reach d am: the case tests nothing"
        assert np.array_equal(np.isnan(a_live), np.isnan(a_dense)), (C, smooth, b)
        assert np.array_equal(np.isnan(l_live), np.isnan(l_dense)), (C, smooth, b)
        assert np.array_equal(a_live, a_dense, equal_nan=True) and np.array_equal(l_live, l_dense, equal_nan=True), (C, smooth, b)


def _bits_nonzero(a):
    return (a.view(np.int32) & 0x7fffffff) != 0


@pytest.mark.parametrize("Tn", [132, 130])       # 130: the W kernel's scalar tail (T % 4 != 0; outside the fused d am kernel's domain)
@pytest.mark.parametrize("modified", [0, 1])
def test_live_table(ft, dev, monkeypatch, modified, Tn):
    """live[b,s] = [first, last + 1) of the frames where x, y or W of the same call is not an exact zero; (T, 0) for a row
    without one; every interval [0, T) under FTR_BWD_LIVE=dense."""
    from tf_fast_rnnt import _lib
    RL = _rl()
    C = 20
    p = _problem(C, ragged=True, T=Tn)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    lm, am, sym, bnd = t(p["lm"]), t(p["am"]), t(p["symbols"]), t(p["boundary"])
    rnnt_type = "modified" if modified else "regular"
    _, (gx, gy) = _loss(ft, dev, p, rnnt_type, None, am, lm)
    _assert_dead_and_live_blocks(gx.cpu().numpy(), gy.cpu().numpy(), p["boundary"], bool(modified), f"T={Tn} {rnnt_type}")
    _, _, saved, _meta = RL._simple_forward(lm, am, sym, p["termination_symbol"], bnd, modified, 0.0)
    prod = saved[2]
    ptr = lambda x: None if x is None else x.data_ptr()
    st = torch.cuda.current_stream(dev).cuda_stream
    mul = 0.5                                    # a power of two: x = g_px * mul is the same float here and in the kernel
    for cs in (None, 0.7):                       # the simple entry, and the smoothed one (same kernel, W times the combined scale)
        out = {}
        for mode in ("table", "dense"):
            if mode == "dense":
                monkeypatch.setenv("FTR_BWD_LIVE", "dense")
            else:
                monkeypatch.delenv("FTR_BWD_LIVE", raising=False)
            W = torch.empty_like(prod); rsx = torch.empty((B, S + 1), device=dev); rsy = torch.empty((B, S + 1), device=dev)
            live = torch.full((B, S + 1, 2), -7, dtype=torch.int32, device=dev)
            if cs is None:
                _lib.call("ftr_simple_logprobs_bwd_w_live_f32", ptr(gx), ptr(gy), None, 0, mul, ptr(prod), ptr(bnd), ptr(W),
                          ptr(rsx), ptr(rsy), ptr(live), B, Tn, S, modified, st)
            else:
                _lib.call("ftr_smoothed_logprobs_bwd_w_live_f32", ptr(gx), ptr(gy), None, 0, mul, ptr(prod), ptr(bnd), cs,
                          ptr(W), ptr(rsx), ptr(rsy), ptr(live), B, Tn, S, modified, st)
            out[mode] = (W.cpu().numpy(), live.cpu().numpy())
        Wn, table = out["table"]
        assert np.array_equal(out["dense"][0], Wn)                      # the knob changes the table, not W
        assert (out["dense"][1] == np.array([0, Tn], np.int32)).all()
        x = np.zeros((B, S + 1, Tn), np.float32)
        x[:, :S, :] = gx.cpu().numpy()[:, :, :Tn] * np.float32(mul)
        if not modified:
            for b in range(B):
                if int(p["boundary"][b, 3]) < Tn:
                    x[b, :, int(p["boundary"][b, 3])] = 0.0
        y = gy.cpu().numpy() * np.float32(mul)
        cell = _bits_nonzero(x) | _bits_nonzero(y) | _bits_nonzero(Wn)
        empty = 0
        for b in range(B):
            for s in range(S + 1):
                idx = np.flatnonzero(cell[b, s])
                want = (Tn, 0) if idx.size == 0 else (int(idx[0]), int(idx[-1]) + 1)
                empty += idx.size == 0
                assert tuple(table[b, s]) == want, (cs, b, s, tuple(table[b, s]), want)
        assert empty >= 1, "no row without a live cell: the empty interval is untested"   # the rows past s_end of utterance 1
        assert (table[:, :, 1] - table[:, :, 0] < Tn).any()
