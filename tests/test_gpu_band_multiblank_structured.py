"""The band-native multi-blank route (the multi-blank domain of csrc/mi_band_tdt.hip, the band-shaped mb_* kernels of
csrc/pruned_logprobs.hip, the band branch of rnnt_loss_multiblank_pruned) against FLOAT64 on structured, non-iid and long
bands (tests/band_multiblank_cases.py): a sharp planted path, two regimes, blank-heavy, tilted, deep, positive values and
-inf / -1e20 holes, on four shapes: a short one with durations (1,2,4,8); 16 lanes with eight blanks up to 32 frames (M = 9,
ring of 64 steps); the shape of the memory test; and the longest walk at r = 2 with a blank of 32 frames.
tests/test_band_multiblank_cases.py shows on the CPU that every case has a path and a finite reference, so every result
here must be finite.  The rule is the project's: ans to 1e-4 relative, occupancies normwise max|d| / max|ref| <= 1e-4.

The loss test puts +12 on the planted path's columns of random logits and runs both routes of rnnt_loss_multiblank_pruned
against tests/multiblank_restatement.py.  It runs without a delay penalty, which enters the loss with either sign and can
bring it near 0, where a relative error says nothing (the penalty is covered by tests/test_gpu_band_multiblank.py); with
sigma = 0.05 every move costs at least 0.05, so |loss| >= 1 at every shape (asserted).

With FTR_BAND_MULTIBLANK_PARITY_OUT set, every case's figures are written to that file as JSON when the module is done; a
run on MI355X is committed as profiles/band_multiblank_parity_errors.json."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import band_multiblank_cases as MC
from helpers import max_rel
from multiblank_restatement import multiblank_loss

pytestmark = pytest.mark.gpu

TOL_F64 = 1e-4
_LOG = {}


@pytest.fixture(scope="module", autouse=True)
def _write_log():
    yield
    path = os.environ.get("FTR_BAND_MULTIBLANK_PARITY_OUT")
    if not path or not _LOG:
        return
    try:
        with open(path, "w") as f:
            json.dump(_LOG, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _n(t):
    return t.detach().cpu().numpy()


def _run_case(ft, dev, case, grads=True):
    x, y = _t(case["pxb"], dev).requires_grad_(grads), _t(case["pyb"], dev).requires_grad_(grads)
    ans = ft.mutual_information_recursion_multiblank_band(x, y, _t(case["ranges"], dev), case["durations"], _t(case["bd"], dev),
                                                          S=case["S"])
    if not grads:
        return _n(ans)
    ans.sum().backward()
    return _n(ans), _n(x.grad), _n(y.grad)


def _norm_err(got, ref):
    """normwise max|d| / max|ref| of one utterance's array."""
    return float(np.abs(got.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def _ans_err(ans, want):
    return float(np.max(np.abs(ans.astype(np.float64) - want) / np.abs(want)))


@pytest.mark.parametrize("shape", MC.SHAPES, ids=MC.shape_id)
@pytest.mark.parametrize("kind", MC.KINDS)
def test_recursion_vs_float64(ft, dev, kind, shape):
    case = MC.make_case(kind, shape)
    a64, gx64, gy64 = MC.reference(kind, shape)
    before = ft._lib.band_multiblank_recursions
    ans, gx, gy = _run_case(ft, dev, case)
    ans2, gx2, gy2 = _run_case(ft, dev, case)
    fwd = _run_case(ft, dev, case, grads=False)
    assert ft._lib.band_multiblank_recursions == before + 3
    fin = bool(np.isfinite(ans).all() and np.isfinite(gx).all() and np.isfinite(gy).all())
    e_ans = _ans_err(ans, a64) if fin else float("nan")
    e_occ = [max(_norm_err(gx[b], gx64[b]), _norm_err(gy[b], gy64[b])) for b in range(case["B"])] if fin else [float("nan")]
    _LOG.setdefault(f"{kind}/{MC.shape_id(shape)}", {})["recursion"] = dict(ans_rel_vs_f64=float(f"{e_ans:.3e}"),
                                                                          occupancy_normwise_vs_f64=float(f"{max(e_occ):.3e}"))
    print(f"band multiblank {kind} {MC.shape_id(shape)}: ans rel {e_ans:.3e}, occupancies per utterance {['%.3e' % e for e in e_occ]}")
    assert np.isfinite(a64).all() and np.isfinite(ans).all(), ans
    assert gx.shape == case["pxb"].shape and gy.shape == case["pyb"].shape
    np.testing.assert_allclose(ans, a64, rtol=TOL_F64, atol=0)
    assert np.isfinite(gx).all() and np.isfinite(gy).all()
    assert max(e_occ) <= TOL_F64, e_occ
    assert ans.tobytes() == ans2.tobytes() and gx.tobytes() == gx2.tobytes() and gy.tobytes() == gy2.tobytes()
    assert fwd.tobytes() == ans.tobytes()


# ----------------------------------------------------------------------------------------------- loss level, both routes
LOSS_C = 24


@functools.lru_cache(maxsize=None)
def _loss_case(shape):
    """(logits [B,T,r,C] float32, symbols, ranges, bd, blank, big_blanks, per-utterance float64 loss, float64 d logits): 2 N(0,1)
    with +12 on the planted path's column (the symbol of a symbol move, the id of the blank it takes otherwise).  The band and
    the path are those of the structured case of the shape; the blank is column 0 and the big blanks the last D - 1 columns."""
    B, S, T, r = shape
    c = MC.make_case("sharp", shape)
    durations, C, blank = c["durations"], LOSS_C, 0
    D = len(durations)
    ids = [blank] + list(range(C - D + 1, C))
    big = tuple(zip(ids[1:], durations[1:]))
    rng = np.random.default_rng([S, T, r, D])
    sym = rng.integers(1, C - D + 1, (B, S)).astype(np.int32)
    x = (2.0 * rng.standard_normal((B, T, r, C))).astype(np.float32)
    for b in range(B):
        sb, tb = int(c["bd"][b, 0]), int(c["bd"][b, 1])
        for s, t, m in c["paths"][b]:
            k = sb + s - c["lo"][b, tb + t]
            x[b, tb + t, k, sym[b, sb + s] if m == 0 else ids[m - 1]] += np.float32(12.0)
    l64 = torch.from_numpy(x).double().requires_grad_(True)
    per = multiblank_loss(l64, sym, c["ranges"], blank, big, c["bd"], 0.05, 0.0)
    per.sum().backward()
    return x, sym, c["ranges"], c["bd"], blank, big, per.detach().numpy(), l64.grad.numpy()


@pytest.mark.parametrize("route", ["band", "lattice"])
@pytest.mark.parametrize("shape", MC.SHAPES, ids=MC.shape_id)
def test_peaked_logits_through_both_routes(ft, dev, monkeypatch, shape, route):
    x, sym, ranges, bd, blank, big, per, grad = _loss_case(shape)
    assert np.isfinite(per).all() and np.isfinite(grad).all() and np.abs(per).min() >= 1.0
    if route == "lattice":
        monkeypatch.setenv("FTR_PRUNED_ROUTE", "lattice")
    else:
        monkeypatch.delenv("FTR_PRUNED_ROUTE", raising=False)
    before = ft._lib.band_multiblank_recursions
    logits = _t(x, dev).requires_grad_(True)
    loss = ft.rnnt_loss_multiblank_pruned(logits, _t(sym, dev), _t(ranges, dev), blank, big, _t(bd, dev), sigma=0.05,
                                          reduction="none")
    loss.sum().backward()
    assert ft._lib.band_multiblank_recursions - before == (1 if route == "band" else 0), route     # the route that was meant
    loss, g = _n(loss), _n(logits.grad)
    assert np.isfinite(loss).all() and np.isfinite(g).all()
    el, eg = _ans_err(loss, per), max_rel(g, grad)
    _LOG.setdefault(f"loss/{MC.shape_id(shape)}", {})[route] = dict(loss_rel_vs_f64=float(f"{el:.3e}"),
                                                                    dlogits_normwise_vs_f64=float(f"{eg:.3e}"))
    print(f"band multiblank peaked loss {MC.shape_id(shape)} route={route}: loss {el:.3e} dlogits {eg:.3e}, loss64 {per}")
    assert el <= TOL_F64 and eg <= TOL_F64, (route, el, eg)
    for b in range(shape[0]):
        te = int(bd[b, 3])
        assert not grad[b, te:].any() and not g[b, te:].any()          # outside the boundary zeros stay zeros, exactly
