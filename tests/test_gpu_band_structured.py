"""The band recursion (ftr_mutual_information_band_ws_f32: the LDS and the streaming chain kernels of csrc/mi_band.hip, the
segmented route of csrc/mi_band_seg.hip) against the FLOAT64 oracle on structured, non-iid bands (tests/band_cases.py): a
sharp planted alignment, two regimes that no single mean fits, blank-heavy, tilted, deep (-60 per step), positive values,
and -inf / -1e20 holes -- on shapes chosen for the kernels' code paths (band_cases.SHAPES), both implementations forced in
turn through FTR_BAND_IMPL (read per call).  tests/test_band_cases.py shows on the CPU that every case has a finite float64
answer, so "finite everywhere" is demanded of every case.

What is asserted, all of it against float64 or against no oracle at all:

* ans: finite for every utterance, rtol 1e-4 (the project's loss tolerance).
* occupancies gx_band / gy_band, per utterance: normwise max|d| / max|ref| <= 1e-4 (TOL_F64 of test_gpu_config_parity.py,
  north_star's figure).  The "no worse than the float32 oracle" fallback of helpers.assert_parity is NOT used: on these
  inputs the float32 oracle is itself 6e-4 (sharp) ... 2.9e-1 (deep) away from float64 at T = 2200, which would hide
  nearly anything.
* invariants to 1e-4: the regular type leaves every frame of [t_begin, t_end) through exactly one blank (sum_k gy = 1), the
  modified type through one blank or one symbol (sum_k gx + gy = 1), every symbol row is emitted once (its gx sums to 1);
  exact zeros outside the boundary rectangle.
* shift invariance at band level (kinds sharp and holes): cx added to every finite px entry and cy to every finite py entry
  moves ans by n_x cx + n_y cy (step counts, rtol 3e-6 / atol 3e-5 as test_operand_shift_is_invisible) and leaves the
  occupancies within 1e-4 of the UNSHIFTED float64 ones.
* two launches are bit-identical.

With FTR_BAND_PARITY_OUT set (as FTR_KD_PARITY_OUT of test_gpu_kd.py), every case's figures (relative error of ans, normwise
occupancy error) are written to that file as JSON when the module is done (a run on MI355X is committed as
profiles/band_parity_errors.json); a process that runs with FTR_BAND_FORCE_STREAM (the child of
test_streaming_band_kernel_on_every_size in test_gpu_mi.py, which selects the `chain` cases of the `short` shapes of this
file) adds its figures under "chain+forced_stream".

The last part sends the same structure through the losses: joiner logits 2 N(0,1) with +12 on the planted path's column
(the symbol at an emitting node, blank elsewhere on the path), rnnt_loss_pruned and hat_loss_pruned, both types, both
routes, float32 and bfloat16, against the float64 references of test_gpu_lowp.py (on logits.float()): loss within 1e-4,
gradient normwise 1e-4 (float32) resp. the derived bound of test_gpu_lowp.check_grad (bfloat16).
"""
import json
import os

import numpy as np
import pytest
import torch

import band_cases as BC

pytestmark = pytest.mark.gpu

TOL_F64 = 1e-4          # north_star: loss and px/py gradients within 1e-4 relative
IMPLS = ["chain", "segments"]
SHIFTS = [(-37.5, 11.25), (300.0, -400.0)]
_LOG = {}
_FORCED_STREAM = os.environ.get("FTR_BAND_FORCE_STREAM") is not None      # the library reads it once per process


def _label(impl):
    return impl + ("+forced_stream" if _FORCED_STREAM and impl == "chain" else "")


@pytest.fixture(scope="module", autouse=True)
def _write_log():
    yield
    path = os.environ.get("FTR_BAND_PARITY_OUT")
    if not path or not _LOG:
        return
    try:
        log = {}
        if _FORCED_STREAM and os.path.exists(path):      # the forced-stream child adds to what the suite's own run wrote
            with open(path) as f:
                log = json.load(f)
        for case, figures in _LOG.items():
            log.setdefault(case, {}).update(figures)
        with open(path, "w") as f:
            json.dump(log, f, indent=1, sort_keys=True)
            f.write("\n")
    except (OSError, ValueError):
        pass


def _norm_err(got, ref):
    """normwise max|d| / max|ref| of one utterance's array."""
    return float(np.abs(got.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def run_band(dev, pxb, pyb, case):
    """One launch of ftr_mutual_information_band_ws_f32 -> (ans, gx_band, gy_band) as numpy arrays."""
    from tf_fast_rnnt import _lib
    B, T, S, r = case["B"], case["T"], case["S"], case["r"]
    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tpx, tpy, tbd, trg = t_(pxb), t_(pyb), t_(case["bd"]), t_(case["ranges"])
    ans = torch.full((B,), 7.0, device=dev); gxb = torch.full_like(tpx, 7.0); gyb = torch.full_like(tpy, 7.0)
    assert _lib.lib().ftr_mutual_information_band_supported(T, S, r) in (1, 2)
    nws = _lib.lib().ftr_mutual_information_band_workspace_floats(B, T, S, r)
    bws = torch.empty(max(nws, 1), device=dev)
    _lib.call("ftr_mutual_information_band_ws_f32", tpx.data_ptr(), tpy.data_ptr(), trg.data_ptr(), tbd.data_ptr(), bws.data_ptr(), nws,
              ans.data_ptr(), gxb.data_ptr(), gyb.data_ptr(), B, T, S, r, int(case["modified"]), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return ans.cpu().numpy(), gxb.cpu().numpy(), gyb.cpu().numpy()


def occupancy_errors(case, gx, gy, gx64, gy64):
    """Per utterance: max of the normwise errors of gx_band and gy_band against float64."""
    return [max(_norm_err(gx[b], gx64[b]), _norm_err(gy[b], gy64[b])) for b in range(case["B"])]


def check_invariants(case, gx, gy):
    B, T, S, r, modified = case["shape"]
    gx = gx.astype(np.float64); gy = gy.astype(np.float64)
    for b in range(B):
        sb, tb, se, te = (int(v) for v in case["bd"][b])
        rows = case["s0"][b][:, None] + np.arange(r)[None, :]                   # lattice row of every band cell
        # exact zeros outside the rectangle: frames outside [t_begin, t_end), rows outside [s_begin, s_end] (no symbol leaves s_end)
        assert not gx[b, :tb].any() and not gy[b, :tb].any() and not gx[b, te:].any() and not gy[b, te:].any()
        assert not gx[b][(rows < sb) | (rows >= se)].any() and not gy[b][(rows < sb) | (rows > se)].any()
        per_frame = gy[b, tb:te].sum(axis=1) + (gx[b, tb:te].sum(axis=1) if modified else 0.0)
        assert np.abs(per_frame - 1.0).max() <= 1e-4, (b, float(np.abs(per_frame - 1.0).max()))
        per_symbol = np.bincount(rows.ravel(), weights=gx[b].ravel(), minlength=S + 1)[sb:se]
        assert np.abs(per_symbol - 1.0).max() <= 1e-4, (b, float(np.abs(per_symbol - 1.0).max()))


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("shape", BC.SHAPES, ids=BC.shape_id)
@pytest.mark.parametrize("kind", BC.KINDS)
def test_band_recursion_vs_float64(dev, oracle, kind, shape, impl, monkeypatch):
    monkeypatch.setenv("FTR_BAND_IMPL", impl)
    case = BC.make_case(kind, shape)
    a64, gx64, gy64 = BC.reference(oracle, kind, shape)
    ans, gx, gy = run_band(dev, case["pxb"], case["pyb"], case)
    ans2, gx2, gy2 = run_band(dev, case["pxb"], case["pyb"], case)
    fin = bool(np.isfinite(ans).all() and np.isfinite(gx).all() and np.isfinite(gy).all())
    e_ans = float(np.max(np.abs(ans.astype(np.float64) - a64) / np.abs(a64))) if fin else float("nan")
    e_occ = occupancy_errors(case, gx, gy, gx64, gy64) if fin else [float("nan")]
    _LOG.setdefault(f"{kind}/{BC.shape_id(shape)}", {})[_label(impl)] = dict(ans_rel_vs_f64=float(f"{e_ans:.3e}"),
                                                                               occupancy_normwise_vs_f64=float(f"{max(e_occ):.3e}"))
    print(f"{kind} {BC.shape_id(shape)} {_label(impl)}: ans rel {e_ans:.3e}, occupancies per utterance {['%.3e' % e for e in e_occ]}")
    assert np.isfinite(a64).all() and np.isfinite(ans).all(), ans
    np.testing.assert_allclose(ans, a64, rtol=1e-4, atol=0)
    assert np.isfinite(gx).all() and np.isfinite(gy).all()
    assert max(e_occ) <= TOL_F64, e_occ
    check_invariants(case, gx, gy)
    assert ans.tobytes() == ans2.tobytes() and gx.tobytes() == gx2.tobytes() and gy.tobytes() == gy2.tobytes()


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("shape", BC.SHAPES, ids=BC.shape_id)
@pytest.mark.parametrize("kind", ["sharp", "holes"])
def test_band_shift_is_invisible(dev, oracle, kind, shape, impl, monkeypatch):
    monkeypatch.setenv("FTR_BAND_IMPL", impl)
    case = BC.make_case(kind, shape)
    a64, gx64, gy64 = BC.reference(oracle, kind, shape)
    nx, ny = BC.step_counts(case)
    for cx, cy in SHIFTS:
        pxb, pyb = BC.shifted(case, cx, cy)
        ans, gx, gy = run_band(dev, pxb, pyb, case)
        assert np.isfinite(ans).all() and np.isfinite(gx).all() and np.isfinite(gy).all()
        want = a64 + nx * cx + ny * cy
        e_occ = occupancy_errors(case, gx, gy, gx64, gy64)
        e_ans = float(np.max(np.abs(ans.astype(np.float64) - want) / np.abs(want)))
        _LOG.setdefault(f"{kind}/{BC.shape_id(shape)}", {})[f"{_label(impl)} shift({cx:g},{cy:g})"] = dict(
            ans_rel_vs_f64=float(f"{e_ans:.3e}"), occupancy_normwise_vs_f64=float(f"{max(e_occ):.3e}"))
        print(f"{kind} {BC.shape_id(shape)} {_label(impl)} shift ({cx}, {cy}): ans rel {e_ans:.3e}, occupancies {['%.3e' % e for e in e_occ]}")
        np.testing.assert_allclose(ans, want, rtol=3e-6, atol=3e-5)
        assert max(e_occ) <= TOL_F64, ((cx, cy), e_occ)


# ------------------------------------------------------------------------------------------- the same structure through the losses
LOSS_T, LOSS_S, LOSS_R = 48, 14, 5
LOSS_DTYPES = {"f32": (torch.float32, 0.0), "bf16": (torch.bfloat16, 2.0 ** -8)}      # storage type, its unit roundoff
_LOSS_INPUTS = {}
_LOSS_REFS = {}


def loss_inputs(C, rnnt_type, dtype_name):
    """(case, x [B,T,r,C] cpu tensor in the storage type, symbols, blank): 2 N(0,1) with +12 on the planted path's column.
    The blank is column 0 for C = 36 and the last column for C = 37.  Cached, never modified."""
    key = (C, rnnt_type, dtype_name)
    if key not in _LOSS_INPUTS:
        case = BC.make_case("sharp", (2, LOSS_T, LOSS_S, LOSS_R, rnnt_type == "modified"))
        B, T, S, r = case["B"], case["T"], case["S"], case["r"]
        rng = np.random.default_rng(500 + C)
        blank = 0 if C == 36 else C - 1
        sym = (rng.integers(1, C - 1, (B, S)) if blank == C - 1 else rng.integers(1, C, (B, S))).astype(np.int32)
        x = (2.0 * rng.standard_normal((B, T, r, C))).astype(np.float32)
        rows = np.minimum(case["ranges"], S - 1)
        sym_at = np.take_along_axis(np.broadcast_to(sym[:, None, :], (B, T, S)), rows.astype(np.int64), axis=2)    # [B,T,r]
        b_, t_, k_ = np.nonzero(case["on_x"])
        x[b_, t_, k_, sym_at[b_, t_, k_]] += np.float32(12.0)
        b_, t_, k_ = np.nonzero(case["on_y"])
        x[b_, t_, k_, blank] += np.float32(12.0)
        _LOSS_INPUTS[key] = (case, torch.from_numpy(x).to(LOSS_DTYPES[dtype_name][0]), sym, blank)
    return _LOSS_INPUTS[key]


def loss_reference(oracle, C, rnnt_type, hat, dtype_name):
    """(loss64, g64) of the sum-reduced loss on x.float(): the float64-recursion oracle, or the float64 HAT restatement."""
    key = (C, rnnt_type, hat, dtype_name)
    if key not in _LOSS_REFS:
        case, x, sym, blank = loss_inputs(C, rnnt_type, dtype_name)
        if not hat:
            l64, g64 = oracle.rnnt_loss_pruned_grad(x.float().numpy(), sym, case["ranges"], blank, case["bd"], rnnt_type,
                                                    reduction="sum", dtype=np.float64)
            _LOSS_REFS[key] = (float(l64), np.asarray(g64, np.float64))
        else:
            import hat_restatement as H
            xd = x.double().requires_grad_(True)
            px, py = H.get_hat_logprobs_pruned_torch(xd, torch.from_numpy(sym), torch.from_numpy(case["ranges"]), blank,
                                                     torch.from_numpy(case["bd"]), rnnt_type)
            loss = H.lattice_loss_torch(px, py, case["bd"], rnnt_type).sum()
            loss.backward()
            _LOSS_REFS[key] = (float(loss.detach()), xd.grad.numpy().astype(np.float64))
    return _LOSS_REFS[key]


@pytest.mark.parametrize("route", ["band", "lattice"])
@pytest.mark.parametrize("dtype_name", list(LOSS_DTYPES))
@pytest.mark.parametrize("rnnt_type", ["regular", "modified"])
@pytest.mark.parametrize("hat", [False, True], ids=["rnnt", "hat"])
@pytest.mark.parametrize("C", [36, 37])
def test_sharp_logits_through_the_pruned_losses(ft, dev, oracle, C, hat, rnnt_type, dtype_name, route, monkeypatch):
    monkeypatch.delenv("FTR_BAND_IMPL", raising=False)
    monkeypatch.setenv("FTR_PRUNED_ROUTE", route)
    case, x16, sym, blank = loss_inputs(C, rnnt_type, dtype_name)
    l64, g64 = loss_reference(oracle, C, rnnt_type, hat, dtype_name)
    assert np.isfinite(l64) and np.isfinite(g64).all()
    x = x16.to(dev).requires_grad_(True)
    f = ft.hat_loss_pruned if hat else ft.rnnt_loss_pruned
    loss = f(x, torch.from_numpy(sym).to(dev), torch.from_numpy(case["ranges"]).to(dev), blank, torch.from_numpy(case["bd"]).to(dev),
             rnnt_type=rnnt_type, reduction="sum")
    loss.backward()
    assert loss.dtype == torch.float32 and x.grad.dtype == x16.dtype
    g = x.grad.float().cpu().numpy().astype(np.float64)
    u = LOSS_DTYPES[dtype_name][1]
    # float32: normwise 1e-4.  bfloat16: the bound of test_gpu_lowp.check_grad -- one rounding of the float32 gradient into
    # the storage type (u |g64|) on top of the same float32 budget; bfloat16 has float32's exponent range (no subnormal term)
    bound = u * np.abs(g64) + 1e-4 * np.abs(g64).max()
    worst = float((np.abs(g - g64) / bound).max())
    e_loss = abs(loss.item() - l64) / abs(l64)
    print(f"C={C} {'hat' if hat else 'rnnt'} {rnnt_type} {dtype_name} {route}: loss {loss.item():.6f} vs {l64:.6f} (rel {e_loss:.3e}), "
          f"max |g - g64| / bound = {worst:.3g}, max |g64| = {np.abs(g64).max():.3g}")
    assert e_loss <= 1e-4
    assert np.isfinite(g).all() and worst <= 1.0, worst
    te = int(case["bd"][1, 3])
    assert (g64[1, te:] == 0).all() and (g[1, te:] == 0).all()       # outside the boundary zeros stay zeros, exactly
