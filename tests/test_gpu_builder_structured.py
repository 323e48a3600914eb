"""The simple and the smoothed px / py builders (get_rnnt_logprobs, get_rnnt_logprobs_smoothed, rnnt_loss_simple,
rnnt_loss_smoothed: rowmax_exp*, the f32-MFMA simple_fused_fwd_kernel, the library-GEMM route with simple_fwd_kernel,
simple_bwd_w_kernel, simple_bwd_am_kernel and its fused MFMA twin, simple_bwd_lm*, and the torch glue of _smoothed_forward)
against FLOAT64 on trained-model-shaped am / lm (tests/builder_cases.py): peaked logits that agree or conflict, normaliser
products down to 8e-35, row offsets of hundreds, -inf columns, and products that are subnormal or exactly 0 in float32.
tests/test_builder_cases.py shows on the CPU that the float64 references are finite, that the kinds are what they are named
for, and that the float32 reference arithmetic itself meets every bound asserted here with room to spare.  FTR_GEMM_TUNE=off,
as in the view tests (the library would otherwise swap the GEMM kernel between two launches of a shape).

Forward, all seven kinds, every type: both builders (the smoothed one with three pairs of scales) through the default fused
route, the fused route forced to 128-frame tiles x 7 symbol blocks and to 64-frame tiles x 4 symbol blocks, and the
library-GEMM route.  The exact -inf pattern; no NaN, no +inf; elementwise

    |v - v64| <= 2e-5 + 1e-5 |v64| + k 2^-24 (|a| + |l| + |lm_max| + |am_max| + |nrm64|),   k = builder_cases.K_ROUND = 4

(the project's px / py tolerance plus the rounding of sums of large offsets; the same formula for px and py of every type,
the constrained px = px' + py[1:] included; the float32 oracle reaches at most 0.27 of it); on the `subnormal` and `zero` kinds plus
2 C tiny / prod64 on the cells whose product is at least 2^10 C tiny, and on the others: a finite value and (simple
builder) a normaliser not below log(tiny) + lm_max + am_max - 1e-3.  rnnt_loss_simple / rnnt_loss_smoothed with
delay_penalty = 0.3 within rtol 1e-4 of the float64 recursion on the float64 px / py, every kind.  Two launches are
bit-identical.

Backward, the sound kinds: FTR_BUILDER_BWD=library and =fused (where ftr_simple_logprobs_fused_bwd_supported), the simple
builder and the smoothed one (scales (0.1, 0.2) and (0.25, 0.0)), weights (a) seeded N(0,1) and (b) minus the float64
occupancies.  d am and d lm finite and normwise within 1e-4 of float64 PER UTTERANCE (TOL_F64; no "no worse than the float32
oracle" fallback: the float32 restatement is within 2.9e-6 on every case); exactly 0 in masked columns; for (b) exactly 0 outside the
boundary (d am; d lm for the simple builder -- the smoothed builder's batch-wide unigram mean reaches every lm row, and with
(a) the upstream weights are not 0 there) and every d am row inside the boundary and every d lm row sums to 0 within
1e-4 max|g| (a softmax gradient).  On `subnormal` and `zero` the reference arithmetic has no finite gradient
(test_unsound_kinds_have_no_float32_gradient): whether the GPU's is finite is recorded, and the padding gets exact zeros
when the upstream gradient has them there.

The chain, once per type on agree12 and conflict25: occupancies of rnnt_loss_simple within 1e-4 of float64; get_rnnt_prune_ranges
on the GPU's occupancies bit-identical to the oracle on the same arrays (r = 3, 5: saturated occupancies tie exactly, the
first maximum decides); do_rnnt_pruning + am_p + lm_p + rnnt_loss_pruned against oracle.rnnt_loss_pruned_grad(float64).  (That the
planted path lies in the band is not asserted: see tests/test_builder_cases.py.)

With FTR_BUILDER_PARITY_OUT set (as FTR_BAND_PARITY_OUT), every case's worst figures go to that file as JSON when the module
is done (_summary); a run on MI355X is committed as profiles/builder_parity_errors.json.
"""
import json
import os

import numpy as np
import pytest
import torch

import builder_cases as BC

pytestmark = pytest.mark.gpu

TOL_F64 = 1e-4          # north_star: loss and gradients within 1e-4 relative
LOG_TINY = float(np.log(BC.TINY))
FWD_ROUTES = {
    "fused": {},
    "fused_ft128_ns7": {"FTR_FUSED_FT": "128", "FTR_FUSED_NS": "7"},
    "fused_ft64_ns4": {"FTR_FUSED_FT": "64", "FTR_FUSED_NS": "4"},
    "library": {"FTR_BUILDER_GEMM": "library"},
}
_KNOBS = ("FTR_FUSED_FT", "FTR_FUSED_NS", "FTR_BUILDER_GEMM", "FTR_BUILDER_BWD")
MUST_RUN_FUSED_BWD = [(2, 72, 33, 36), (1, 68, 70, 304)]
_LOG = {}


def _worst(into, figures):
    for k, v in figures.items():
        if isinstance(v, bool):
            into[k] = into.get(k, True) and v
        else:
            into[k] = v if k not in into or not v <= into[k] else into[k]        # the maximum; a NaN wins


def _summary(log):
    """What goes to the file, one entry per case: the worst figure over the three fused tilings ("fused") and over the
    smoothed builder's scales ("smoothed"), and for the gradients also over the two weight sets."""
    out = {}
    for case, sections in log.items():
        rec = out[case] = {}
        for section in ("forward", "backward", "gradient_finite"):
            for label, figures in sections.get(section, {}).items():
                builder, route = label.split("/")[:2]
                key = f"{'simple' if builder == 'simple' else 'smoothed'}/{'fused' if route.startswith('fused') else route}"
                _worst(rec.setdefault(section, {}).setdefault(key, {}), figures)
        if "chain" in sections:
            rec["chain"] = sections["chain"]
    return out


@pytest.fixture(scope="module", autouse=True)
def _write_log():
    yield
    path = os.environ.get("FTR_BUILDER_PARITY_OUT")
    if not path or not _LOG:
        return
    lines = [f' {json.dumps(case)}: {json.dumps(rec, sort_keys=True)}' for case, rec in sorted(_summary(_LOG).items())]
    with open(path, "w") as f:         # whoever set the variable asked for the file: an error here is an error
        f.write("{\n" + ",\n".join(lines) + "\n}\n")


@pytest.fixture(autouse=True)
def _pinned(monkeypatch):
    monkeypatch.setenv("FTR_GEMM_TUNE", "off")
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)


def _route(monkeypatch, env):
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _sig(x):
    return float(f"{x:.3e}")


def _entry(kind, shape, rnnt_type):
    return _LOG.setdefault(f"{kind}/{BC.shape_id(shape)}/{rnnt_type}", {})


def _inputs(c, dev, grad=False):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t(c["lm"]).requires_grad_(grad), t(c["am"]).requires_grad_(grad), t(c["symbols"]), t(c["boundary"])


def _logprobs(ft, c, builder, rnnt_type, lm, am, sym, bd):
    if builder is None:
        return ft.get_rnnt_logprobs(lm, am, sym, c["blank"], rnnt_type, bd)
    return ft.get_rnnt_logprobs_smoothed(lm, am, sym, c["blank"], builder[0], builder[1], bd, rnnt_type)


def _loss(ft, c, builder, rnnt_type, lm, am, sym, bd, **kw):
    if builder is None:
        return ft.rnnt_loss_simple(lm, am, sym, c["blank"], boundary=bd, rnnt_type=rnnt_type, **kw)
    return ft.rnnt_loss_smoothed(lm, am, sym, c["blank"], lm_only_scale=builder[0], am_only_scale=builder[1], boundary=bd,
                                 rnnt_type=rnnt_type, **kw)


def _fwd_routes(ft, C):
    from tf_fast_rnnt import _lib
    return FWD_ROUTES if _lib.lib().ftr_simple_logprobs_fused_supported(C) else {"library": FWD_ROUTES["library"]}


def check_forward(ref, kind, rnnt_type, builder, px, py):
    """The forward assertions on one launch's px / py (numpy); returns the worst ratio to the bound."""
    c = ref["case"]
    unsound = kind in BC.UNSOUND
    pat = np.isneginf(ref["px"])
    assert px.shape == ref["px"].shape and py.shape == ref["py"].shape
    assert np.array_equal(np.isneginf(px), pat) and not np.isneginf(py).any()
    assert not np.isnan(px).any() and not np.isnan(py).any() and not np.isposinf(px).any() and not np.isposinf(py).any()
    bx, by, low, lowx = BC.forward_bounds(ref, rnnt_type, unsound)
    ratio = max(BC.bound_ratio(px, ref["px"], bx, lowx), BC.bound_ratio(py, ref["py"], by, low))
    if unsound and builder is None:      # below the cut: the normaliser, read back from py, has its floor
        am = c["am"].astype(np.float64); lm = c["lm"].astype(np.float64)
        nrm = am[:, :, c["blank"]][:, None, :] + lm[:, :, c["blank"]][:, :, None] - py.astype(np.float64)
        floor = LOG_TINY + lm.max(axis=2)[:, :, None] + am.max(axis=2)[:, None, :]
        assert (nrm >= floor - 1e-3).all(), float((nrm - floor).min())
    return ratio


@pytest.mark.parametrize("rnnt_type", BC.TYPES)
@pytest.mark.parametrize("shape", BC.SHAPES, ids=BC.shape_id)
@pytest.mark.parametrize("kind", BC.KINDS)
def test_builder_forward_vs_float64(ft, dev, oracle, kind, shape, rnnt_type, monkeypatch):
    entry = _entry(kind, shape, rnnt_type).setdefault("forward", {})
    failures = []
    for builder in BC.BUILDERS:
        ref = BC.reference(oracle, kind, shape, rnnt_type, builder)
        c = ref["case"]
        l64 = BC.loss64(oracle, ref, rnnt_type, 0.3)
        assert np.isfinite(l64).all()
        for route, env in _fwd_routes(ft, c["C"]).items():
            _route(monkeypatch, env)
            lm, am, sym, bd = _inputs(c, dev)
            px, py = (x.cpu().numpy() for x in _logprobs(ft, c, builder, rnnt_type, lm, am, sym, bd))
            px2, py2 = (x.cpu().numpy() for x in _logprobs(ft, c, builder, rnnt_type, lm, am, sym, bd))
            loss = _loss(ft, c, builder, rnnt_type, lm, am, sym, bd, delay_penalty=0.3, reduction="none").cpu().numpy()
            loss2 = _loss(ft, c, builder, rnnt_type, lm, am, sym, bd, delay_penalty=0.3, reduction="none").cpu().numpy()
            label = f"{BC.builder_id(builder)}/{route}"
            ratio = check_forward(ref, kind, rnnt_type, builder, px, py)
            e_loss = float(np.max(np.abs(loss.astype(np.float64) - l64) / np.abs(l64))) if np.isfinite(loss).all() else float("nan")
            entry[label] = dict(worst_ratio_to_bound=_sig(ratio), loss_rel_vs_f64=_sig(e_loss))
            print(f"{kind} {BC.shape_id(shape)} {rnnt_type} {label}: worst |v - v64| / bound {ratio:.3f}, loss rel {e_loss:.3e}")
            if not ratio <= 1.0: failures.append((label, "bound", ratio))
            if not e_loss <= 1e-4: failures.append((label, "loss", e_loss))
            assert px.tobytes() == px2.tobytes() and py.tobytes() == py2.tobytes() and loss.tobytes() == loss2.tobytes(), label
    assert not failures, failures


def gpu_grads(ft, dev, c, builder, rnnt_type, weights):
    """d / d (am, lm) of (px wx).sum() + (py wy).sum() over the finite cells on the GPU's builder, as numpy arrays."""
    lm, am, sym, bd = _inputs(c, dev, grad=True)
    px, py = _logprobs(ft, c, builder, rnnt_type, lm, am, sym, bd)
    wx, wy = (w.to(dev) for w in weights)
    finite = torch.isfinite(px.detach())
    (torch.where(finite, px, torch.zeros_like(px)) * wx).sum().add((py * wy).sum()).backward()
    return am.grad.cpu().numpy(), lm.grad.cpu().numpy()


def _bwd_routes(c):
    from tf_fast_rnnt import _lib
    routes = ["library"]
    if _lib.lib().ftr_simple_logprobs_fused_supported(c["C"]) and _lib.lib().ftr_simple_logprobs_fused_bwd_supported(c["T"], c["C"]):
        routes.append("fused")
    if c["shape"] in MUST_RUN_FUSED_BWD:
        assert "fused" in routes
    return routes


@pytest.mark.parametrize("rnnt_type", BC.TYPES)
@pytest.mark.parametrize("shape", BC.SHAPES, ids=BC.shape_id)
@pytest.mark.parametrize("kind", BC.SOUND)
def test_builder_backward_vs_float64(ft, dev, oracle, kind, shape, rnnt_type, monkeypatch):
    entry = _entry(kind, shape, rnnt_type).setdefault("backward", {})
    failures = []
    for builder in BC.BWD_BUILDERS:
        ref = BC.reference(oracle, kind, shape, rnnt_type, builder)
        c = ref["case"]
        B = c["B"]
        for route in _bwd_routes(c):
            _route(monkeypatch, {"FTR_BUILDER_BWD": route})
            for w in ("a", "b"):
                label = f"{BC.builder_id(builder)}/{route}/{w}"
                gam64, glm64 = ref["grads"][w]
                gam, glm = gpu_grads(ft, dev, c, builder, rnnt_type, ref["weights"][w])
                fin = bool(np.isfinite(gam).all() and np.isfinite(glm).all())
                e_am = [BC.norm_err(gam[b], gam64[b]) for b in range(B)] if fin else [float("nan")]
                e_lm = [BC.norm_err(glm[b], glm64[b]) for b in range(B)] if fin else [float("nan")]
                entry[label] = dict(d_am_normwise_vs_f64=_sig(max(e_am)), d_lm_normwise_vs_f64=_sig(max(e_lm)))
                print(f"{kind} {BC.shape_id(shape)} {rnnt_type} {label}: d am {['%.2e' % e for e in e_am]}, d lm {['%.2e' % e for e in e_lm]}")
                if not fin:
                    failures.append((label, "not finite")); continue
                if not max(e_am) <= TOL_F64: failures.append((label, "d am", e_am))
                if not max(e_lm) <= TOL_F64: failures.append((label, "d lm", e_lm))
                if c["masked_lm"] is not None:
                    assert not gam[:, :, c["masked_am"]].any() and not glm[:, :, c["masked_lm"]].any(), label
                if w == "b":
                    for b in range(B):
                        se, te = int(c["boundary"][b, 2]), int(c["boundary"][b, 3])
                        assert not gam[b, te:].any(), label
                        if builder is None:
                            assert not glm[b, se + 1:].any(), label
                        g = gam[b, :te].astype(np.float64); h = glm[b].astype(np.float64)
                        assert np.abs(g.sum(axis=1)).max() <= 1e-4 * np.abs(g).max(), label
                        assert np.abs(h.sum(axis=1)).max() <= 1e-4 * np.abs(h).max(), label
    assert not failures, failures


@pytest.mark.parametrize("rnnt_type", BC.TYPES)
@pytest.mark.parametrize("shape", BC.SHAPES, ids=BC.shape_id)
@pytest.mark.parametrize("kind", BC.UNSOUND)
def test_unsound_backward_is_recorded(ft, dev, oracle, kind, shape, rnnt_type, monkeypatch):
    """No value inside the boundary is asserted (the reference arithmetic has no gradient below the normal range): whether
    the gradients are finite goes to the record.  What the reference arithmetic does give, also here, is exact zeros in the
    padding when the upstream gradient is zero there: 0 / (0 + tiny) = 0 (test_unsound_kinds_have_no_float32_gradient)."""
    entry = _entry(kind, shape, rnnt_type).setdefault("gradient_finite", {})
    c = BC.make_case(kind, shape, rnnt_type != "regular")
    for builder in (None, (0.1, 0.2)):
        for route in _bwd_routes(c):
            _route(monkeypatch, {"FTR_BUILDER_BWD": route})
            gam, glm = gpu_grads(ft, dev, c, builder, rnnt_type, BC.boundary_weights(c, rnnt_type))
            assert gam.shape == c["am"].shape and glm.shape == c["lm"].shape
            entry[f"{BC.builder_id(builder)}/{route}"] = dict(d_am=bool(np.isfinite(gam).all()), d_lm=bool(np.isfinite(glm).all()))
            for b in range(c["B"]):
                se, te = int(c["boundary"][b, 2]), int(c["boundary"][b, 3])
                assert not gam[b, te:].any(), (BC.builder_id(builder), route, b)
                if builder is None:
                    assert not glm[b, se + 1:].any(), (route, b)


CHAIN_SHAPES = [(2, 130, 20, 37), (2, 72, 33, 36)]


@pytest.mark.parametrize("rnnt_type", BC.TYPES)
@pytest.mark.parametrize("shape", CHAIN_SHAPES, ids=BC.shape_id)
@pytest.mark.parametrize("kind", ["agree12", "conflict25"])
def test_chain_from_simple_loss_to_pruned_loss(ft, dev, oracle, kind, shape, rnnt_type):
    ref = BC.reference(oracle, kind, shape, rnnt_type, None)
    c = ref["case"]
    B, blank, bd_np = c["B"], c["blank"], c["boundary"]
    entry = _entry(kind, shape, rnnt_type).setdefault("chain", {})
    lm, am, sym, bd = _inputs(c, dev)
    # 1. the occupancies of the simple loss
    loss, (gx, gy) = ft.rnnt_loss_simple(lm, am, sym, blank, boundary=bd, rnnt_type=rnnt_type, reduction="none", calc_gradients=True)
    gx_np, gy_np = gx.cpu().numpy(), gy.cpu().numpy()
    gx64, gy64 = ref["occ"]
    e_occ = [max(BC.norm_err(gx_np[b], gx64[b]), BC.norm_err(gy_np[b], gy64[b])) for b in range(B)]
    entry["occupancy_normwise_vs_f64"] = _sig(max(e_occ))
    np.testing.assert_allclose(loss.cpu().numpy(), -ref["ans64"], rtol=1e-4)
    assert np.isfinite(gx_np).all() and np.isfinite(gy_np).all() and max(e_occ) <= TOL_F64, e_occ
    for r in (3, 5):
        # 2. ranges: an integer function of the occupancies, bit-exact given the same arrays
        ranges = ft.get_rnnt_prune_ranges(gx, gy, bd, r)
        want = oracle.get_rnnt_prune_ranges(gx_np, gy_np, bd_np, r)
        assert np.array_equal(ranges.cpu().numpy(), want), r
        # 4. the pruned loss on the joiner am_p + lm_p
        am_p, lm_p = ft.do_rnnt_pruning(am, lm, ranges)
        logits = (am_p + lm_p).detach().requires_grad_(True)
        pl = ft.rnnt_loss_pruned(logits, sym, ranges, blank, bd, rnnt_type=rnnt_type, reduction="sum")
        pl.backward()
        l64, g64 = oracle.rnnt_loss_pruned_grad(logits.detach().cpu().numpy(), c["symbols"], want, blank, bd_np, rnnt_type,
                                                reduction="sum", dtype=np.float64)
        g = logits.grad.cpu().numpy()
        e_g = [BC.norm_err(g[b], g64[b].astype(np.float64)) for b in range(B)]
        e_l = abs(pl.item() - float(l64)) / abs(float(l64))
        entry[f"r{r}"] = dict(pruned_loss_rel_vs_f64=_sig(e_l), d_logits_normwise_vs_f64=_sig(max(e_g)))
        print(f"{kind} {BC.shape_id(shape)} {rnnt_type} r={r}: occupancies {['%.2e' % e for e in e_occ]}, pruned loss rel {e_l:.3e}, d logits {['%.2e' % e for e in e_g]}")
        assert np.isfinite(l64) and e_l <= 1e-4, (r, pl.item(), float(l64))
        assert np.isfinite(g).all() and max(e_g) <= TOL_F64, (r, e_g)
