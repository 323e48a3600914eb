"""The structured band cases of tests/band_cases.py are what their docstring says (CPU only): every utterance of every
(kind, shape) has a complete path -- the planted one -- inside its ranges and its boundary rectangle, the ranges are what
the band kernels accept, and the float64 reference is finite.  tests/test_gpu_band_structured.py relies on this when it
demands finite results everywhere without leaving cases out."""
import numpy as np
import pytest

import band_cases as BC


@pytest.mark.parametrize("shape", BC.SHAPES, ids=BC.shape_id)
@pytest.mark.parametrize("kind", BC.KINDS)
def test_case_is_well_formed(oracle, kind, shape):
    c = BC.make_case(kind, shape)
    B, T, S, r, modified = shape
    s0, bd, rg = c["s0"], c["bd"], c["ranges"]
    assert c["pxb"].dtype == np.float32 and c["pyb"].dtype == np.float32 and rg.dtype == np.int32
    # ranges: contiguous, inside [0, S], monotone with steps <= r - 1
    assert np.array_equal(rg, rg[:, :, :1] + np.arange(r, dtype=np.int32))
    assert rg[:, :, 0].min() >= 0 and rg[:, :, 0].max() <= max(S + 1 - r, 0)
    d = np.diff(s0, axis=1)
    assert d.min() >= 0 and d.max() <= r - 1
    for b in range(B):
        ts = c["ts"][b]
        sb, tb, se, te = (int(v) for v in bd[b])
        assert 0 <= tb < te <= T and 0 <= sb <= se <= S
        assert len(ts) == S and (np.diff(ts) >= (1 if modified else 0)).all() and ts.min() >= 0 and ts.max() <= T - 1
        # the planted path, walked inside the rectangle: every transition is a finite band entry, and it ends on (se, te)
        e = BC.emitted_before(ts, T)
        assert sb == e[tb] and se == e[te]
        s, score, t = sb, 0.0, tb
        while t < te:
            syms = np.flatnonzero(ts == t) if not modified else np.flatnonzero(ts == t)[:1]
            emitted = False
            for sym in syms:
                assert sym == s and s < se
                k = s - s0[b, t]
                assert 0 <= k < r and c["on_x"][b, t, k] and np.isfinite(c["pxb"][b, t, k]) and c["pxb"][b, t, k] > -1e4
                assert c["px"][b, s, t] == c["pxb"][b, t, k]
                score += float(c["pxb"][b, t, k]); s += 1; emitted = True
            if not (modified and emitted):
                k = s - s0[b, t]
                assert 0 <= k < r and c["on_y"][b, t, k] and np.isfinite(c["pyb"][b, t, k]) and c["pyb"][b, t, k] > -1e4
                assert c["py"][b, s, t] == c["pyb"][b, t, k]
                score += float(c["pyb"][b, t, k])
            t += 1
        assert s == se
        a64, gx64, gy64 = BC.reference(oracle, kind, shape)
        assert np.isfinite(a64[b]) and a64[b] >= score - 1e-9 * abs(score)       # the planted path is one of the paths
    # the occupancies live on the band: the collapse loses none of them, and every frame is left exactly once
    a64, gx64, gy64 = BC.reference(oracle, kind, shape)
    _, (lgx, lgy) = oracle.mutual_information_recursion(c["px"], c["py"], bd, True, np.float64)
    assert np.isfinite(gx64).all() and np.isfinite(gy64).all()
    np.testing.assert_allclose(gx64.sum(axis=(1, 2)), lgx.sum(axis=(1, 2)), rtol=1e-12)
    np.testing.assert_allclose(gy64.sum(axis=(1, 2)), lgy.sum(axis=(1, 2)), rtol=1e-12)
    for b in range(B):
        tb, te = int(bd[b, 1]), int(bd[b, 3])
        per_frame = gy64[b, tb:te].sum(axis=1) + (gx64[b, tb:te].sum(axis=1) if modified else 0.0)
        np.testing.assert_allclose(per_frame, 1.0, rtol=1e-9)


def test_band_lattice_round_trip():
    """lattice_to_band(band_to_lattice(x)) == x on the cells the lattice has; band_to_lattice writes the builder's -inf."""
    rng = np.random.default_rng(3)
    B, T, S, r = 2, 9, 6, 3
    s0 = np.minimum(np.arange(T)[None, :] // 2, S + 1 - r) * np.ones((B, 1), np.int64)
    bd = np.array([[0, 0, S, T], [0, 0, S, T - 2]], np.int32)
    for modified in (False, True):
        pxb = rng.standard_normal((B, T, r)).astype(np.float32); pyb = rng.standard_normal((B, T, r)).astype(np.float32)
        px, py = BC.band_to_lattice(pxb, pyb, s0, bd, S, modified)
        assert px.shape == (B, S, T if modified else T + 1) and py.shape == (B, S + 1, T)
        assert np.isneginf(pxb[:, -1, -1]).all() and np.isfinite(pyb[:, -1, -1]).all()      # row S: no symbol, a blank
        assert np.isneginf(pxb[1, T - 2]).all() == (not modified)                            # column t_end, regular type
        ex, ey = BC.lattice_to_band(np.where(np.isfinite(px), px, 0.0), py, s0, r)
        assert np.array_equal(ex, np.where(np.isfinite(pxb), pxb, 0.0)) and np.array_equal(ey, pyb)
