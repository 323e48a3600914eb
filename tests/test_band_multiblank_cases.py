"""The band cases of tests/band_multiblank_cases.py are what their docstring says (CPU only): the path planter handles a
blank of 32 frames, every utterance of every structured (kind, shape) has a complete path -- the planted one -- inside its
band and its boundary rectangle, the ranges are what the band kernels accept, the float64 reference is finite, its
occupancies survive the gather and satisfy the two oracle-free invariants.  tests/test_gpu_band_multiblank_structured.py
relies on this when it demands finite results everywhere without leaving cases out."""
import numpy as np
import pytest

import band_multiblank_cases as MC
from band_tdt_cases import _random_path


def test_the_planter_is_wide_enough_for_a_blank_of_32_frames():
    rng = np.random.default_rng(0)
    with pytest.raises(IndexError):                       # the TDT planter's table ends 16 frames past the last column
        _random_path(rng, 7, 80, (0,), (1, 32), 3)
    for durations in ((1, 32), (32,), (2, 3), (1, 2, 4, 8, 16, 17, 31, 32)):
        path = MC.random_path(rng, 7, 65, durations, 4)
        assert path is not None
        s = t = 0
        for ps, pt, m in path:
            assert (ps, pt) == (s, t)
            s, t = (s + 1, t) if m == 0 else (s, t + durations[m - 1])
        assert (s, t) == (6, 64)
    assert MC.random_path(rng, 6, 2, (1,), 4) is None       # six rows on one frame do not fit a band of four
    assert MC.random_path(rng, 3, 2, (2, 3), 4) is None     # no blank lands on the last column


def test_recursion_cases_cover_every_chunk_residue():
    """The chain fetches its operands four walk steps at a time: (S_n + T_n) mod 4 takes every value over the full
    rectangles of the GPU parity test's shapes alone; and only the one-frame shape is without a path."""
    assert {(S + T) % 4 for _, S, T, _ in MC.RECURSION_SHAPES} == {0, 1, 2, 3}
    for shape in MC.RECURSION_SHAPES[:4]:
        for durations in MC.RECURSION_DURATIONS:
            for with_boundary in (False, True):
                has_path, (a64, gx64, gy64) = MC.recursion_case(shape, durations, with_boundary)[4:]
                assert has_path == (shape != MC.ONE_FRAME), (shape, durations, with_boundary)
                if has_path:
                    assert np.isfinite(a64).all()
                else:
                    assert (a64 == MC.NEG).all() and not gx64.any() and not gy64.any()


@pytest.mark.parametrize("shape", MC.SHAPES, ids=MC.shape_id)
@pytest.mark.parametrize("kind", ["sharp", "holes"])
def test_case_is_well_formed(kind, shape):
    c = MC.make_case(kind, shape)
    B, S, T, r = shape
    durations = c["durations"]
    D = len(durations)
    rg, bd, pxb, pyb = c["ranges"], c["bd"], c["pxb"], c["pyb"]
    assert pxb.dtype == np.float32 and pyb.dtype == np.float32 and rg.dtype == np.int32 and bd.dtype == np.int32
    assert pxb.shape == (B, T, r) and pyb.shape == (B, D, T, r) and rg.shape == (B, T, r) and bd.shape == (B, 4)
    assert np.array_equal(rg, rg[:, :, :1] + np.arange(r, dtype=np.int32))
    assert rg[:, :, 0].min() >= 0 and rg[:, :, 0].max() <= S + 1 - r and np.diff(rg[:, :, 0], axis=1).min() >= 0
    a64, gx64, gy64 = MC.reference(kind, shape)
    assert np.isfinite(gx64).all() and np.isfinite(gy64).all()
    for b in range(B):
        sb, tb, se, te = (int(v) for v in bd[b])
        assert 0 <= tb < te <= T and 0 <= sb <= se <= S
        s, t, score = sb, tb, 0.0
        for ps, pt, m in c["paths"][b]:                   # the planted path, move by move, on finite entries of the band
            assert (sb + ps, tb + pt) == (s, t) and sb <= s <= se and tb <= t < te
            k = s - int(rg[b, t, 0])
            assert 0 <= k < r
            plane, on = (pxb[b], c["on_x"][b]) if m == 0 else (pyb[b, m - 1], c["on_y"][b, m - 1])
            v = float(plane[t, k])
            assert on[t, k] and np.isfinite(v) and v > -1e4
            score += v
            s, t = (s + 1, t) if m == 0 else (s, t + durations[m - 1])
        assert (s, t) == (se, te)
        assert np.isfinite(a64[b]) and a64[b] >= score - 1e-9 * abs(score)       # the planted path is one of the paths
        # every symbol row is emitted once, and the durations taken add up to the frames of the rectangle
        per_row = np.bincount(rg[b].astype(np.int64).ravel(), weights=gx64[b].ravel(), minlength=S + 2)
        np.testing.assert_allclose(per_row[sb:se], 1.0, rtol=1e-12)
        assert not per_row[:sb].any() and not per_row[se:].any()
        np.testing.assert_allclose((gy64[b].sum(axis=(1, 2)) * np.array(durations, np.float64)).sum(), te - tb, rtol=1e-12)
    lx, ly = MC.lattice_totals(kind, shape)                # the gather loses no occupancy
    np.testing.assert_allclose(gx64.sum(axis=(1, 2)), lx, rtol=1e-12)
    np.testing.assert_allclose(gy64.sum(axis=(1, 2, 3)), ly, rtol=1e-12)
