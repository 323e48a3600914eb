"""The structured TDT band cases of tests/band_tdt_cases.py are what their docstring says (CPU only): every utterance of
every (kind, shape) has a complete path -- the planted one -- inside its band and its boundary rectangle, the ranges are
what the band kernels accept, the float64 reference is finite, its occupancies survive the gather, and they satisfy the two
oracle-free invariants that tests/test_gpu_band_tdt_structured.py then demands of the GPU's occupancies.  That file relies
on this when it demands finite results everywhere without leaving cases out."""
import numpy as np
import pytest

import band_tdt_cases as TC


@pytest.mark.parametrize("shape", TC.SHAPES, ids=TC.shape_id)
@pytest.mark.parametrize("kind", TC.KINDS)
def test_case_is_well_formed(kind, shape):
    c = TC.make_case(kind, shape)
    B, S, T, r = shape
    tok, blk = c["tok"], c["blk"]
    N, Ny = len(tok), len(blk)
    rg, bd, pxb, pyb = c["ranges"], c["bd"], c["pxb"], c["pyb"]
    assert pxb.dtype == np.float32 and pyb.dtype == np.float32 and rg.dtype == np.int32 and bd.dtype == np.int32
    assert pxb.shape == (B, N, T, r) and pyb.shape == (B, Ny, T, r) and rg.shape == (B, T, r) and bd.shape == (B, 4)
    # ranges: contiguous, non-decreasing, inside [0, S + 1 - r]
    assert np.array_equal(rg, rg[:, :, :1] + np.arange(r, dtype=np.int32))
    assert rg[:, :, 0].min() >= 0 and rg[:, :, 0].max() <= S + 1 - r
    assert np.diff(rg[:, :, 0], axis=1).min() >= 0
    if B > 1:
        assert tuple(bd[1]) == (2, 5, S - 3, T - 7)
    a64, gx64, gy64 = TC.reference(kind, shape)
    assert np.isfinite(gx64).all() and np.isfinite(gy64).all()
    moves = [(1, e) for e in tok] + [(0, d) for d in blk]
    dur = np.array([d for _, d in moves], np.float64)
    for b in range(B):
        sb, tb, se, te = (int(v) for v in bd[b])
        assert 0 <= tb < te <= T and 0 <= sb <= se <= S
        # the planted path, walked move by move: inside the band and the rectangle, on finite entries, ending on (se, te)
        s, t, score = sb, tb, 0.0
        for ps, pt, m in c["paths"][b]:
            assert (sb + ps, tb + pt) == (s, t) and sb <= s <= se and tb <= t < te
            k = s - int(rg[b, t, 0])
            assert 0 <= k < r
            plane, on = (pxb[b, m], c["on_x"][b, m]) if m < N else (pyb[b, m - N], c["on_y"][b, m - N])
            v = float(plane[t, k])
            assert on[t, k] and np.isfinite(v) and v > -1e4
            score += v
            s, t = s + moves[m][0], t + moves[m][1]
        assert (s, t) == (se, te)
        assert c["on_x"][b].sum() + c["on_y"][b].sum() == len(c["paths"][b])
        assert np.isfinite(a64[b]) and a64[b] >= score - 1e-9 * abs(score)       # the planted path is one of the paths
        # on the reference: every symbol row is emitted once, and the durations taken add up to the frames of the rectangle
        rows = TC.band_rows(c)[b]
        per_row = np.bincount(rows.ravel(), weights=gx64[b].sum(axis=0).ravel(), minlength=S + 2)
        np.testing.assert_allclose(per_row[sb:se], 1.0, rtol=1e-12)
        assert not per_row[:sb].any() and not per_row[se:].any()
        frames = (np.concatenate((gx64[b].sum(axis=(1, 2)), gy64[b].sum(axis=(1, 2)))) * dur).sum()
        np.testing.assert_allclose(frames, te - tb, rtol=1e-12)
    # the gather loses no occupancy
    lx, ly = TC.lattice_totals(kind, shape)
    np.testing.assert_allclose(gx64.sum(axis=(1, 2, 3)), lx, rtol=1e-12)
    np.testing.assert_allclose(gy64.sum(axis=(1, 2, 3)), ly, rtol=1e-12)


def test_shapes_and_kinds_are_the_stated_ones():
    assert TC.KINDS == ["sharp", "two_regime", "blank_heavy", "tilted", "deep", "positive", "holes"]
    assert sorted(len(t) + len(k) for t, k in TC.MOVES_OF.values()) == [4, 5, 7, 8, 9, 9, 10]
    for shape, (tok, blk) in TC.CASES:
        c = TC.make_case("holes", shape)
        off_x, off_y = ~c["on_x"], ~c["on_y"]
        assert (c["pxb"][0][off_x[0]] == np.float32(-1e20)).any() and (c["pyb"][0][off_y[0]] == np.float32(-1e20)).any()
        assert not (c["pxb"][1:] == np.float32(-1e20)).any() and not (c["pyb"][1:] == np.float32(-1e20)).any()
        s = TC.make_case("sharp", shape)
        assert (s["pxb"][s["on_x"]] == np.float32(-0.1)).all() and (s["pyb"][s["on_y"]] == np.float32(-0.05)).all()


def test_shift_moves_every_path_by_the_same_amount():
    """`shifted` on the reference itself: ans64 of the shifted operands is ans64 + path_gain (the rounding of the shifted
    float32 operands aside), the occupancies are those of the unshifted ones."""
    shape = TC.SHAPES[0]
    c = TC.make_case("holes", shape)
    a64, gx64, gy64 = TC.reference("holes", shape)
    from tdt_restatement import tdt_dp_with_grads
    for cx, cc in ((-37.5, 11.25), (300.0, -40.0)):
        pxb, pyb = TC.shifted(c, cx, cc)
        assert pxb.dtype == np.float32 and np.array_equal(np.isfinite(pxb), np.isfinite(c["pxb"]))
        assert np.array_equal(np.isneginf(pyb), np.isneginf(c["pyb"]))
        a, gx, gy = tdt_dp_with_grads(TC._scatter(pxb, c["ranges"], c["S"], c["S"], c["T"] + 1),
                                      TC._scatter(pyb, c["ranges"], c["S"], c["S"] + 1, c["T"]), c["tok"], c["blk"], c["bd"])
        steps = (c["bd"][:, 2] - c["bd"][:, 0]) + (c["bd"][:, 3] - c["bd"][:, 1])
        big = max(np.abs(pxb[np.isfinite(pxb) & (pxb > -1e19)]).max(), np.abs(pyb[np.isfinite(pyb) & (pyb > -1e19)]).max())
        assert (np.abs(a - (a64 + TC.path_gain(c, cx, cc))) <= steps * 2.0 ** -24 * big).all()
        assert np.abs(TC._gather(gx, c["ranges"]) - gx64).max() <= 1e-4 and np.abs(TC._gather(gy, c["ranges"]) - gy64).max() <= 1e-4


def test_scatter_gather_round_trip():
    """_gather(_scatter(x)) == x on the band rows the lattice has, 0 on the others; _scatter leaves -inf off the band."""
    rng = np.random.default_rng(5)
    B, P, T, S, r = 2, 3, 9, 6, 3
    lo = np.minimum(np.arange(T)[None, :] // 2 + np.array([[0], [2]]), S + 1 - r)
    lo[1, -1] = S - 1                                       # band rows S and S + 1: the second is beyond every lattice
    ranges = lo[:, :, None] + np.arange(r)
    band = rng.standard_normal((B, P, T, r)).astype(np.float32)
    for rows, cols in ((S, T + 1), (S + 1, T)):
        lat = TC._scatter(band, ranges, S, rows, cols)
        assert lat.shape == (B, P, rows, cols) and lat.dtype == np.float32
        on = np.zeros((B, rows, cols), bool)
        for b in range(B):
            for t in range(T):
                for k in range(r):
                    if ranges[b, t, k] < rows:
                        on[b, ranges[b, t, k], t] = True
        assert np.isneginf(lat[~np.broadcast_to(on[:, None], lat.shape)]).all() and np.isfinite(lat[np.broadcast_to(on[:, None], lat.shape)]).all()
        back = TC._gather(lat, ranges)
        inside = np.broadcast_to((ranges < rows)[:, None], band.shape)
        assert np.array_equal(back[inside], band[inside]) and not back[~inside].any() and (~inside).any()


def test_the_recursions_take_five_moves_of_each_kind():
    """The (2,100,300,8) shape has ten moves.  Both recursions take them (include/ftr_band_tdt.h: N <= 5, Ny <= 5;
    include/ftr.h: Dx + Dy <= 10); the limit of nine moves is the alignment's alone."""
    from tf_fast_rnnt.mutual_information import _check_tdt_moves
    ten = TC.MOVES_OF[(2, 100, 300, 8)]
    assert len(ten[0]) + len(ten[1]) == 10
    assert _check_tdt_moves(*ten) == ten
    with pytest.raises(ValueError, match="at most 9"):
        _check_tdt_moves(*ten, 32, max_moves=9)
    with pytest.raises(ValueError, match="at most 10"):
        _check_tdt_moves((0, 1, 2, 3, 4, 5), (1, 2, 3, 4, 5))
