"""Best-path (Viterbi) alignment, CPU side: the float32 restatement against brute-force enumeration of every path, the
exported surface, and the error paths that need no device."""
import ctypes

import numpy as np
import pytest
import torch

import viterbi_restatement as VR


def _case(rng, B, S, T, modified, integer=False):
    T1 = T if modified else T + 1
    if integer:
        px = rng.integers(-3, 1, (B, S, T1)).astype(np.float32)
        py = rng.integers(-3, 1, (B, S + 1, T)).astype(np.float32)
    else:
        px = rng.standard_normal((B, S, T1)).astype(np.float32)
        py = rng.standard_normal((B, S + 1, T)).astype(np.float32)
    return px, py


@pytest.mark.parametrize("modified", [False, True])
def test_restatement_matches_brute_force(modified):
    rng = np.random.default_rng(11 + modified)
    for S, T in [(1, 1), (2, 3), (3, 5), (4, 4), (5, 6), (0, 4), (3, 0)]:
        px, py = _case(rng, 3, S, T, modified)
        bd = np.array([[0, 0, S, T],
                       [min(1, S), min(1, T), S, T],
                       [min(1, S), min(2, T), max(S - 1, min(1, S)), T]], np.int32)
        for boundary in (None, bd):
            got = VR.viterbi(px, py, boundary)
            want = VR.brute_force(px, py, boundary)
            assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32)), (S, T, got[0], want[0])
            assert np.array_equal(got[1], want[1]), (S, T, got[1], want[1])


@pytest.mark.parametrize("modified", [False, True])
def test_restatement_frames_are_a_path(modified):
    """Re-summing px / py along the path given by frames reproduces the score bit for bit, also with ties everywhere."""
    rng = np.random.default_rng(5)
    S, T = 7, 12
    px, py = _case(rng, 4, S, T, modified, integer=True)
    score, frames = VR.viterbi(px, py)
    for b in range(4):
        acc, s, t = np.float32(0), 0, 0
        while s < S or t < T:
            if s < S and frames[b, s] == t:
                acc = np.float32(acc + px[b, s, t]); s += 1; t += 1 if modified else 0
            else:
                acc = np.float32(acc + py[b, s, t]); t += 1
        assert acc == score[b]
        d = np.diff(frames[b])
        assert (d > 0).all() if modified else (d >= 0).all()


def test_restatement_edges():
    px = np.zeros((2, 3, 5), np.float32); py = np.zeros((2, 4, 4), np.float32)
    score, frames = VR.viterbi(px, py, np.array([[1, 2, 1, 2], [2, 3, 1, 1]], np.int32))
    assert score.tolist() == [0.0, 0.0] and (frames == -1).all()      # empty and inverted rectangles
    px[0, :, 4] = -np.inf; px[0, :, :] = -np.inf                       # no path: frames -1
    score, frames = VR.viterbi(px, py)
    assert score[0] == -np.inf and (frames[0] == -1).all() and score[1] == 0
    px[1, 1, 2] = np.nan
    score, frames = VR.viterbi(px, py)
    assert np.isnan(score[1]) and (frames[1] == -1).all()


def test_viterbi_surface_is_exported(ft):
    assert callable(ft.mutual_information_viterbi) and callable(ft.rnnt_alignment_pruned)
    for name in ("ftr_mutual_information_viterbi_workspace_bytes", "ftr_mutual_information_viterbi_f32"):
        assert name in ft._lib.EXPORTED_SYMBOLS
    L = ft._lib.lib()
    assert L.ftr_mutual_information_viterbi_workspace_bytes(2, 3, 4) > 0
    assert L.ftr_mutual_information_viterbi_workspace_bytes(-1, 3, 4) == 0
    assert L.ftr_abi_version() == 133 and ft.__version__ == "1.2"


def test_viterbi_invalid_arguments(ft):
    L = ft._lib.lib()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    assert L.ftr_mutual_information_viterbi_f32(a, a, None, a, 1 << 20, a, a, -1, 3, 4, 0, None) == 0
    assert b"negative" in L.ftr_last_error()
    need = L.ftr_mutual_information_viterbi_workspace_bytes(2, 3, 4)
    assert L.ftr_mutual_information_viterbi_f32(a, a, None, a, need - 1, a, a, 2, 3, 4, 0, None) == 0
    assert b"too small" in L.ftr_last_error()
    assert L.ftr_mutual_information_viterbi_f32(a, a, None, None, need, a, a, 2, 3, 4, 0, None) == 0
    assert L.ftr_mutual_information_viterbi_f32(a, a, None, a, need, a, a, 2, 3, 4, 2, None) == 0
    assert L.ftr_mutual_information_viterbi_f32(None, None, None, None, 0, None, None, 0, 3, 4, 0, None) == 1   # B == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device error path")
def test_viterbi_no_cpu_fallback(ft):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ft.mutual_information_viterbi(torch.zeros(1, 2, 4), torch.zeros(1, 3, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ft.rnnt_alignment_pruned(torch.zeros(1, 3, 2, 5), torch.zeros(1, 2, dtype=torch.int32),
                                 torch.zeros(1, 3, 2, dtype=torch.int32), 4)
    L = ft._lib.lib()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    need = L.ftr_mutual_information_viterbi_workspace_bytes(1, 2, 3)
    assert L.ftr_mutual_information_viterbi_f32(a, a, None, a, need, a, a, 1, 2, 3, 0, None) == -3   # FTR_ERR_NO_DEVICE
