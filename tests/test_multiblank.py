"""Multi-blank transducer surface without a GPU: the five ftr_*multiblank* entry points are exported and validate D, the
durations and the big-blank ids before any device check, the Python functions exist with the documented signatures and
refuse CPU tensors, and the float64 restatement the GPU tests compare against (tests/multiblank_restatement.py) agrees
with explicit path enumeration and, for D = 1, with the oracle's recursion."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from multiblank_restatement import enumerate_paths, multiblank_dp, multiblank_dp_with_grads, multiblank_logprobs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MB_SYMBOLS = ("ftr_mutual_information_multiblank_workspace_floats", "ftr_mutual_information_multiblank_fwd_f32",
              "ftr_mutual_information_multiblank_bwd_f32", "ftr_multiblank_pruned_logprobs_fwd_f32",
              "ftr_multiblank_pruned_logprobs_bwd_scaled_f32")
ENTRY_POINTS = MB_SYMBOLS[1:]


def test_multiblank_symbols_exported(ft):
    handle = ctypes.CDLL(ft._lib.LIB_PATH)
    for n in MB_SYMBOLS:
        assert hasattr(handle, n), n
        assert n in ft._lib.EXPORTED_SYMBOLS, n
    L = ft._lib.lib()
    assert L.ftr_abi_version() == 133
    # p (float64) of every cell, ans and the strip carry
    assert L.ftr_mutual_information_multiblank_workspace_floats(2, 3, 4) >= 2 * 2 * 4 * 5
    assert L.ftr_mutual_information_multiblank_workspace_floats(-1, 3, 4) == 0


def _arr(vals):
    return (ctypes.c_int32 * max(len(vals), 1))(*vals)


def _call(L, name, durations, D=None, ids=(), blank=0, C=10):
    """B=1 T=4 S=2 r=2 with null device pointers: only argument validation can answer (FTR_ERR_INVALID_ARG = 0)."""
    B, T, S, r = 1, 4, 2, 2
    D = len(durations) if D is None else D
    dur = _arr(durations) if durations is not None else None
    f = getattr(L, name)
    if name == "ftr_mutual_information_multiblank_fwd_f32":
        return f(None, None, None, dur, D, None, 0, None, B, S, T, None)
    if name == "ftr_mutual_information_multiblank_bwd_f32":
        return f(None, None, None, dur, D, None, 0, None, None, None, B, S, T, None)
    if name == "ftr_multiblank_pruned_logprobs_fwd_f32":
        return f(None, None, None, None, blank, _arr(ids), dur, D, 0.0, 0.0, None, None, None, B, T, S, C, r, None)
    return f(None, None, None, None, blank, _arr(ids), dur, D, None, None, None, None, 0, 1.0, None, B, T, S, C, r, None)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_multiblank_argument_validation_without_device(ft, name):
    L = ft._lib.lib()
    builder = "pruned_logprobs" in name
    for D in (0, 9, -1):
        assert _call(L, name, (1, 2, 3, 4, 5, 6, 7, 8, 9), D=D, ids=(1, 2, 3, 4, 5, 6, 7, 8)) == 0
        msg = L.ftr_last_error()
        assert b"multiblank" in msg and b"D = " in msg, msg
    for durs in ((1, 2, 2), (1, 4, 3), (1, 33), (0, 2), (1, -2)):
        assert _call(L, name, durs, ids=(1, 2)[:len(durs) - 1]) == 0
        assert b"durations" in L.ftr_last_error(), (durs, L.ftr_last_error())
    if not builder:
        # the recursion takes any strictly increasing durations: a valid set gets as far as the pointer checks
        assert _call(L, name, (2, 3)) == 0 and b"durations" not in L.ftr_last_error()
        return
    assert _call(L, name, (2, 3), ids=(1,)) == 0 and b"durations[0]" in L.ftr_last_error()
    for ids in ((10, 2), (-1, 2)):          # out of range
        assert _call(L, name, (1, 2, 4), ids=ids) == 0 and b"big_blank_ids[0]" in L.ftr_last_error()
    assert _call(L, name, (1, 2, 4), ids=(1, 3), blank=3) == 0
    assert b"big_blank_ids[1]" in L.ftr_last_error() and b"termination_symbol" in L.ftr_last_error()
    assert _call(L, name, (1, 2, 4), ids=(5, 5)) == 0
    assert b"big_blank_ids[1]" in L.ftr_last_error() and b"duplicate" in L.ftr_last_error()
    for blank in (-1, 10):
        assert _call(L, name, (1, 2), ids=(1,), blank=blank) == 0 and b"termination_symbol" in L.ftr_last_error()
    # a valid description gets as far as the pointer checks
    assert _call(L, name, (1, 2, 4), ids=(1, 2), blank=9) == 0 and b"null pointer" in L.ftr_last_error()
    assert _call(L, name, (1,), ids=()) == 0 and b"null pointer" in L.ftr_last_error()


def test_multiblank_signatures(ft):
    sig = lambda f: list(inspect.signature(f).parameters)
    par = lambda f: inspect.signature(f).parameters
    assert sig(ft.mutual_information_recursion_multiblank) == ["px", "py", "durations", "boundary", "calc_gradients"]
    p = par(ft.mutual_information_recursion_multiblank)
    assert p["boundary"].default is None and p["calc_gradients"].default is False
    assert sig(ft.get_rnnt_logprobs_multiblank_pruned) == ["logits", "symbols", "ranges", "termination_symbol", "big_blanks",
                                                           "boundary", "sigma"]
    assert par(ft.get_rnnt_logprobs_multiblank_pruned)["sigma"].default == 0.0
    assert sig(ft.get_rnnt_logprobs_multiblank_joint) == ["logits", "symbols", "termination_symbol", "big_blanks", "boundary",
                                                          "sigma"]
    p = par(ft.get_rnnt_logprobs_multiblank_joint)
    assert p["boundary"].default is None and p["sigma"].default == 0.0
    # the listed parameters in the listed order; `rnnt_type` follows them (only "regular" exists, anything else raises)
    assert sig(ft.rnnt_loss_multiblank_pruned)[:9] == ["logits", "symbols", "ranges", "termination_symbol", "big_blanks",
                                                       "boundary", "sigma", "delay_penalty", "reduction"]
    assert sig(ft.rnnt_loss_multiblank)[:8] == ["logits", "symbols", "termination_symbol", "big_blanks", "boundary", "sigma",
                                                "delay_penalty", "reduction"]
    for f in (ft.rnnt_loss_multiblank_pruned, ft.rnnt_loss_multiblank):
        p = par(f)
        assert p["boundary"].default is None and p["sigma"].default == 0.0 and p["delay_penalty"].default == 0.0
        assert p["reduction"].default == "mean"
        assert sig(f)[-1] == "rnnt_type" and p["rnnt_type"].default == "regular"


def test_multiblank_no_cpu_fallback(ft):
    B, T, S, C, r = 1, 4, 2, 5, 2
    logits = torch.zeros(B, T, r, C)
    joint = torch.zeros(B, T, S + 1, C)
    sym = torch.zeros(B, S, dtype=torch.int32)
    ranges = torch.zeros(B, T, r, dtype=torch.int32) + torch.arange(r, dtype=torch.int32)
    bd = torch.tensor([[0, 0, S, T]], dtype=torch.int32)
    bb = ((1, 2),)
    for call in (lambda: ft.mutual_information_recursion_multiblank(torch.zeros(B, S, T + 1), torch.zeros(B, 2, S + 1, T), (1, 2)),
                 lambda: ft.get_rnnt_logprobs_multiblank_pruned(logits, sym, ranges, C - 1, bb, bd),
                 lambda: ft.get_rnnt_logprobs_multiblank_joint(joint, sym, C - 1, bb, bd),
                 lambda: ft.rnnt_loss_multiblank_pruned(logits, sym, ranges, C - 1, bb, bd),
                 lambda: ft.rnnt_loss_multiblank_pruned(logits, sym, ranges, C - 1, (), bd),
                 lambda: ft.rnnt_loss_multiblank(joint, sym, C - 1, bb, bd)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


DURATION_SETS = [(1,), (1, 2), (1, 2, 3), (1, 4), (2, 3)]


@pytest.mark.parametrize("sub", [False, True], ids=["full", "subrect"])
@pytest.mark.parametrize("durations", DURATION_SETS, ids=str)
def test_restatement_matches_enumeration(durations, sub):
    """Every S <= 3, T <= 5 (S = 0: the log-sum over the compositions of T; T < max d included), one lattice each."""
    rng = np.random.default_rng(100 + 7 * len(durations) + durations[-1])
    D = len(durations)
    for S in range(0, 4):
        for T in range(0, 6):
            px = rng.standard_normal((1, S, T + 1))
            py = rng.standard_normal((1, D, S + 1, T))
            bd = None
            if sub:
                sb, tb = min(1, S), min(1, T)
                bd = np.array([[sb, tb, max(sb, S - 1) if S > 1 else S, max(tb, T - 1)]], dtype=np.int64)
            ans = multiblank_dp(torch.from_numpy(px), torch.from_numpy(py), durations, bd).item()
            want = enumerate_paths(px[0], py[0], durations, None if bd is None else tuple(int(v) for v in bd[0]))
            if want == float("-inf"):
                assert ans == want, (S, T)
            else:
                assert abs(ans - want) <= 1e-12 * max(1.0, abs(want)), (S, T, ans, want)


def test_restatement_counts_compositions():
    """S = 0 with all-zero weights: exp(ans) = the number of compositions of T into parts from the durations."""
    T = 5
    for durations, count in (((1,), 1), ((1, 2), 8), ((1, 2, 3), 13), ((2, 3), 2), ((1, 4), 3)):
        ans = multiblank_dp(torch.zeros(1, 0, T + 1, dtype=torch.float64), torch.zeros(1, len(durations), 1, T, dtype=torch.float64),
                            durations).item()
        assert abs(np.exp(ans) - count) < 1e-9, (durations, np.exp(ans))
    # T = 1 is not reachable with durations (2, 3): no path
    assert multiblank_dp(torch.zeros(1, 0, 2, dtype=torch.float64), torch.zeros(1, 2, 1, 1, dtype=torch.float64), (2, 3)).item() == float("-inf")


def test_restatement_d1_matches_oracle_recursion(oracle):
    d = np.load(os.path.join(ROOT, "tests", "golden", "seed1234_B2_T10_S7_C4.npz"))
    px, py, bd = d["simple_px"], d["simple_py"], d["boundary"]
    o_ans, (o_gx, o_gy) = oracle.mutual_information_recursion(px, py, bd, calc_gradients=True, dtype=np.float64)
    ans, gx, gy = multiblank_dp_with_grads(px, py[:, None], (1,), bd)
    np.testing.assert_allclose(ans, o_ans, rtol=1e-12)
    np.testing.assert_allclose(gx, o_gx, atol=1e-12)
    np.testing.assert_allclose(gy[:, 0], o_gy, atol=1e-12)


def test_restatement_builder_rows_and_masks():
    """D = 1, sigma = 0: the ordinary pruned lattice except that py is -inf from column t_end on; big blanks: the planes
    are the log-softmax columns, masked where they would overshoot."""
    rng = np.random.default_rng(3)
    B, T, S, C, r = 2, 7, 4, 6, 3
    logits = torch.from_numpy(rng.standard_normal((B, T, r, C)))
    sym = rng.integers(0, C - 1, (B, S))
    sym[0, 1] = 2                                   # a symbol that is a big blank
    s0 = np.sort(rng.integers(0, S - r + 2, (B, T)), axis=1)
    ranges = s0[..., None] + np.arange(r)
    bd = np.array([[0, 0, S, T], [0, 0, S - 1, T - 2]])
    px, py = multiblank_logprobs(logits, sym, ranges, C - 1, ((2, 2), (0, 3)), bd, sigma=0.25)
    assert tuple(px.shape) == (B, S, T + 1) and tuple(py.shape) == (B, 3, S + 1, T)
    logp = torch.log_softmax(logits, -1) - 0.25
    for b in range(B):
        te = bd[b, 3]
        for t in range(T):
            for k in range(r):
                s = ranges[b, t, k]
                for j, (i, dur) in enumerate(((C - 1, 1), (2, 2), (0, 3))):
                    want = logp[b, t, k, i].item() if t + dur <= te else float("-inf")
                    assert py[b, j, s, t].item() == want
                if s < S:
                    want = float("-inf") if (sym[b, s] in (2, 0) or t == te) else logp[b, t, k, sym[b, s]].item()
                    assert px[b, s, t].item() == want
        assert torch.isneginf(px[b, :, te]).all() and torch.isneginf(px[b, :, T]).all()
    assert torch.isneginf(px[0, 1]).all()
    # outside the band
    inband = np.zeros((B, S + 1, T), bool)
    for b in range(B):
        for t in range(T):
            inband[b, ranges[b, t], t] = True
    assert torch.isneginf(py[:, 0][torch.from_numpy(~inband)]).all()
