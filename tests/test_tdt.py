"""TDT (token-and-duration transducer) surface without a GPU: the five ftr_*tdt* entry points are exported and validate the
duration lists and sigma before any device check, the Python functions exist with the documented signatures and refuse CPU
tensors, and the float64 restatement the GPU tests compare against (tests/tdt_restatement.py) agrees with explicit path
enumeration, with the multi-blank restatement for token_durations = (0,), with the oracle's recursion for (0,)/(1,), and
with a hand-computed row set."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

from multiblank_restatement import multiblank_dp
from tdt_restatement import enumerate_paths, tdt_dp, tdt_dp_with_grads, tdt_logprobs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDT_SYMBOLS = ("ftr_mutual_information_tdt_workspace_floats", "ftr_mutual_information_tdt_fwd_f32",
               "ftr_mutual_information_tdt_bwd_f32", "ftr_tdt_pruned_logprobs_fwd_f32",
               "ftr_tdt_pruned_logprobs_bwd_scaled_f32")
NEG = float("-inf")


def test_tdt_symbols_exported(ft):
    handle = ctypes.CDLL(ft._lib.LIB_PATH)
    for n in TDT_SYMBOLS:
        assert hasattr(handle, n), n
        assert n in ft._lib.EXPORTED_SYMBOLS, n
    L = ft._lib.lib()
    assert L.ftr_abi_version() == 133 and L.ftr_package_version() == b"1.2"
    # p (float64) of every cell, ans and the strip carry
    assert L.ftr_mutual_information_tdt_workspace_floats(2, 3, 4) >= 2 * 2 * 4 * 5
    assert L.ftr_mutual_information_tdt_workspace_floats(-1, 3, 4) == 0


def _arr(vals):
    return (ctypes.c_int32 * max(len(vals), 1))(*vals)


def _recursion(L, name, tok, blk, Dx=None, Dy=None):
    """B=1 T=4 S=2 with null device pointers: only argument validation can answer (FTR_ERR_INVALID_ARG = 0)."""
    Dx = len(tok) if Dx is None else Dx
    Dy = len(blk) if Dy is None else Dy
    if name.endswith("fwd_f32"):
        return getattr(L, name)(None, None, None, _arr(tok), Dx, _arr(blk), Dy, None, 0, None, 1, 2, 4, None)
    return getattr(L, name)(None, None, None, _arr(tok), Dx, _arr(blk), Dy, None, 0, None, None, None, 1, 2, 4, None)


def _builder(L, name, durs, N=None, sigma=0.0, blank=0, C=10):
    N = len(durs) if N is None else N
    if name.endswith("fwd_f32"):
        return getattr(L, name)(None, None, None, None, blank, _arr(durs), N, sigma, 0.0, None, None, None, None, 1, 4, 2, C, 2, None)
    return getattr(L, name)(None, None, None, None, blank, _arr(durs), N, sigma, 0.0, None, None, None, None, None, 0, 1.0,
                            None, 1, 4, 2, C, 2, None)


@pytest.mark.parametrize("name", TDT_SYMBOLS[1:3])
def test_tdt_recursion_argument_validation_without_device(ft, name):
    L = ft._lib.lib()
    err = lambda: L.ftr_last_error()
    for tok in ((), (0, 0), (2, 1), (-1,), (17,), (0, 1, 1)):
        assert _recursion(L, name, tok, (1,)) == 0 and b"token_durations" in err(), (tok, err())
    for blk in ((), (0,), (0, 1), (1, 1), (3, 2), (17,), (1, -2)):
        assert _recursion(L, name, (0,), blk) == 0 and b"blank_durations" in err(), (blk, err())
    assert _recursion(L, name, (0,), (1,), Dx=-1) == 0 and b"token_durations" in err()
    assert _recursion(L, name, (0,), (1,), Dy=0) == 0 and b"blank_durations" in err()
    assert _recursion(L, name, (0, 1, 2, 3, 4, 5), (1, 2, 3, 4, 5)) == 0 and b"Dx + Dy" in err()    # 11 moves
    # valid descriptions (9 moves and 10, five of each kind, among them) get as far as the size / pointer checks
    for tok, blk in (((0, 1, 2, 3, 4), (1, 2, 3, 4)), ((0, 1, 2, 3, 4), (1, 2, 3, 4, 5)), ((1, 2, 3, 4, 8), (1, 2, 3, 4, 8)),
                     ((0,), (1, 2, 3, 4, 5, 6, 7, 8)), ((0, 16), (3, 16)), ((1, 2), (1,))):
        assert _recursion(L, name, tok, blk) == 0
        assert b"durations" not in err() and (b"workspace" in err() or b"null" in err()), err()


@pytest.mark.parametrize("name", TDT_SYMBOLS[3:])
def test_tdt_builder_argument_validation_without_device(ft, name):
    L = ft._lib.lib()
    err = lambda: L.ftr_last_error()
    for durs in ((), (0, 1, 2, 3, 4, 5), (0, 0), (2, 1), (-1, 1), (0, 17)):
        assert _builder(L, name, durs) == 0 and b"durations" in err(), (durs, err())
    assert _builder(L, name, (0,)) == 0 and b"durations" in err() and b"positive" in err()
    assert _builder(L, name, (0, 1), sigma=-0.5) == 0 and b"sigma" in err()
    for blank in (-1, 10):
        assert _builder(L, name, (0, 1), blank=blank) == 0 and b"termination_symbol" in err()
    for durs in ((0, 1), (1,), (0, 1, 2, 3, 4), (2, 16)):
        assert _builder(L, name, durs, sigma=0.05) == 0 and b"null pointer" in err(), (durs, err())


def test_tdt_signatures(ft):
    sig = lambda f: list(inspect.signature(f).parameters)
    par = lambda f: inspect.signature(f).parameters
    assert sig(ft.mutual_information_recursion_tdt) == ["px", "py", "token_durations", "blank_durations", "boundary",
                                                        "calc_gradients"]
    p = par(ft.mutual_information_recursion_tdt)
    assert p["boundary"].default is None and p["calc_gradients"].default is False
    assert sig(ft.get_rnnt_logprobs_tdt_pruned) == ["logits", "symbols", "ranges", "termination_symbol", "durations", "boundary",
                                                    "sigma", "delay_penalty"]
    assert sig(ft.get_rnnt_logprobs_tdt_joint)[:5] == ["logits", "symbols", "termination_symbol", "durations", "boundary"]
    assert par(ft.get_rnnt_logprobs_tdt_joint)["boundary"].default is None
    assert sig(ft.rnnt_loss_tdt_pruned) == ["logits", "symbols", "ranges", "termination_symbol", "durations", "boundary", "sigma",
                                            "rnnt_type", "delay_penalty", "reduction"]
    assert sig(ft.rnnt_loss_tdt)[:5] == ["logits", "symbols", "termination_symbol", "durations", "boundary"]
    for f in (ft.get_rnnt_logprobs_tdt_pruned, ft.get_rnnt_logprobs_tdt_joint, ft.rnnt_loss_tdt_pruned, ft.rnnt_loss_tdt):
        assert par(f)["sigma"].default == 0.0 and par(f)["delay_penalty"].default == 0.0
    for f in (ft.rnnt_loss_tdt_pruned, ft.rnnt_loss_tdt):
        p = par(f)
        assert p["boundary"].default is None and p["rnnt_type"].default == "regular" and p["reduction"].default == "mean"
    assert "0 and 1" in ft.rnnt_loss_tdt_pruned.__doc__          # when ranges of the simple loss guarantee a path


def test_tdt_no_cpu_fallback(ft):
    B, T, S, C, r, durs = 1, 4, 2, 5, 2, (0, 1, 2)
    logits = torch.zeros(B, T, r, C + 3)
    joint = torch.zeros(B, T, S + 1, C + 3)
    sym = torch.zeros(B, S, dtype=torch.int32)
    ranges = torch.zeros(B, T, r, dtype=torch.int32) + torch.arange(r, dtype=torch.int32)
    bd = torch.tensor([[0, 0, S, T]], dtype=torch.int32)
    for call in (lambda: ft.mutual_information_recursion_tdt(torch.zeros(B, 3, S, T + 1), torch.zeros(B, 2, S + 1, T), durs, (1, 2)),
                 lambda: ft.get_rnnt_logprobs_tdt_pruned(logits, sym, ranges, C - 1, durs, bd),
                 lambda: ft.get_rnnt_logprobs_tdt_joint(joint, sym, C - 1, durs, bd),
                 lambda: ft.rnnt_loss_tdt_pruned(logits, sym, ranges, C - 1, durs, bd),
                 lambda: ft.rnnt_loss_tdt(joint, sym, C - 1, durs, bd)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


MOVE_SETS = [((0, 1, 2), (1, 2)), ((1, 2), (1,)), ((0,), (1, 3))]


@pytest.mark.parametrize("sub", [False, True], ids=["full", "subrect"])
@pytest.mark.parametrize("moves", MOVE_SETS, ids=str)
def test_restatement_matches_enumeration(moves, sub):
    """Every S <= 3, T <= 5, one lattice each (T smaller than a duration and lattices without any path included)."""
    tok, blk = moves
    rng = np.random.default_rng(200 + 7 * len(tok) + blk[-1])
    for S in range(0, 4):
        for T in range(0, 6):
            px = rng.standard_normal((1, len(tok), S, T + 1))
            py = rng.standard_normal((1, len(blk), S + 1, T))
            bd = None
            if sub:
                sb, tb = min(1, S), min(1, T)
                bd = np.array([[sb, tb, max(sb, S - 1) if S > 1 else S, max(tb, T - 1)]], dtype=np.int64)
            ans = tdt_dp(torch.from_numpy(px), torch.from_numpy(py), tok, blk, bd).item()
            want = enumerate_paths(px[0], py[0], tok, blk, None if bd is None else tuple(int(v) for v in bd[0]))
            if want == NEG:
                assert ans == want, (S, T)
            else:
                assert abs(ans - want) <= 1e-12 * max(1.0, abs(want)), (S, T, ans, want)


def test_restatement_counts_paths_and_rectangles():
    """All-zero weights: exp(ans) counts the paths.  S = 1, T = 2, token durations (0,1), blank (1,): the symbol leaves
    at frame 0, 1 or 2 with duration 0 (3 paths) or at frame 0 or 1 with duration 1 (2 paths)."""
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    assert abs(math.exp(tdt_dp(z(1, 2, 1, 3), z(1, 1, 2, 2), (0, 1), (1,)).item()) - 5) < 1e-9
    # no token move fits: S = 1 needs a frame skip of 2 or 3, T = 1 has none; and T = 1 is not reachable by blanks of 2
    assert tdt_dp(z(1, 2, 1, 2), z(1, 1, 2, 1), (2, 3), (1,)).item() == NEG
    assert tdt_dp(z(1, 1, 0, 2), z(1, 1, 1, 1), (0,), (2,)).item() == NEG
    # an inverted rectangle answers 0
    assert tdt_dp(z(1, 1, 2, 4), z(1, 1, 3, 3), (0,), (1,), np.array([[2, 0, 1, 3]])).item() == 0.0


@pytest.mark.parametrize("durations", [(1,), (1, 2, 4), (2, 3)], ids=str)
def test_restatement_token_duration_zero_is_the_multiblank_restatement(durations):
    rng = np.random.default_rng(5)
    B, S, T = 2, 4, 9
    px = torch.from_numpy(rng.standard_normal((B, S, T + 1))).requires_grad_(True)
    py = torch.from_numpy(rng.standard_normal((B, len(durations), S + 1, T))).requires_grad_(True)
    bd = np.array([[0, 0, S, T], [1, 1, S - 1, T - 2]])
    a = tdt_dp(px[:, None], py, (0,), durations, bd)
    b = multiblank_dp(px, py, durations, bd)
    assert torch.equal(torch.isneginf(a), torch.isneginf(b))
    fin = torch.isfinite(b)
    np.testing.assert_allclose(a[fin].detach().numpy(), b[fin].detach().numpy(), rtol=1e-13)
    if fin.any():
        ga = torch.autograd.grad(a[fin].sum(), (px, py))
        gb = torch.autograd.grad(b[fin].sum(), (px, py))
        for u, v in zip(ga, gb):
            np.testing.assert_allclose(u.numpy(), v.numpy(), atol=1e-13)


def test_restatement_0_1_matches_oracle_recursion(oracle):
    d = np.load(os.path.join(ROOT, "tests", "golden", "seed1234_B2_T10_S7_C4.npz"))
    px, py, bd = d["simple_px"], d["simple_py"], d["boundary"]
    o_ans, (o_gx, o_gy) = oracle.mutual_information_recursion(px, py, bd, calc_gradients=True, dtype=np.float64)
    ans, gx, gy = tdt_dp_with_grads(px[:, None], py[:, None], (0,), (1,), bd)
    np.testing.assert_allclose(ans, o_ans, rtol=1e-12)
    np.testing.assert_allclose(gx[:, 0], o_gx, atol=1e-12)
    np.testing.assert_allclose(gy[:, 0], o_gy, atol=1e-12)


def test_restatement_builder_by_hand():
    """B = 1, T = 2 frames, S = 1 symbol, r = 2 (the whole lattice), C = 2 tokens (blank = 0, the symbol = 1), durations
    (0, 1, 2), sigma = 0.5.  Token logits (0, ln 3) -> softmax (1/4, 3/4); duration logits (0, 0, ln 2) -> (1/4, 1/4, 1/2),
    the same in all four rows, so every entry is one of a handful of logs."""
    row = [0.0, math.log(3.0), 0.0, 0.0, math.log(2.0)]
    logits = torch.tensor(row, dtype=torch.float64).expand(1, 2, 2, 5).contiguous()
    ranges = np.array([[[0, 1], [0, 1]]])
    sigma = 0.5
    tok_sym, tok_blank = math.log(0.75) - sigma, math.log(0.25) - sigma
    dur = [math.log(0.25), math.log(0.25), math.log(0.5)]
    px, py = tdt_logprobs(logits, np.array([[1]]), ranges, 0, (0, 1, 2), None, sigma=sigma)
    assert tuple(px.shape) == (1, 3, 1, 3) and tuple(py.shape) == (1, 2, 2, 2)
    # px[i, s=0, t]: t_end = 2; column 2 is -inf, and t + e_i > 2 masks (e=2, t=1)
    want_px = [[tok_sym + dur[0], tok_sym + dur[0], NEG],
               [tok_sym + dur[1], tok_sym + dur[1], NEG],
               [tok_sym + dur[2], NEG, NEG]]
    np.testing.assert_allclose(px[0, :, 0].numpy(), np.array(want_px), rtol=1e-14)
    # py[j, s, t] with blank durations (1, 2) = duration columns 1 and 2; (d=2, t=1) overshoots
    for s in range(2):
        np.testing.assert_allclose(py[0, :, s].numpy(), np.array([[tok_blank + dur[1], tok_blank + dur[1]],
                                                                  [tok_blank + dur[2], NEG]]), rtol=1e-14)
    # t_end = 1 by boundary: frame 1 is column t_end for px and lies beyond every blank move
    px, py = tdt_logprobs(logits, np.array([[1]]), ranges, 0, (0, 1, 2), np.array([[0, 0, 1, 1]]), sigma=sigma, delay_penalty=0.25)
    pen0 = (0.0 - 0.0) * 0.25                                    # offset = (t_end - 1) / 2 = 0, source frame 0
    np.testing.assert_allclose(px[0, :, 0].numpy(), np.array([[tok_sym + dur[0] + pen0, NEG, NEG],
                                                              [tok_sym + dur[1] + pen0, NEG, NEG],
                                                              [NEG, NEG, NEG]]), rtol=1e-14)
    np.testing.assert_allclose(py[0, :, 0].numpy(), np.array([[tok_blank + dur[1], NEG], [NEG, NEG]]), rtol=1e-14)
    # the loss of this lattice by hand: paths from (0,0) to (1,1): symbol e=0 at t=0 then blank 1; blank 1 then symbol
    # e=0 at t=1 is column t_end (-inf); symbol e=1 from t=0 lands on (1,1)
    ans = tdt_dp(px, py, (0, 1, 2), (1, 2), np.array([[0, 0, 1, 1]])).item()
    want = math.log(math.exp(tok_sym + dur[0] + tok_blank + dur[1]) + math.exp(tok_sym + dur[1]))
    assert abs(ans - want) < 1e-13
