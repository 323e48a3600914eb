"""HAT loss surface without a GPU: the four ftr_hat_* entry points are exported and validate their arguments before any
device check, the four Python functions exist with the documented signatures and refuse CPU tensors, and the float64
restatement the GPU tests compare against (tests/hat_restatement.py) checks out on its own."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from hat_restatement import get_hat_logprobs_pruned_torch, hat_log_probs

HAT_SYMBOLS = ("ftr_hat_pruned_logprobs_fwd_f32", "ftr_hat_pruned_logprobs_bwd_scaled_f32",
               "ftr_hat_pruned_band_fwd_f32", "ftr_hat_pruned_band_bwd_scaled_f32")


def test_hat_symbols_exported(ft):
    handle = ctypes.CDLL(ft._lib.LIB_PATH)
    for n in HAT_SYMBOLS:
        assert hasattr(handle, n), n
        assert n in ft._lib.EXPORTED_SYMBOLS, n
    assert ft._lib.lib().ftr_abi_version() == 133


def _call(L, name, C, blank):
    """B=1 T=2 S=2 r=2 with null pointers: only argument validation can answer (FTR_ERR_INVALID_ARG = 0)."""
    B, T, S, r = 1, 2, 2, 2
    if name.endswith("_fwd_f32"):
        return getattr(L, name)(None, None, None, None, blank, 0.0, None, None, None, B, T, S, C, r, 0, None)
    return getattr(L, name)(None, None, None, None, blank, None, None, None, None, 0, 1.0, None, B, T, S, C, r, 0, None)


@pytest.mark.parametrize("name", HAT_SYMBOLS)
def test_hat_argument_validation_without_device(ft, name):
    L = ft._lib.lib()
    assert _call(L, name, 1, 0) == 0
    msg = L.ftr_last_error()
    assert b"hat_" in msg and b"C = 1" in msg
    for blank in (-1, 5):
        assert _call(L, name, 5, blank) == 0
        assert b"termination_symbol" in L.ftr_last_error()
    # the ordinary twin still accepts C = 1 up to its null-pointer check
    twin = name.replace("ftr_hat_", "ftr_")
    assert _call(L, twin, 1, 0) == 0 and b"null pointer" in L.ftr_last_error()


def test_hat_signatures(ft):
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(ft.get_hat_logprobs_pruned) == ["logits", "symbols", "ranges", "termination_symbol", "boundary", "rnnt_type"]
    assert sig(ft.get_hat_logprobs_joint) == ["logits", "symbols", "termination_symbol", "boundary", "rnnt_type"]
    assert sig(ft.hat_loss_pruned) == ["logits", "symbols", "ranges", "termination_symbol", "boundary", "rnnt_type",
                                       "delay_penalty", "reduction"]
    assert sig(ft.hat_loss) == ["logits", "symbols", "termination_symbol", "boundary", "rnnt_type", "delay_penalty",
                                "reduction"]
    p = inspect.signature(ft.hat_loss_pruned).parameters
    assert p["rnnt_type"].default == "regular" and p["delay_penalty"].default == 0.0 and p["reduction"].default == "mean"
    assert inspect.signature(ft.get_hat_logprobs_joint).parameters["boundary"].default is None


def test_hat_no_cpu_fallback(ft):
    B, T, S, C, r = 1, 4, 2, 5, 2
    logits = torch.zeros(B, T, r, C)
    joint = torch.zeros(B, T, S + 1, C)
    sym = torch.zeros(B, S, dtype=torch.int32)
    ranges = torch.zeros(B, T, r, dtype=torch.int32) + torch.arange(r, dtype=torch.int32)
    bd = torch.tensor([[0, 0, S, T]], dtype=torch.int32)
    for call in (lambda: ft.get_hat_logprobs_pruned(logits, sym, ranges, C - 1, bd),
                 lambda: ft.get_hat_logprobs_joint(joint, sym, C - 1, bd),
                 lambda: ft.hat_loss_pruned(logits, sym, ranges, C - 1, bd),
                 lambda: ft.hat_loss(joint, sym, C - 1, bd)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


@pytest.mark.parametrize("blank", [0, 3, 6])
def test_restatement_rows_normalise(blank):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 9, 7, generator=g, dtype=torch.float64) * 3
    x[0, 0, blank] = 40.0
    x[0, 1, blank] = -40.0
    lp = hat_log_probs(x, blank)
    assert torch.allclose(torch.logsumexp(lp, dim=-1), torch.zeros(4, 9, dtype=torch.float64), atol=1e-12)
    assert torch.allclose(lp[..., blank], torch.nn.functional.logsigmoid(x[..., blank]))


@pytest.mark.parametrize("rnnt_type", ["regular", "modified", "constrained"])
@pytest.mark.parametrize("blank", [0, 4, 10])
def test_restatement_matches_ordinary_builder_through_identity(oracle, rnnt_type, blank):
    """HAT log-probs of x = the ordinary log_softmax of z, where z = x except z[blank] = x[blank] + Z(x): the restatement
    against the oracle's ordinary pruned builder on z (symbols never blank)."""
    rng = np.random.default_rng(11 + blank)
    B, T, S, C, r = 3, 9, 6, 11, 3
    x = rng.standard_normal((B, T, r, C)) * 2
    others = np.array([c for c in range(C) if c != blank])
    sym = others[rng.integers(0, C - 1, (B, S))].astype(np.int32)
    s0 = np.sort(rng.integers(0, S - r + 2, (B, T)), axis=1)
    ranges = (s0[..., None] + np.arange(r)).astype(np.int32)
    bd = np.zeros((B, 4), np.int32)
    bd[:, 2] = [S, S - 1, S - 2]
    bd[:, 3] = [T, T - 2, T - 3]
    nb = np.delete(x, blank, axis=-1)
    m = nb.max(-1)
    Z = m + np.log(np.exp(nb - m[..., None]).sum(-1))
    z = x.copy()
    z[..., blank] += Z
    o_px, o_py = oracle.get_rnnt_logprobs_pruned(z.astype(np.float32), sym, ranges, blank, bd, rnnt_type)
    px, py = get_hat_logprobs_pruned_torch(torch.from_numpy(x), torch.from_numpy(sym), torch.from_numpy(ranges), blank,
                                           torch.from_numpy(bd), rnnt_type)
    px, py = px.numpy(), py.numpy()
    assert np.array_equal(np.isneginf(px), np.isneginf(o_px)) and np.array_equal(np.isneginf(py), np.isneginf(o_py))
    fin = np.isfinite(o_px)
    np.testing.assert_allclose(px[fin], o_px[fin], rtol=1e-5, atol=2e-5)
    fin = np.isfinite(o_py)
    np.testing.assert_allclose(py[fin], o_py[fin], rtol=1e-5, atol=2e-5)
