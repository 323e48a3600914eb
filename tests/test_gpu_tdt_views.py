"""Memory geometry of caller tensors for the five TDT functions, in the manner of tests/test_gpu_views.py (whose layouts,
data and comparison these tests reuse): views 1-3 elements into a larger buffer, permuted and sliced non-contiguous
tensors, int64 symbols / ranges / boundary.  Outputs and gradients must be the BYTES of the same call on fresh contiguous
16-byte-aligned int32 / float32 clones, and a gradient must have its input's shape."""
import functools

import pytest
import torch

from test_gpu_views import B, DEV, LAYOUTS, S, SHAPES, _data, check_all

pytestmark = pytest.mark.gpu

DURATIONS = (0, 1, 2, 3, 4)          # pruned logits: the last 5 of the C columns of test_gpu_views' logits are the duration head
JOINT_DURATIONS = (1, 2, 4)          # no zero: as many blank planes as token planes
TOKEN_MOVES, BLANK_MOVES = (0, 1, 2), (1, 2)


@pytest.fixture(autouse=True)
def _same_code_in_both_runs(monkeypatch):
    monkeypatch.setenv("FTR_GEMM_TUNE", "off")
    monkeypatch.delenv("FTR_PRUNED_ROUTE", raising=False)
    monkeypatch.delenv("FTR_BAND_IMPL", raising=False)


@functools.lru_cache(maxsize=None)
def _lattices(T):
    g = torch.Generator(device="cpu").manual_seed(31 * T)
    px = (torch.randn((B, len(TOKEN_MOVES), S, T + 1), generator=g) - 1.0).to(DEV)
    py = (torch.randn((B, len(BLANK_MOVES), S + 1, T), generator=g) - 1.0).to(DEV)
    return px, py


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("T", [33, 36])
def test_mutual_information_recursion_tdt(ft, dev, T, layout):
    px, py = _lattices(T)
    fn = lambda px, py, bd: (lambda r: (r[0], *r[1]))(
        ft.mutual_information_recursion_tdt(px, py, TOKEN_MOVES, BLANK_MOVES, bd, calc_gradients=True))
    got = check_all(fn, dict(px=px, py=py, bd=_data(T, 12)["bd"]), ("px", "py"), layout, "mutual_information_recursion_tdt")
    assert torch.isfinite(got[0]).all()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("op", ["logprobs", "loss"])
@pytest.mark.parametrize("T,C", SHAPES)
def test_tdt_pruned(ft, dev, T, C, op, layout):
    D = _data(T, C)
    ntok = C - len(DURATIONS)

    def fn(logits, sym, ranges, bd):
        if op == "logprobs":
            return ft.get_rnnt_logprobs_tdt_pruned(logits, sym, ranges, 0, DURATIONS, bd, sigma=0.05, delay_penalty=0.1)
        return ft.rnnt_loss_tdt_pruned(logits, sym, ranges, 0, DURATIONS, bd, sigma=0.05, delay_penalty=0.1, reduction="none")
    tensors = dict(logits=D["logits"], sym=D["sym"] % ntok, ranges=D["reg"]["ranges"], bd=D["bd"])
    got = check_all(fn, tensors, ("logits",), layout, f"tdt pruned {op}")
    if op == "loss":
        assert torch.isfinite(got[0]).all()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("op", ["logprobs", "loss"])
@pytest.mark.parametrize("T", [33, 36])
def test_tdt_joint(ft, dev, T, op, layout):
    D = _data(T, 12)
    ntok = D["joint"].shape[3] - len(JOINT_DURATIONS)

    def fn(logits, sym, bd):
        if op == "logprobs":
            return ft.get_rnnt_logprobs_tdt_joint(logits, sym, 0, JOINT_DURATIONS, bd, sigma=0.05)
        return ft.rnnt_loss_tdt(logits, sym, 0, JOINT_DURATIONS, bd, sigma=0.05, reduction="sum")
    check_all(fn, dict(logits=D["joint"], sym=D["sym"] % ntok, bd=D["bd"]), ("logits",), layout, f"tdt joint {op}")
