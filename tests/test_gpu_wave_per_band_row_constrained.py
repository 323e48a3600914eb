"""rnnt_type="constrained" on the pruned band (csrc/pruned_constrained.hip) against float64 references of the up-converted
logits: oracle.rnnt_loss_pruned_grad, and for HAT tests/hat_restatement.py through a float64 autograd DP.  Tolerances: the
1e-4 rule of tests/test_gpu_config_parity.py (losses elementwise, gradients normwise); a 16-bit gradient is rounded once by
contract, so it is compared with the float64 gradient rounded into the dtype, one unit in the last place on top."""
import numpy as np
import pytest
import torch

from tf_fast_rnnt.rnnt_loss import _apply_delay_penalty, _is_band

pytestmark = pytest.mark.gpu

TOL = 1e-4
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def _inputs(ft, dev, r, C, dtype, S=4, T=9, seed=3):
    if r == 15:        # B = 2, one utterance over the whole lattice and one over [0,0,S-1,T-3]; ranges from random occupancies
        S, T = 16, 20
    rng = np.random.default_rng(seed + 100 * r + C)
    bd = torch.tensor([[0, 0, S, T], [0, 0, S - 1, T - 3]], dtype=torch.int32, device=dev)
    occ = lambda *shape: torch.from_numpy(rng.random(shape).astype(np.float32)).to(dev)
    ranges = ft.get_rnnt_prune_ranges(occ(2, S, T), occ(2, S + 1, T), bd, r)
    logits = torch.from_numpy(rng.standard_normal((2, T, ranges.shape[2], C)).astype(np.float32)).to(dev).to(DTYPES[dtype])
    symbols = torch.from_numpy(rng.integers(0, C - 1, (2, S)).astype(np.int32)).to(dev)
    return logits, symbols, ranges, bd


def _reference(oracle, ft, hat, logits, symbols, ranges, bd, penalty):
    blank = logits.shape[-1] - 1       # -> float64 (loss [B], d sum(loss) / d logits) of the up-converted logits, numpy
    if not hat:
        loss, g = oracle.rnnt_loss_pruned_grad(logits.float().cpu().numpy(), symbols.cpu().numpy(), ranges.cpu().numpy(), blank,
                                               bd.cpu().numpy(), "constrained", penalty, "none", dtype=np.float64)
        return np.asarray(loss, np.float64), np.asarray(g, np.float64)
    from hat_restatement import get_hat_logprobs_pruned_torch, lattice_loss_torch
    x = logits.double().cpu().requires_grad_(True)
    px, py = get_hat_logprobs_pruned_torch(x, symbols.cpu(), ranges.cpu(), blank, bd.cpu(), "constrained")
    px = _apply_delay_penalty(px, bd.cpu(), "constrained", penalty)
    loss = lattice_loss_torch(px, py, bd.cpu().numpy(), "constrained")
    loss.sum().backward()
    return loss.detach().numpy(), x.grad.numpy()


def _run(fn, logits, symbols, ranges, bd, penalty):
    x = logits.clone().requires_grad_(True)
    loss = fn(x, symbols, ranges, x.shape[-1] - 1, bd, rnnt_type="constrained", delay_penalty=penalty, reduction="none")
    loss.sum().backward()
    return loss.detach(), x.grad


def _grad_distances(grads, ref64, dtype):
    slack = 0.0     # -> (distance of each gradient from the reference, distance between the first two), in units of max|ref|
    if dtype != "f32":
        ref64 = torch.from_numpy(ref64).to(DTYPES[dtype]).double().numpy()             # the one rounding
        slack = np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64) * 2.0 ** (23 - {"bf16": 7, "fp16": 10}[dtype])
        slack = np.maximum(slack, 2.0 ** -24 if dtype == "fp16" else 0.0)       # one unit in the last place (fp16: its subnormals)
    grads = [g.float().cpu().numpy().astype(np.float64) for g in grads]
    assert all(np.isfinite(g).all() for g in grads)
    excess = lambda d, n: float(np.max(np.maximum(np.abs(d) - n * slack, 0.0)) / np.abs(ref64).max())
    return [excess(g - ref64, 1) for g in grads], excess(grads[0] - grads[1], 2)


def _check(oracle, ft, monkeypatch, hat, inputs, penalty, dtype):
    fn = ft.hat_loss_pruned if hat else ft.rnnt_loss_pruned
    ref_loss, ref_grad = _reference(oracle, ft, hat, *inputs, penalty)
    loss, grad = _run(fn, *inputs, penalty)
    assert np.isfinite(ref_loss).all() and grad.dtype == inputs[0].dtype
    monkeypatch.setenv("FTR_PRUNED_ROUTE", "lattice")
    lat_loss, lat_grad = _run(fn, *inputs, penalty)
    monkeypatch.delenv("FTR_PRUNED_ROUTE")
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.abs(ref_loss)))
    d_loss, d_lat_loss = rel(loss.cpu().numpy(), ref_loss), rel(lat_loss.cpu().numpy(), ref_loss)
    (d_grad, d_lat_grad), routes_grad = _grad_distances((grad, lat_grad), ref_grad, dtype)
    print(f"loss {d_loss:.2e} (lattice route {d_lat_loss:.2e})  grad {d_grad:.2e} (lattice route {d_lat_grad:.2e})")
    assert d_loss <= TOL and d_grad <= TOL
    assert rel(loss.cpu().numpy().astype(np.float64), lat_loss.cpu().numpy()) <= 2 * max(d_loss, d_lat_loss)
    assert routes_grad <= 2 * max(d_grad, d_lat_grad)


CASES = [(r, C, dtype, p) for r in (2, 5, 15) for C in (8, 7, 260) for dtype in DTYPES for p in (0.0, 0.01)]   # C: vector form, scalar form, > 1 quad per lane
CASES.append((5, 2052, "f32", 0.01))                   # the general form beyond the register row


@pytest.mark.parametrize("r,C,dtype,penalty", CASES)
@pytest.mark.parametrize("hat", [False, True], ids=["rnnt", "hat"])
def test_loss_and_gradient_match_float64_on_both_routes(oracle, ft, dev, monkeypatch, hat, r, C, dtype, penalty):
    _check(oracle, ft, monkeypatch, hat, _inputs(ft, dev, r, C, dtype), penalty, dtype)


def test_one_band_row_has_no_symbol_move(ft, dev):
    T, C = 6, 8        # r = 1: px_band is -inf everywhere; S > 0 has no path (loss +inf, a gradient of exact zeros), S = 0 is finite
    logits = torch.randn((1, T, 1, C), device=dev, generator=torch.Generator(dev).manual_seed(1))
    ranges = torch.zeros((1, T, 1), dtype=torch.int32, device=dev)
    for S in (2, 0):
        symbols = torch.zeros((1, S), dtype=torch.int32, device=dev)
        bd = torch.tensor([[0, 0, S, T]], dtype=torch.int32, device=dev)
        loss, grad = _run(ft.rnnt_loss_pruned, logits, symbols, ranges, bd, 0.0)
        assert torch.isposinf(loss).all() and torch.equal(grad, torch.zeros_like(grad)) if S else torch.isfinite(loss).all() and torch.isfinite(grad).all()


@pytest.mark.parametrize("case", ["s_range_16", "not_a_band"])
def test_outside_the_band_route_the_composition_is_unchanged(ft, dev, case):
    if case == "s_range_16":
        logits, symbols, ranges, bd = _inputs(ft, dev, 16, 8, "f32", S=16, T=20)
    else:
        logits, symbols, ranges, bd = _inputs(ft, dev, 3, 8, "f32", S=8, T=12)
        ranges = ranges.clone()
        ranges[:, 2, 2] -= 1                             # slots 0, 1, 1 of one frame: not contiguous
        assert not _is_band(ranges, bd)
    loss, grad = _run(ft.rnnt_loss_pruned, logits, symbols, ranges, bd, 0.01)
    x = logits.clone().requires_grad_(True)
    px, py = ft.get_rnnt_logprobs_pruned(x, symbols, ranges, 7, bd, "constrained")       # what the parent computed
    px = _apply_delay_penalty(px, bd, "constrained", 0.01)
    want = -ft.mutual_information_recursion(px=px, py=py, boundary=bd)
    want.sum().backward()
    assert torch.equal(loss, want.detach()) and torch.equal(grad, x.grad)


def test_peak_memory_stays_below_one_lattice(ft, dev):
    T, S, r, C = 1500, 300, 5, 16                       # forward + backward above the inputs: less than ONE py lattice
    s0 = torch.clamp((torch.arange(T, device=dev) * (S - r + 2)) // T, max=S - r + 1).to(torch.int32)
    ranges = (s0[None, :, None] + torch.arange(r, dtype=torch.int32, device=dev)).contiguous()
    logits = torch.randn((1, T, r, C), device=dev, generator=torch.Generator(dev).manual_seed(2)).requires_grad_(True)
    symbols = torch.randint(0, C - 1, (1, S), dtype=torch.int32, device=dev)
    bd = torch.tensor([[0, 0, S, T]], dtype=torch.int32, device=dev)
    for _ in range(2):                                  # the first pass also loads the kernels and checks the ranges
        logits.grad = None
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        loss = ft.rnnt_loss_pruned(logits, symbols, ranges, C - 1, bd, rnnt_type="constrained", reduction="sum")
        loss.backward()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev) - base
    print(f"peak above the inputs {peak} bytes, one py lattice {4 * (S + 1) * T}")
    assert torch.isfinite(loss) and peak < 4 * (S + 1) * T


@pytest.mark.parametrize("r", [2, 5, 15])
def test_alignment_returns_what_the_lattice_route_returns(ft, dev, monkeypatch, r):
    logits, symbols, ranges, bd = _inputs(ft, dev, r, 8, "f32")
    score, frames = ft.rnnt_alignment_pruned(logits, symbols, ranges, 7, bd, rnnt_type="constrained")
    monkeypatch.setenv("FTR_PRUNED_ROUTE", "lattice")
    lat_score, lat_frames = ft.rnnt_alignment_pruned(logits, symbols, ranges, 7, bd, rnnt_type="constrained")
    assert torch.isfinite(score).all() and torch.equal(score, lat_score) and torch.equal(frames, lat_frames)


def test_step_replays_from_a_graph_with_the_eager_bits(ft, dev):
    from test_gpu_graph import _capture
    logits, symbols, ranges, bd = _inputs(ft, dev, 5, 260, "bf16")      # ranges from get_rnnt_prune_ranges: marked as a band
    x = logits.clone().requires_grad_(True)

    def step():
        x.grad = None
        loss = ft.rnnt_loss_pruned(x, symbols, ranges, 259, bd, rnnt_type="constrained", delay_penalty=0.01, reduction="none")
        loss.sum().backward()
        return loss.detach(), x.grad

    g, out = _capture(step)
    for seed in (5, 6):
        with torch.no_grad():
            x.copy_(torch.randn(x.shape, device=dev, generator=torch.Generator(dev).manual_seed(seed)))   # new values, same buffers
        g.replay()
        got = [v.clone() for v in out]
        assert all(torch.equal(a, b) for a, b in zip(got, step()))
