"""Best-path (Viterbi) alignment on the device (csrc/mi_viterbi.hip): bit-exact against the float32 restatement
(tests/viterbi_restatement.py) in score and frames, properties that do not depend on the restatement, the pruned
wrapper, and graph capture."""
import numpy as np
import pytest
import torch

import viterbi_restatement as VR

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.asarray(x, np.float32).view(np.int32)


def _check(ft, dev, px, py, bd):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    score, frames = ft.mutual_information_viterbi(t(px), t(py), None if bd is None else t(bd))
    torch.cuda.synchronize()
    score, frames = score.cpu().numpy(), frames.cpu().numpy()
    want_s, want_f = VR.viterbi(px, py, bd)
    assert np.array_equal(_bits(score), _bits(want_s)), (score, want_s)
    for b in range(px.shape[0]):
        assert np.array_equal(frames[b], want_f[b]), (b, np.nonzero(frames[b] != want_f[b])[0][:10])
    return score, frames


def _resum(px, py, score, frames, sb=0, tb=0, se=None, te=None):
    """Sums px / py along the path given by frames, left to right in float32."""
    B, S, T1 = px.shape
    T = py.shape[2]
    modified = T1 == T
    for b in range(B):
        s, t = sb, tb
        e_s = S if se is None else se
        e_t = T if te is None else te
        acc = np.float32(0)
        while s < e_s or t < e_t:
            if s < e_s and frames[b, s] == t:
                acc = np.float32(acc + px[b, s, t]); s += 1; t += 1 if modified else 0
            else:
                acc = np.float32(acc + py[b, s, t]); t += 1
        assert s == e_s and t == e_t
        assert _bits(acc) == _bits(score[b]), (b, acc, score[b])


@pytest.mark.parametrize("modified", [False, True])
@pytest.mark.parametrize("T", [1, 2, 100, 3000])
@pytest.mark.parametrize("S1", [1, 2, 63, 64, 65, 1023, 1024, 1025, 1100])
def test_viterbi_bit_exact(ft, dev, S1, T, modified):
    """Four utterances: normal values with the full rectangle, normal values with a ragged one (s_begin / t_begin > 0),
    integer values (ties everywhere) with the full rectangle and with a ragged one."""
    S = S1 - 1
    T1 = T if modified else T + 1
    rng = np.random.default_rng(S1 * 7919 + T * 31 + modified)
    px = rng.standard_normal((4, S, T1)).astype(np.float32)
    py = rng.standard_normal((4, S1, T)).astype(np.float32)
    px[2:] = rng.integers(-2, 1, (2, S, T1)).astype(np.float32)
    py[2:] = rng.integers(-2, 1, (2, S1, T)).astype(np.float32)
    bd = np.zeros((4, 4), np.int32); bd[:, 2] = S; bd[:, 3] = T
    for b in (1, 3):
        sb, tb = min(S, S // 7 + 1), min(T, T // 9 + 1)
        se = max(sb, S - S // 5)
        te = max(tb, T - T // 6)
        if modified:
            te = max(te, min(T, tb + (se - sb)))      # a modified path needs te - tb >= se - sb
        bd[b] = (sb, tb, se, te)
    _check(ft, dev, px, py, bd)
    _check(ft, dev, px, py, None)


@pytest.mark.parametrize("modified", [False, True])
def test_viterbi_edges_nan_and_empty(ft, dev, modified):
    S, T = 70, 90
    T1 = T if modified else T + 1
    rng = np.random.default_rng(3)
    px = rng.standard_normal((6, S, T1)).astype(np.float32)
    py = rng.standard_normal((6, S + 1, T)).astype(np.float32)
    bd = np.array([[0, 0, S, T], [5, 7, 5, 7], [9, 4, 3, 50], [2, 3, 60, 1], [0, 0, S, T], [10, 10, 60, 80]], np.int32)
    px[4, 30, 40] = np.nan                    # NaN inside one rectangle: score NaN, frames -1
    py[5, 70, 20] = np.nan                    # NaN outside utterance 5's rectangle: no effect
    score, frames = _check(ft, dev, px, py, bd)
    assert score[1] == 0 and (frames[1] == -1).all()            # empty rectangle
    assert score[2] == 0 and score[3] == 0 and (frames[2:4] == -1).all()   # inverted ones
    assert np.isnan(score[4]) and (frames[4] == -1).all()
    assert np.isfinite(score[5])
    # B == 0 and S == 0
    e = ft.mutual_information_viterbi(torch.zeros((0, 3, T1), device=dev), torch.zeros((0, 4, T), device=dev))
    assert e[0].shape == (0,) and e[1].shape == (0, 3)
    py0 = rng.standard_normal((2, 1, T)).astype(np.float32)
    s0, f0 = ft.mutual_information_viterbi(torch.zeros((2, 0, T1), device=dev), torch.from_numpy(py0).to(dev))
    acc = np.zeros(2, np.float32)
    for t in range(T):
        acc = (acc + py0[:, 0, t]).astype(np.float32)
    assert f0.shape == (2, 0) and np.array_equal(_bits(s0.cpu().numpy()), _bits(acc))


def test_viterbi_inf_patterns_of_the_builders(ft, dev):
    """-inf in px[:, :, T] (regular get_rnnt_logprobs) and outside the band (pruned builder)."""
    torch.manual_seed(0)
    B, T, S, C, r = 3, 120, 30, 17, 4
    am = torch.randn(B, T, C, device=dev); lm = torch.randn(B, S + 1, C, device=dev)
    sym = torch.randint(0, C - 1, (B, S), device=dev, dtype=torch.int32)
    bd = torch.tensor([[0, 0, S, T], [0, 0, S - 4, T - 20], [0, 0, S - 9, T - 7]], dtype=torch.int32, device=dev)
    for rt in ("regular", "modified"):
        px, py = ft.get_rnnt_logprobs(lm, am, sym, C - 1, rnnt_type=rt, boundary=bd)
        _check(ft, dev, px.cpu().numpy(), py.cpu().numpy(), bd.cpu().numpy())
        _, (gx, gy) = ft.rnnt_loss_simple(lm, am, sym, C - 1, bd, rnnt_type=rt, reduction="none", calc_gradients=True)
        ranges = ft.get_rnnt_prune_ranges(gx, gy, bd, r)
        logits = torch.randn(B, T, r, C, device=dev)
        ppx, ppy = ft.get_rnnt_logprobs_pruned(logits, sym, ranges, C - 1, bd, rnnt_type=rt)
        _check(ft, dev, ppx.cpu().numpy(), ppy.cpu().numpy(), bd.cpu().numpy())


@pytest.mark.parametrize("config", ["c3", "c5"])
@pytest.mark.parametrize("rnnt_type", ["regular", "modified"])
def test_viterbi_baseline_lattices(ft, dev, config, rnnt_type):
    from bench import CONFIGS, make_inputs
    B, T, S, C, _ = CONFIGS[config]
    inp = make_inputs(B, T, S, C, seed=1000, device=dev)
    px, py = ft.get_rnnt_logprobs(inp["lm"], inp["am"], inp["symbols"], inp["blank"], rnnt_type=rnnt_type, boundary=inp["boundary"])
    pxn, pyn = px.cpu().numpy(), py.cpu().numpy()
    score, frames = _check(ft, dev, pxn, pyn, inp["boundary"].cpu().numpy())
    _resum(pxn, pyn, score, frames)
    ans = ft.mutual_information_recursion(px, py, inp["boundary"]).cpu().numpy()
    assert (score <= ans + 1e-4 * np.abs(ans)).all()


@pytest.mark.parametrize("modified", [False, True])
def test_viterbi_properties(ft, dev, modified):
    """Independent of the restatement: the frames are a path whose float32 sum is the score; the score is at most the
    log-sum over all paths; repeated calls are bit-identical."""
    B, S, T = 4, 150, 700
    T1 = T if modified else T + 1
    rng = np.random.default_rng(17)
    px = (rng.standard_normal((B, S, T1)) - 1).astype(np.float32)
    py = (rng.standard_normal((B, S + 1, T)) - 1).astype(np.float32)
    tpx, tpy = torch.from_numpy(px).to(dev), torch.from_numpy(py).to(dev)
    s1, f1 = ft.mutual_information_viterbi(tpx, tpy)
    s2, f2 = ft.mutual_information_viterbi(tpx.clone().requires_grad_(True), tpy)
    assert not s2.requires_grad and not f2.requires_grad
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32)) and torch.equal(f1, f2)
    score, frames = s1.cpu().numpy(), f1.cpu().numpy()
    _resum(px, py, score, frames)
    d = np.diff(frames, axis=1)
    assert (d > 0).all() if modified else (d >= 0).all()
    ans = ft.mutual_information_recursion(tpx, tpy).cpu().numpy()
    assert (score <= ans + 1e-4 * np.abs(ans)).all()


def test_viterbi_recovers_a_planted_alignment(ft, dev):
    """The sharp lattice of test_gpu_mi.py: px ~ -0.1 / py ~ -0.05 on a planted alignment, -10 / -3 off it."""
    B, S, T = 2, 200, 1000
    rng = np.random.default_rng(5)
    px = (rng.standard_normal((B, S, T + 1)) - 10.0).astype(np.float32)
    py = (rng.standard_normal((B, S + 1, T)) - 3.0).astype(np.float32)
    planted = np.zeros((B, S), np.int32)
    for b in range(B):
        ts = np.sort(np.clip(np.round((np.arange(S) + 0.5) * T / S).astype(int) + rng.integers(-3, 4, S), 0, T - 1))
        prev = 0
        for s_ in range(S + 1):
            end = ts[s_] if s_ < S else T
            py[b, s_, prev:end] = -0.05
            if s_ < S:
                px[b, s_, end] = -0.1
            prev = end
        planted[b] = ts
    px[:, :, T] = -np.inf
    score, frames = _check(ft, dev, px, py, None)
    assert np.array_equal(frames, planted)


@pytest.mark.parametrize("rnnt_type", ["regular", "modified", "constrained"])
def test_rnnt_alignment_pruned(ft, dev, rnnt_type):
    torch.manual_seed(1)
    B, T, S, C, r = 4, 300, 60, 33, 5
    am = torch.randn(B, T, C, device=dev); lm = torch.randn(B, S + 1, C, device=dev)
    sym = torch.randint(0, C - 1, (B, S), device=dev, dtype=torch.int32)
    bd = torch.tensor([[0, 0, S, T], [0, 0, S - 10, T - 40], [0, 0, S, T - 100], [0, 0, S - 30, T]], dtype=torch.int32, device=dev)
    _, (gx, gy) = ft.rnnt_loss_simple(lm, am, sym, C - 1, bd, rnnt_type=rnnt_type, reduction="none", calc_gradients=True)
    ranges = ft.get_rnnt_prune_ranges(gx, gy, bd, r)
    logits = torch.randn(B, T, r, C, device=dev, requires_grad=True)
    score, frames = ft.rnnt_alignment_pruned(logits, sym, ranges, C - 1, bd, rnnt_type=rnnt_type)
    assert not score.requires_grad
    s2, f2 = ft.mutual_information_viterbi(*ft.get_rnnt_logprobs_pruned(logits, sym, ranges, C - 1, bd, rnnt_type=rnnt_type), bd)
    assert torch.equal(score.view(torch.int32), s2.view(torch.int32)) and torch.equal(frames, f2)
    fr, rg, bdn = frames.cpu().numpy(), ranges.cpu().numpy(), bd.cpu().numpy()
    assert np.isfinite(score.cpu().numpy()).all()
    for b in range(B):
        for s in range(bdn[b, 2]):
            t = fr[b, s]
            assert 0 <= t <= bdn[b, 3]
            if t < T:
                assert rg[b, t, 0] <= s <= rg[b, t, -1], (b, s, t, rg[b, t])
        assert (fr[b, bdn[b, 2]:] == -1).all()


def test_viterbi_graph_capture(ft, dev):
    """Both functions captured into one graph; three replays with fresh inputs copied into the static tensors each
    equal an eager run (kernels only: no memset / memcpy nodes)."""
    torch.manual_seed(2)
    B, T, S, C, r = 3, 1200, 1100, 9, 4
    px = torch.randn(B, S, T + 1, device=dev); py = torch.randn(B, S + 1, T, device=dev)
    logits = torch.randn(B, T, r, C, device=dev)
    sym = torch.randint(0, C - 1, (B, S), device=dev, dtype=torch.int32)
    start = torch.clamp((torch.arange(T, device=dev) * S) // T - 1, min=0).clamp(max=S + 1 - r)
    ranges = (start[None, :, None] + torch.arange(r, device=dev)[None, None, :]).expand(B, T, r).to(torch.int32).contiguous()
    bd = torch.tensor([[0, 0, S, T]] * B, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            ft.mutual_information_viterbi(px, py, bd); ft.rnnt_alignment_pruned(logits, sym, ranges, C - 1, bd)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out1 = ft.mutual_information_viterbi(px, py, bd)
        out2 = ft.rnnt_alignment_pruned(logits, sym, ranges, C - 1, bd)
    for i in range(3):
        px.copy_(torch.randn_like(px)); py.copy_(torch.randn_like(py)); logits.copy_(torch.randn_like(logits))
        g.replay()
        torch.cuda.synchronize()
        e1 = ft.mutual_information_viterbi(px, py, bd)
        e2 = ft.rnnt_alignment_pruned(logits, sym, ranges, C - 1, bd)
        torch.cuda.synchronize()
        for a, b in ((out1, e1), (out2, e2)):
            assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), i
            assert torch.equal(a[1], b[1]), i
