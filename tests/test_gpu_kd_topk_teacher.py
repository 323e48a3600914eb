"""rnnt_kd_topk_cache on the device against a numpy restatement of its definition: a stable argsort of the canonical float32
values (-0 = +0, NaN above +inf; ties go to the lower column) and a float64 logsumexp over the complement.  Indices and values
are exact; rest is held to 8 * 2^-24 * max(1, max|ref|), the bound the torch maker is held to.  Leading dims [2,7,3]: 42 rows.
The cases of a test run in a loop inside it, each named in the assertion that fails: the module adds four items to the suite.
The refusals need no device: tests/test_kd_topk_teacher_abi.py."""
import itertools

import numpy as np
import pytest
import torch

import kd_cases as K
import kd_topk_cases as TC

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
LEAD = (2, 7, 3)
# one quad per lane and k = C; the general form; one quad exactly full; the first with two; c3's row; eight quads; past the registers
SHAPES = [(8, 1), (8, 8), (37, 5), (256, 8), (260, 8), (500, 8), (500, 64), (2048, 8), (2052, 8)]
NAN, INF = float("nan"), float("inf")
HARD = ["five_values", "all_equal", "zeros", "nan3", "nan12", "finite4", "posinf"]


def reference(y, k, tau):
    """y float32 [..., C] -> (indices int32 [..., k], rest float64 [...])"""
    d = y.astype(np.float64) + 0.0                                              # -0 -> +0
    d = np.where(np.isnan(d), np.inf, np.clip(d, -1e300, 1e300))                # NaN above +inf
    idx = np.argsort(-d, axis=-1, kind="stable")[..., :k]
    rest = np.empty(y.shape[:-1])
    for pos in np.ndindex(*y.shape[:-1]):
        o = np.delete(y[pos].astype(np.float64), idx[pos]) / tau
        m = o.max() if o.size else -np.inf                                      # a NaN comes through the maximum
        rest[pos] = m if not np.isfinite(m) else m + np.log(np.exp(o - m).sum())
    return idx.astype(np.int32), rest


def bits(t):
    return t.cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def check(ft, dev, yt, k, tau, **kw):
    vals, idx, rest = ft.rnnt_kd_topk_cache(yt.to(dev), k, temperature=tau, **kw)
    ri, rr = reference(yt.float().numpy(), k, tau)
    case = (tuple(yt.shape), str(yt.dtype), k, tau)
    assert idx.dtype == torch.int32 and vals.dtype == yt.dtype and rest.dtype == torch.float32, case
    assert np.array_equal(idx.cpu().numpy(), ri), case
    assert torch.equal(bits(vals), bits(torch.gather(yt, -1, torch.from_numpy(ri).long()))), case       # bit for bit
    got, fin = rest.cpu().numpy().astype(np.float64), np.isfinite(rr)
    assert got.shape == rr.shape and np.array_equal(got[~fin], rr[~fin], equal_nan=True), case
    assert np.abs(got[fin] - rr[fin]).max(initial=0.0) <= 8 * 2.0 ** -24 * max(1.0, np.abs(rr[fin]).max(initial=0.0)), case
    return vals, idx, rest


def _hard_rows(kind, rng, n=5, C=260):
    y = rng.standard_normal((n, C)).astype(np.float32)
    if kind in ("five_values", "zeros"):
        y = rng.choice(np.array([-1.5, 0.0, 0.25, 2.0, 3.0] if kind == "five_values" else [0.0, -0.0], np.float32), (n, C))
    elif kind == "all_equal":
        y[:] = 0.75
    elif kind == "finite4":
        y[:, rng.permutation(C)[4:]] = -INF
    for i, row in enumerate(y):
        if kind in ("nan3", "nan12"):
            row[rng.choice(C, int(kind[3:]), replace=False)] = NAN
        elif kind == "posinf":
            row[rng.choice(C, 2 if i else 10, replace=False)] = INF   # row 0: more than k of them, rest = +inf
    return y


def test_exact_against_the_reference(ft, dev):
    for (C, k), dtype in itertools.product(SHAPES, DTYPES.values()):
        rng = np.random.default_rng(100 * C + k)
        yt = torch.from_numpy((2.0 * rng.standard_normal(LEAD + (C,))).astype(np.float32)).to(dtype)
        for tau in (1.0, 2.0):
            rest = check(ft, dev, yt, k, tau)[2]
            assert k < C or bool((rest == -INF).all()), (C, k, dtype)
        assert ft.rnnt_kd_topk_cache(yt.to(dev), k, with_rest=False)[2] is None
    for kind, dtype in itertools.product(HARD, DTYPES.values()):          # the hard rows, C = 260, k = 8
        y = _hard_rows(kind, np.random.default_rng(len(kind)))
        rest = check(ft, dev, torch.from_numpy(y).to(dtype), 8, 1.0)[2].cpu()
        want = {"nan12": torch.isnan(rest).all(), "finite4": (rest == -INF).all(), "posinf": rest[0] == INF and torch.isfinite(rest[1:]).all()}
        assert bool(want.get(kind, torch.isfinite(rest).all())), (kind, dtype)


def test_boundary_and_odd_element_base(ft, dev):
    boundary = torch.tensor([[0, 1, 5, 7], [0, 0, 5, 4]], dtype=torch.int32)
    inside = torch.zeros(LEAD[:2], dtype=torch.bool)
    inside[0, 1:7] = inside[1, 0:4] = True
    for C, dtype in itertools.product((37, 260), (torch.float32, torch.bfloat16)):
        yt = torch.from_numpy(np.random.default_rng(C).standard_normal(LEAD + (C,)).astype(np.float32)).to(dtype)
        poisoned = torch.where(inside[..., None, None], yt, torch.full_like(yt, NAN))   # a row that is read would show
        out = ft.rnnt_kd_topk_cache(poisoned.to(dev), 8, boundary=boundary.to(dev))
        fillers = (torch.zeros(8, dtype=yt.dtype), torch.arange(8, dtype=torch.int32), torch.zeros((), dtype=torch.float32))
        for got, ref, filler in zip(out, ft.rnnt_kd_topk_cache(yt.to(dev), 8), fillers):
            got = got.cpu()
            assert torch.equal(bits(got[inside]), bits(ref.cpu()[inside])), (C, dtype)
            assert torch.equal(bits(got[~inside]), bits(filler.expand_as(got[~inside]))), (C, dtype)
    yt = torch.from_numpy(np.random.default_rng(3).standard_normal(LEAD + (260,)).astype(np.float32)).to(torch.bfloat16)
    view = torch.empty(yt.numel() + 1, dtype=torch.bfloat16, device=dev)[1:].view(yt.shape)
    view.copy_(yt)
    assert view.is_contiguous() and view.data_ptr() % 4 == 2
    for got, ref in zip(ft.rnnt_kd_topk_cache(view, 8, temperature=2.0), check(ft, dev, yt, 8, 2.0)):
        assert torch.equal(bits(got), bits(ref))


def test_feeds_the_stored_teacher_loss(ft, dev):
    x, y = torch.from_numpy(TC.student(500)).to(dev), torch.from_numpy(TC.dense_teacher(500, None)).to(dev)
    ranges, boundary = torch.from_numpy(K.band_ranges()).to(dev), torch.from_numpy(K.BOUNDARY).to(dev)
    for with_rest in (False, True):
        v0, i0, r0 = ft.rnnt_kd_topk_teacher(y, 8, with_rest=with_rest)
        v1, i1, r1 = ft.rnnt_kd_topk_cache(y, 8, with_rest=with_rest, boundary=boundary)
        old = ft.rnnt_kd_loss_pruned_topk(x, v0, i0, ranges, boundary, teacher_rest=r0, reduction="none")
        new = ft.rnnt_kd_loss_pruned_topk(x, v1, i1, ranges, boundary, teacher_rest=r1, reduction="none")
        assert bool(((new - old).abs() <= 1e-4 * old.abs() + 1e-5).all()) if with_rest else torch.equal(new, old)

def test_same_bits_every_run_and_under_graph_replay(ft, dev):
    rng = np.random.default_rng(11)
    fresh = lambda: torch.from_numpy(rng.standard_normal(LEAD + (500,)).astype(np.float32)).to(torch.bfloat16).to(dev)
    static = fresh()
    same = lambda a, b: all(torch.equal(bits(p), bits(q)) for p, q in zip(a, b))
    assert same(ft.rnnt_kd_topk_cache(static, 8), ft.rnnt_kd_topk_cache(static, 8))
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        ft.rnnt_kd_topk_cache(static, 8)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ft.rnnt_kd_topk_cache(static, 8)
    for _ in range(3):
        new = fresh()
        static.copy_(new)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert same(out, ft.rnnt_kd_topk_cache(new, 8))

