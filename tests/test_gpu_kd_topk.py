"""rnnt_kd_loss_pruned_topk on the device: distillation on the pruned band from a stored top-K teacher on the teacher's own
band, against the float64 restatement of its definition (tests/kd_topk_restatement.py) on the up-converted values.

Geometry and inputs: tests/kd_topk_cases.py (B=2 T=12 S=5 r=3 of tests/kd_cases.py; a teacher band of r_t = 2 or 4 rows that
is shifted against the student's by -1, 0, 1, 2 rows from frame to frame, or the student's own ranges).  (C, K) crosses every
path of the kernels: (8, 1); (8, 8) every column stored, no rest; (37, 5) the element path; (500, 8); (500, 64) one entry
on every lane; (2048, 8) the largest register-resident row; (2056, 8) the two-pass form over two stretches of the slot table.

Tolerances, those of tests/test_gpu_kd.py taken over unchanged, none of them measured from the code under test:
  loss      |err| <= 1e-4 |ref| + 1e-5 per utterance
  gradient  |g - g64| <= u |g64| + a + 1e-4 max|g64|, (u, a) = (0, 0) float32, (2^-8, 0) bfloat16, (2^-11, 2^-25) float16;
            rows of nodes that are not distilled are exactly 0
With FTR_KD_TOPK_PARITY_OUT set, the largest errors seen are written there as JSON when the module is done."""
import json
import os

import numpy as np
import pytest
import torch

import kd_cases as K
import kd_restatement as R
import kd_topk_cases as TC
import kd_topk_restatement as TR

pytestmark = pytest.mark.gpu

DT = {"f32": (torch.float32, 0.0, 0.0), "bf16": (torch.bfloat16, 2.0 ** -8, 0.0), "fp16": (torch.float16, 2.0 ** -11, 2.0 ** -25)}
PAIRS = [("f32", "f32"), ("bf16", "bf16"), ("fp16", "fp16"), ("f32", "bf16"), ("bf16", "f32")]   # (student, teacher values)
SHAPES = [(8, 1), (8, 8), (37, 5), (500, 8), (500, 64), (2048, 8), (2056, 8)]
_WORST = {}


def _parity_cases():
    """(C, K, rest, tau, r_t, student dtype, values dtype): every shape with the rest on and off (K = C: off), tau 1 and 2,
    r_t 2, 4 and None; the dtype pairs go round, so every pair meets every kind of path"""
    out, i = [], 0
    for C, k in SHAPES:
        combos = ([(False, 1.0, 2), (False, 2.0, 4), (False, 1.0, None)] if k == C else
                  [(True, 1.0, 2), (False, 2.0, 4), (True, 2.0, None), (False, 1.0, None), (True, 1.0, 4)])
        for rest, tau, rt in combos:
            out.append((C, k, rest, tau, rt) + PAIRS[i % len(PAIRS)])
            i += 1
    return out


CASES = _parity_cases()
assert {c[5:] for c in CASES} == set(PAIRS) and {c[2] for c in CASES} == {True, False}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("FTR_KD_TOPK_PARITY_OUT")
    if path and _WORST:
        with open(path, "w") as f:
            json.dump({k: _WORST[k] for k in sorted(_WORST)}, f, indent=1)
            f.write("\n")


def _note(key, **vals):
    rec = _WORST.setdefault(key, {})
    for k, v in vals.items():
        rec[k] = max(rec.get(k, 0.0), float(v))


_INPUTS, _REFS = {}, {}


def inputs(C, k, rest, tau, rt, sdt, tdt):
    """(student, values, indices, rest | None): cpu tensors, the student and the values rounded to their dtypes (the cache is
    the top-K of the ROUNDED dense teacher, its rest the float64 logsumexp of the other rounded columns); cached, never modified"""
    key = (C, k, rest, tau, rt, sdt, tdt)
    if key not in _INPUTS:
        y = torch.from_numpy(TC.dense_teacher(C, rt)).to(DT[tdt][0]).float().numpy()
        vals, idx, rs = TC.topk_cache(y, k, tau, rest)
        _INPUTS[key] = (torch.from_numpy(TC.student(C)).to(DT[sdt][0]), torch.from_numpy(vals).to(DT[tdt][0]), torch.from_numpy(idx),
                        None if rs is None else torch.from_numpy(rs))
        assert torch.equal(_INPUTS[key][1].float(), torch.from_numpy(vals))
    return _INPUTS[key]


def case(C, k, rest, tau, rt, sdt, tdt, weights=None):
    """inputs() and the float64 reference (loss [B], gradient, distilled [B,T,r]) on the up-converted values, once per key"""
    x, vals, idx, rs = inputs(C, k, rest, tau, rt, sdt, tdt)
    key = (C, k, rest, tau, rt, sdt, tdt, None if weights is None else weights.tobytes())
    if key not in _REFS:
        _REFS[key] = TR.topk_loss_and_grad(x.float().numpy(), vals.float().numpy(), idx.numpy(), K.band_ranges(), K.S, K.BOUNDARY,
                                           TC.teacher_ranges(rt), None if rs is None else rs.numpy(), tau, weights)
    return (x, vals, idx, rs) + _REFS[key]


def run(ft, dev, x, vals, idx, rs, rt, tau, reduction="none", weight=None, node_weights=None):
    """(loss, d (weight . loss) / d x) for tensors x, vals, idx, rs on any device (x is made a leaf on `dev` here)"""
    x = x.detach().to(dev).requires_grad_(True)
    tr = TC.teacher_ranges(rt)
    loss = ft.rnnt_kd_loss_pruned_topk(x, vals.to(dev), idx.to(dev), torch.from_numpy(K.band_ranges()).to(dev),
                                       torch.from_numpy(K.BOUNDARY).to(dev),
                                       teacher_ranges=None if tr is None else torch.from_numpy(tr).to(dev),
                                       teacher_rest=None if rs is None else rs.to(dev), temperature=tau,
                                       node_weights=None if node_weights is None else torch.from_numpy(node_weights).to(dev),
                                       reduction=reduction)
    out = loss if weight is None else loss * weight
    out.sum().backward()
    return loss.detach(), x.grad


def check_loss(loss, ref, what, times=1.0, ref64=None):
    """ref64: the float64 value the bound is a function of, where `ref` is another float32 result (times = 2: two bounds)"""
    got = loss.cpu().numpy().astype(np.float64)
    assert loss.dtype == torch.float32 and got.shape == ref.shape and np.isfinite(got).all(), what
    err = np.abs(got - ref)
    worst = float((err / (times * (1e-4 * np.abs(ref if ref64 is None else ref64) + 1e-5))).max())
    print(f"{what}: loss {got}, reference {ref}, |err| / bound = {worst:.3g}")
    assert worst <= 1.0, f"{what}: loss error is {worst:.3g} x its bound"
    return float((err / np.abs(ref)).max())


def check_grad(g, g64, on, sdt, what, times=1.0, other=None):
    """other: another device result to compare with instead of g64, which then only gives the bound (times = 2: two bounds)"""
    _, u, a = DT[sdt]
    g = g.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all(), what
    bound = times * (u * np.abs(g64) + a + 1e-4 * np.abs(g64).max())
    err = np.abs(g - (g64 if other is None else other.float().cpu().numpy().astype(np.float64)))
    worst = float((err / bound).max())
    print(f"{what}: max |g - g64| / bound = {worst:.3g}, max |g64| = {np.abs(g64).max():.3g}")
    assert worst <= 1.0, f"{what}: gradient error is {worst:.3g} x its bound"
    assert (g[~on] == 0).all(), f"{what}: gradient in a row that is not distilled"
    return worst, float(err.max() / np.abs(g64).max())


@pytest.mark.parametrize("C,k,rest,tau,rt,sdt,tdt", CASES)
def test_loss_and_gradient(ft, dev, C, k, rest, tau, rt, sdt, tdt):
    x, vals, idx, rs, ref, g64, on = case(C, k, rest, tau, rt, sdt, tdt)
    assert np.array_equal(on, TC.matched(rt)) and (ref > 0).all()
    what = f"C={C} K={k} rest={rest} tau={tau} r_t={rt} {sdt}/{tdt}"
    loss, g = run(ft, dev, x, vals, idx, rs, rt, tau)
    rel = check_loss(loss, ref, what)
    assert g.dtype == x.dtype and g.shape == x.shape
    frac, gerr = check_grad(g, g64, on, sdt, what)
    _note(f"{'rest' if rest else 'renormalised'} {sdt}/{tdt}", loss_rel_err=rel, grad_err_over_bound=frac, grad_err_over_max=gerr)


@pytest.mark.parametrize("sdt,tdt", [("f32", "f32"), ("bf16", "bf16"), ("fp16", "f32")])
@pytest.mark.parametrize("C,k,tau", [(8, 8, 1.0), (37, 5, 2.0), (500, 8, 1.0), (500, 64, 2.0), (2056, 8, 1.0)])
def test_renormalised_form_against_the_dense_op(ft, dev, C, k, tau, sdt, tdt):
    """teacher_ranges = None, no rest: rnnt_kd_loss_pruned against a dense teacher that is -inf outside the stored columns
    computes the same float64 value, each side within its bound of it -- so the two agree within the sum of the bounds."""
    x, vals, idx, rs, ref, g64, on = case(C, k, False, tau, None, sdt, tdt)
    loss, g = run(ft, dev, x, vals, idx, None, None, tau)
    dense = torch.from_numpy(TC.dense_from_cache(vals.float().numpy(), idx.numpy(), C)).to(DT[tdt][0])
    xd = x.to(dev).requires_grad_(True)
    dl = ft.rnnt_kd_loss_pruned(xd, dense.to(dev), torch.zeros((K.B, K.S), dtype=torch.int32, device=dev),
                                torch.from_numpy(K.band_ranges()).to(dev), 0, torch.from_numpy(K.BOUNDARY).to(dev), mode="full",
                                temperature=tau, reduction="none")
    dl.sum().backward()
    what = f"dense op C={C} K={k} tau={tau} {sdt}/{tdt}"
    check_loss(loss, dl.detach().cpu().numpy().astype(np.float64), what, times=2.0, ref64=ref)
    check_grad(g, g64, on, sdt, what, times=2.0, other=xd.grad)
    check_grad(g, g64, on, sdt, what + " (float64)")


def _used_teacher_rows(rt):
    """bool [B,T,r_t]: the teacher rows some distilled node maps to"""
    on, kp = TR.distilled_nodes(K.band_ranges(), K.BOUNDARY, K.S, TC.teacher_ranges(rt))
    used = np.zeros((K.B, K.T, K.R if rt is None else rt), bool)
    for b, t, k in zip(*np.nonzero(on)):
        used[b, t, kp[b, t, k]] = True
    return on, used


@pytest.mark.parametrize("C,k,rest,rt,sdt,tdt", [(8, 8, False, 2, "f32", "f32"), (37, 5, True, 2, "bf16", "fp16"),
                                                  (500, 8, True, 4, "f32", "bf16"), (500, 64, False, None, "fp16", "fp16"),
                                                  (2048, 8, True, 2, "bf16", "bf16"), (2056, 8, True, 4, "f32", "f32")])
def test_what_is_not_distilled_is_never_read(ft, dev, C, k, rest, rt, sdt, tdt):
    """Teacher rows no distilled node maps to: NaN values (and rest), indices 2^31 - 1 and -5; student rows of nodes that are
    not distilled: NaN.  Loss and gradient bit for bit.  And indices out of range in rows that ARE used are clamped."""
    x, vals, idx, rs = inputs(C, k, rest, 1.0, rt, sdt, tdt)
    clean = run(ft, dev, x, vals, idx, rs, rt, 1.0)
    on, used = _used_teacher_rows(rt)
    assert (~used).any() and (~on).any()
    xp, vp, ip = x.clone(), vals.clone(), idx.clone()
    xp[torch.from_numpy(~on)] = float("nan")
    vp[torch.from_numpy(~used)] = float("nan")
    ip[torch.from_numpy(~used)] = torch.tensor([2 ** 31 - 1, -5], dtype=torch.int32).repeat(k)[:k]
    rp = None
    if rs is not None:
        rp = rs.clone()
        rp[torch.from_numpy(~used)] = float("nan")
    poisoned = run(ft, dev, xp, vp, ip, rp, rt, 1.0)
    assert torch.isfinite(poisoned[0]).all() and torch.equal(clean[0], poisoned[0]) and torch.equal(clean[1], poisoned[1])
    assert (poisoned[1].cpu()[torch.from_numpy(~on)] == 0).all() and poisoned[1].abs().max() > 0
    # clamping: C - 1 written as 2^31 - 1 and column 0 as -5, in the rows that are used
    ic = idx.clone()
    ic[idx == C - 1] = 2 ** 31 - 1
    ic[idx == 0] = -5
    if C <= 37:
        assert (ic[torch.from_numpy(used)] != idx[torch.from_numpy(used)]).any()
    clamped = run(ft, dev, x, vals, ic, rs, rt, 1.0)
    assert torch.equal(clean[0], clamped[0]) and torch.equal(clean[1], clamped[1])


@pytest.mark.parametrize("C,k,rest,rt,sdt,tdt", [(37, 5, True, 4, "f32", "f32"), (500, 8, False, 2, "bf16", "f32"),
                                                  (2056, 8, True, None, "fp16", "bf16")])
def test_node_weights(ft, dev, C, k, rest, rt, sdt, tdt):
    """Weights against the restatement; exact zeros on a chosen set of distilled nodes take them out: their student rows are
    NaN here and their gradient rows zero."""
    rng = np.random.default_rng(17)
    w = rng.uniform(0.25, 2.0, (K.B, K.T, K.R)).astype(np.float32)
    base_on = TC.matched(rt)
    off = base_on & (rng.uniform(size=base_on.shape) < 0.3)
    assert off.any() and (base_on & ~off).sum(axis=(1, 2)).min() >= 2
    w[off] = 0.0
    x, vals, idx, rs, ref, g64, on = case(C, k, rest, 2.0, rt, sdt, tdt, weights=w)
    assert np.array_equal(on, base_on & ~off)
    xp = x.clone()
    xp[torch.from_numpy(~on)] = float("nan")
    what = f"weights C={C} K={k} {sdt}/{tdt}"
    loss, g = run(ft, dev, xp, vals, idx, rs, rt, 2.0, node_weights=w)
    check_loss(loss, ref, what)
    check_grad(g, g64, on, sdt, what)
    ones = run(ft, dev, x, vals, idx, rs, rt, 2.0, node_weights=np.ones_like(w))
    none = run(ft, dev, x, vals, idx, rs, rt, 2.0)
    assert torch.equal(ones[0], none[0]) and torch.equal(ones[1], none[1])
    w[0, 0, 0] = float("nan")        # a valid, matched node of utterance 0: its utterance is poisoned, the other is not
    assert base_on[0, 0, 0]
    bad, _ = run(ft, dev, x, vals, idx, rs, rt, 2.0, node_weights=w)
    assert torch.isnan(bad[0]) and torch.isfinite(bad[1])


@pytest.mark.parametrize("sdt,tdt", [("f32", "f32"), ("bf16", "f32")])
@pytest.mark.parametrize("C,k,rest", [(37, 5, True), (500, 8, False)])
def test_reductions(ft, dev, C, k, rest, sdt, tdt):
    x, vals, idx, rs, ref, g64, on = case(C, k, rest, 1.0, 4, sdt, tdt)
    none, _ = run(ft, dev, x, vals, idx, rs, 4, 1.0)
    for reduction, want, scale in (("sum", none.double().sum().item(), 1.0), ("mean", none.double().mean().item(), 1.0 / K.B)):
        loss, g = run(ft, dev, x, vals, idx, rs, 4, 1.0, reduction=reduction)
        assert loss.shape == () and loss.dtype == torch.float32
        assert abs(loss.item() - want) <= 4 * 2.0 ** -24 * abs(want)          # B = 2 addends, one division: a few ulp
        check_grad(g, g64 * scale, on, sdt, f"{reduction} C={C} {sdt}/{tdt}")


@pytest.mark.parametrize("sdt,tdt", [("f32", "f32"), ("bf16", "bf16")])
def test_upstream_gradient_is_folded_in(ft, dev, sdt, tdt):
    x, vals, idx, rs, ref, g64, on = case(500, 8, True, 2.0, 2, sdt, tdt)
    for reduction, scale in (("sum", 2.5), ("mean", 2.5 / K.B)):
        _, g = run(ft, dev, x, vals, idx, rs, 2, 2.0, reduction=reduction, weight=2.5)
        check_grad(g, g64 * scale, on, sdt, f"2.5 x {reduction} {sdt}")
    w = np.array([0.75, -1.5])
    _, g = run(ft, dev, x, vals, idx, rs, 2, 2.0, weight=torch.tensor(w, dtype=torch.float32, device=dev))
    check_grad(g, g64 * w[:, None, None, None], on, sdt, f"weighted none {sdt}")


@pytest.mark.parametrize("C,k,rest,rt,sdt,tdt", [(500, 8, True, 2, "f32", "f32"), (500, 64, False, 4, "fp16", "bf16"),
                                                  (2056, 8, True, None, "bf16", "bf16")])
def test_two_runs_are_bit_identical(ft, dev, C, k, rest, rt, sdt, tdt):
    x, vals, idx, rs = inputs(C, k, rest, 1.0, rt, sdt, tdt)
    for reduction in ("none", "mean"):
        a = run(ft, dev, x, vals, idx, rs, rt, 1.0, reduction=reduction)
        b = run(ft, dev, x, vals, idx, rs, rt, 1.0, reduction=reduction)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_non_contiguous_and_offset_views(ft, dev):
    x, vals, idx, rs, ref, g64, on = case(37, 5, True, 1.0, 4, "f32", "f32")
    big = torch.full((K.B, K.T, K.R, 37 + 5), 7.0, device=dev)
    big[..., :37] = x.to(dev)
    tv = vals.to(dev).transpose(1, 2).contiguous().transpose(1, 2)
    ti = torch.zeros((K.B, K.T, 4, 5 + 3), dtype=torch.int32, device=dev)
    ti[..., 3:] = idx.to(dev)
    tr = torch.full((K.B, K.T, 4), -9.0, device=dev)
    tr[...] = rs.to(dev)
    tr2 = torch.stack([tr, tr], -1)[..., 1]
    assert not big[..., :37].is_contiguous() and not tv.is_contiguous() and not ti[..., 3:].is_contiguous() and not tr2.is_contiguous()
    loss, g = run(ft, dev, big[..., :37], tv, ti[..., 3:], tr2, 4, 1.0)
    check_loss(loss, ref, "views")
    check_grad(g, g64, on, "f32", "views")
    clean = run(ft, dev, x, vals, idx, rs, 4, 1.0)
    assert torch.equal(loss, clean[0]) and torch.equal(g, clean[1])


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_student_at_an_odd_element(ft, dev, dt):
    """A contiguous 16-bit student whose storage starts at an odd element (2-byte aligned only: no 8-byte access may be made)
    takes the element path and gives the values of the aligned run."""
    x, vals, idx, rs, ref, g64, on = case(500, 8, True, 1.0, 2, dt, dt)
    n = x.numel()
    buf = torch.zeros(n + 9, dtype=x.dtype, device=dev)
    off = buf[1:1 + n].view(x.shape)
    off.copy_(x)
    assert off.is_contiguous() and off.data_ptr() % 4 == 2
    loss, g = run(ft, dev, off, vals, idx, rs, 2, 1.0)
    check_loss(loss, ref, f"odd student {dt}")
    check_grad(g, g64, on, dt, f"odd student {dt}")
    aligned = run(ft, dev, x, vals, idx, rs, 2, 1.0)
    assert float(buf[0]) == 0 and (buf[1 + n:] == 0).all() and torch.equal(off, x.to(dev))     # the neighbours are untouched
    assert (aligned[0] - loss).abs().max() <= 1e-4 * loss.abs().max()


@pytest.mark.parametrize("rest,sdt,tdt", [(True, "f32", "f32"), (False, "bf16", "f32")])
def test_replays_from_a_graph_with_new_values(ft, dev, rest, sdt, tdt):
    """Forward + backward captured once on one stream; two replays with other input contents give the eager results, bit
    for bit."""
    C, k, rt = 500, 8, 2
    x0, v0, i0, r0 = inputs(C, k, rest, 1.0, rt, sdt, tdt)
    x = x0.to(dev).requires_grad_(True)
    vals, idx = v0.to(dev), i0.to(dev)
    rs = None if r0 is None else r0.to(dev)
    rg, bd = torch.from_numpy(K.band_ranges()).to(dev), torch.from_numpy(K.BOUNDARY).to(dev)
    tr = torch.from_numpy(TC.teacher_ranges(rt)).to(dev)

    def step():
        loss = ft.rnnt_kd_loss_pruned_topk(x, vals, idx, rg, bd, teacher_ranges=tr, teacher_rest=rs, reduction="mean")
        (g,) = torch.autograd.grad(loss, x)
        return loss, g

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):          # warm-up outside the capture: allocator pools
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    torch.cuda.synchronize()
    for seed in (11, 12):
        fx = K.logits_pair(C, True, False, seed=seed)[0]
        fy = torch.from_numpy(TC.dense_teacher(C, rt, seed=seed)).to(DT[tdt][0]).float().numpy()
        fv, fi, fr = TC.topk_cache(fy, k, 1.0, rest)
        with torch.no_grad():
            x.copy_(torch.from_numpy(fx))                 # new values, same buffers
            vals.copy_(torch.from_numpy(fv))
            idx.copy_(torch.from_numpy(fi))
            if rest:
                rs.copy_(torch.from_numpy(fr))
        graph.replay()
        torch.cuda.synchronize()
        got = [v.clone() for v in out]
        ref = step()
        torch.cuda.synchronize()
        assert torch.isfinite(got[0]) and got[0] > 0
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


@pytest.mark.parametrize("sdt,tdt", [("f32", "f32"), ("bf16", "bf16")])
@pytest.mark.parametrize("C,tau", [(8, 1.0), (37, 2.0)])
def test_cache_builder_and_the_full_loss(ft, dev, C, tau, sdt, tdt):
    """rnnt_kd_topk_teacher on the device against the numpy top-K; and its output with K = C on the student's own ranges is
    the whole teacher, so the loss is rnnt_kd_loss_pruned's full loss -- within the sum of the two bounds."""
    y = torch.from_numpy(TC.dense_teacher(C, None)).to(DT[tdt][0])
    for k in (1 if C == 8 else 5, C):     # the shapes of the parity cases, whose rest class carries mass
        vals, idx, rest = ft.rnnt_kd_topk_teacher(y.to(dev), k, temperature=tau)
        nv, ni, nr = TC.topk_cache(y.float().numpy(), k, tau, k < C)
        assert vals.dtype == y.dtype and idx.dtype == torch.int32 and rest.dtype == torch.float32 and rest.is_cuda
        assert np.array_equal(vals.float().cpu().numpy(), nv)
        assert np.array_equal(np.take_along_axis(y.float().numpy(), idx.cpu().numpy().astype(np.int64), -1), nv)
        if k < C:
            assert np.abs(rest.cpu().numpy() - nr).max() <= 8 * 2.0 ** -24 * max(1.0, np.abs(nr).max())
        else:
            assert (rest == float("-inf")).all()
    x = torch.from_numpy(TC.student(C)).to(DT[sdt][0])
    rg, bd = torch.from_numpy(K.band_ranges()).to(dev), torch.from_numpy(K.BOUNDARY).to(dev)
    xa, xb = x.to(dev).requires_grad_(True), x.to(dev).requires_grad_(True)
    la = ft.rnnt_kd_loss_pruned_topk(xa, vals, idx, rg, bd, teacher_ranges=rg, teacher_rest=rest, temperature=tau, reduction="none")
    lb = ft.rnnt_kd_loss_pruned(xb, y.to(dev), torch.zeros((K.B, K.S), dtype=torch.int32, device=dev), rg, 0, bd, mode="full",
                                temperature=tau, reduction="none")
    la.sum().backward()
    lb.sum().backward()
    ref, g64 = R.kd_loss_and_grad(x.float().numpy(), y.float().numpy(), np.zeros((K.B, K.S), np.int32), K.band_ranges(), 0,
                                  K.BOUNDARY, "full", tau)
    on = R.valid_nodes(K.band_ranges(), K.BOUNDARY, K.S)
    what = f"K = C = {C} tau={tau} {sdt}/{tdt}"
    check_loss(la.detach(), ref, what)
    check_grad(xa.grad, g64, on, sdt, what)
    check_loss(la.detach(), lb.detach().cpu().numpy().astype(np.float64), what + " against the dense op", times=2.0, ref64=ref)
    check_grad(xa.grad, g64, on, sdt, what + " against the dense op", times=2.0, other=xb.grad)
