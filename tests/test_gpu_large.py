"""Logits-shaped tensors past 2^31 elements (and once past 2^32): does any index reach a [B,T,r,C] pointer in 32 bits?

The largest tensor elsewhere in the suite has 3.3e8 elements; the pruned logits of an ordinary training step pass 2^31.
Every kernel treats utterances independently, so the check needs no large reference: the op runs on the whole batch
(built on the device by a seeded generator) and again on the three-utterance batch made of utterance 0, the utterance k
that straddles element 2^31 (2^32) and the last one, which lies wholly beyond it; the three utterances' outputs and
their slices of every gradient must agree (normwise max|d| / max|ref| <= 1e-4, the suite's TOL_F64; integers bit for
bit).  One 32-bit product anywhere would make the big run read or write another utterance's rows.  In addition 64
seeded rows of the LAST utterance of the big run are pinned to float64 directly: log-softmax for px / py, and
``gx 1[sym] + gy 1[blank] - softmax (gx + gy)`` for d logits with the known upstream gradient; for the losses (whose
upstream, the occupancies, is internal) the rows must have that form for the `gx + gy` they imply.  d logits of the big
run is finite everywhere.

Each case computes what it needs (tensor + gradient + copies + outputs) and skips only when the device reports less
free memory than that plus 4 GiB; it frees everything before it returns.  Measured differences are printed.
"""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL_F64 = 1e-4
S = 24
T = 8192
BIG_BLANKS = ((1, 2), (2, 4), (3, 8))
BLANK = 0
GIB = 1 << 30


def _need_or_skip(dev, n_big, per, extra=0):
    """n_big logits-sized tensors + the three-utterance copies of each + `extra` bytes, or skip with the figures."""
    need = 4 * (n_big * per[0] * per[1] + n_big * 3 * per[1]) + extra
    free, total = torch.cuda.mem_get_info(dev)
    if free < need + 4 * GIB:
        pytest.skip(f"needs {need / GIB:.1f} GiB + 4 GiB headroom, device reports {free / GIB:.1f} GiB free of {total / GIB:.1f} GiB")
    return need


def _free():
    gc.collect()
    torch.cuda.empty_cache()


def _straddler(B, per, limit):
    k = limit // per
    assert 0 < k < B - 1 and k * per < limit < (k + 1) * per and (B - 1) * per >= limit, (B, per, limit, k)
    return [0, k, B - 1]


def _inputs(ft, dev, B, r, C, seed):
    """symbols in [4, C-2] (no blank of any op here), ragged t_end / s_end, ranges from get_rnnt_prune_ranges on a small
    simple loss (16 columns), as test_gpu_multiblank._loss_inputs does."""
    g = torch.Generator(device=dev).manual_seed(seed)
    sym = torch.randint(4, C - 1, (B, S), generator=g, device=dev, dtype=torch.int32)
    bd = torch.zeros((B, 4), dtype=torch.int32, device=dev)
    bd[:, 2] = torch.randint(S // 2, S + 1, (B,), generator=g, device=dev, dtype=torch.int32)
    bd[:, 3] = torch.randint(T // 2, T + 1, (B,), generator=g, device=dev, dtype=torch.int32)
    bd[0, 2], bd[0, 3] = S, T
    am = torch.randn((B, T, 16), generator=g, device=dev); lm = torch.randn((B, S + 1, 16), generator=g, device=dev)
    _, (gx, gy) = ft.rnnt_loss_simple(lm, am, sym % 15, 15, boundary=bd, reduction="sum", calc_gradients=True)
    ranges = ft.get_rnnt_prune_ranges(gx, gy, bd, r)
    assert tuple(ranges.shape) == (B, T, r)
    w = torch.rand((B,), generator=g, device=dev) + 0.5
    return sym, bd, ranges, w, g


def _logits(shape, g, dev):
    x = torch.empty(shape, dtype=torch.float32, device=dev)
    for b in range(shape[0]):          # utterance by utterance: the generator kernels stay far below 2^31 themselves
        x[b].normal_(0.0, 2.0, generator=g)
    return x


def _pick(x, idx):
    return torch.stack([x[i] for i in idx])


def _rel(got, ref, what):
    """normwise max|d| / max|ref| on the device; the -inf pattern must be the same."""
    if not got.dtype.is_floating_point:
        assert torch.equal(got, ref), f"{what}: integer output differs"
        return 0.0
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(got), fin), f"{what}: finite pattern differs"
    z = torch.zeros((), device=ref.device)
    e = float(torch.where(fin, got - ref, z).abs().max() / torch.where(fin, ref, z).abs().max().clamp_min(1e-30))
    return e


def _compare(pairs, tag):
    errs = {name: _rel(a, b, f"{tag} {name}") for name, (a, b) in pairs.items()}
    print(f"large {tag}: big run vs three-utterance run: " + ", ".join(f"{k} {v:.3g}" for k, v in errs.items()))
    bad = {k: v for k, v in errs.items() if not v <= TOL_F64}
    assert not bad, (tag, bad)


def _sample_rows(bd_last, n_t, r, seed):
    rs = np.random.RandomState(seed)
    te = int(bd_last[3])
    return rs.randint(0, te, 64), rs.randint(0, r, 64)


def _rows64(x_last, ts, ks):
    return torch.stack([x_last[int(t), int(k)] for t, k in zip(ts, ks)]).double().cpu().numpy()


def _nrel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _log_softmax64(x):
    m = x.max(axis=1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=1, keepdims=True))


# (B, r, C, limit, ops): the 2^31 shapes of the pruned ops
SHAPES31 = {"C2048": (27, 5, 2048), "C501": (106, 5, 501)}


@pytest.mark.parametrize("shape", list(SHAPES31))
def test_pruned_logprobs_past_2_31(ft, dev, shape):
    """get_rnnt_logprobs_pruned forward + backward and rnnt_alignment_pruned."""
    B, r, C = SHAPES31[shape]
    per = T * r * C
    idx = _straddler(B, per, 1 << 31)
    _need_or_skip(dev, 2, (B, per), extra=8 * 4 * B * (S + 1) * (T + 1))
    sym, bd, ranges, w, g = _inputs(ft, dev, B, r, C, 31)
    x = _logits((B, T, r, C), g, dev).requires_grad_(True)
    assert x.numel() > (1 << 31)
    px, py = ft.get_rnnt_logprobs_pruned(x, sym, ranges, BLANK, bd)
    gpx = torch.randn(px.shape, generator=g, device=dev); gpy = torch.randn(py.shape, generator=g, device=dev)
    torch.autograd.backward([px, py], [gpx, gpy])
    score, frames = ft.rnnt_alignment_pruned(x.detach(), sym, ranges, BLANK, bd)
    assert bool(torch.isfinite(x.grad).all())

    xs = _pick(x.detach(), idx).requires_grad_(True)
    spx, spy = ft.get_rnnt_logprobs_pruned(xs, sym[idx], ranges[idx], BLANK, bd[idx])
    torch.autograd.backward([spx, spy], [gpx[idx], gpy[idx]])
    sscore, sframes = ft.rnnt_alignment_pruned(xs.detach(), sym[idx], ranges[idx], BLANK, bd[idx])
    _compare(dict(px=(px.detach()[idx], spx.detach()), py=(py.detach()[idx], spy.detach()), dlogits=(_pick(x.grad, idx), xs.grad),
                  score=(score[idx], sscore), frames=(frames[idx], sframes)), f"pruned logprobs {shape}")

    # the last utterance of the big run against float64, 64 rows
    b = B - 1
    bdl = bd[b].cpu().numpy(); rg = ranges[b].cpu().numpy(); sy = sym[b].cpu().numpy()
    ts, ks = _sample_rows(bdl, T, r, 5)
    rows = _rows64(x.detach()[b], ts, ks)
    lsm = _log_softmax64(rows)
    sm = np.exp(lsm)
    grows = _rows64(x.grad[b], ts, ks)
    pxb, pyb = px.detach()[b].double().cpu().numpy(), py.detach()[b].double().cpu().numpy()
    gpxb, gpyb = gpx[b].double().cpu().numpy(), gpy[b].double().cpu().numpy()
    got_l, want_l, want_g = [], [], np.zeros_like(rows)
    for i, (t, k) in enumerate(zip(ts, ks)):
        s = rg[t, k]
        gy = gpyb[s, t]; gx = 0.0
        got_l.append(pyb[s, t]); want_l.append(lsm[i, BLANK])
        if s < S:
            got_l.append(pxb[s, t]); want_l.append(lsm[i, sy[s]])      # t < t_end: not the boundary column
            gx = gpxb[s, t]
            want_g[i, sy[s]] += gx
        want_g[i, BLANK] += gy
        want_g[i] -= sm[i] * (gx + gy)
    el, eg = _nrel(np.array(got_l), np.array(want_l)), _nrel(grows, want_g)
    print(f"large pruned logprobs {shape}: last utterance vs float64: px/py {el:.3g}, d logits rows {eg:.3g}")
    assert el <= TOL_F64 and eg <= TOL_F64, (el, eg)
    del x, xs, px, py, spx, spy, gpx, gpy
    _free()


def _loss_case(ft, dev, B, r, C, limit, fn, tag, pin=True, identity=False):
    """A loss (reduction "none", per-utterance upstream weights) forward + backward on the whole batch and on the three."""
    per = T * r * C
    idx = _straddler(B, per, limit)
    _need_or_skip(dev, 2, (B, per), extra=8 * 4 * B * (S + 1) * (T + 1) * 4)
    sym, bd, ranges, w, g = _inputs(ft, dev, B, 5 if identity else r, C, 17)
    x = _logits((B, T, r, C), g, dev).requires_grad_(True)
    assert x.numel() > limit
    loss = fn(x, sym, ranges, bd)
    (loss * w).sum().backward()
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(x.grad).all())
    xs = _pick(x.detach(), idx).requires_grad_(True)
    sloss = fn(xs, sym[idx], ranges[idx].clone(), bd[idx])
    (sloss * w[idx]).sum().backward()
    _compare(dict(loss=(loss.detach()[idx], sloss.detach()), dlogits=(_pick(x.grad, idx), xs.grad)), tag)
    if pin:
        # rows of the last utterance: g = gx 1[sym] + gy 1[blank] - softmax64 (gx + gy) for the (gx + gy) the row implies
        b = B - 1
        ts, ks = _sample_rows(bd[b].cpu().numpy(), T, r, 9)
        sm = np.exp(_log_softmax64(_rows64(x.detach()[b], ts, ks)))
        grows = _rows64(x.grad[b], ts, ks)
        rg = np.arange(r)[None, :].repeat(T, 0) if identity else ranges[b].cpu().numpy()
        sy = sym[b].cpu().numpy()
        worst, wsum = 0.0, 0.0
        for i, (t, k) in enumerate(zip(ts, ks)):
            s = rg[t, k]
            other = np.ones(C, bool); other[BLANK] = False
            if s < S:
                other[sy[s]] = False
            tot = -grows[i, other].sum() / sm[i, other].sum()
            scale = max(np.abs(grows[i]).max(), 1e-30)
            if scale > 1e-20:                       # rows off every path carry (numerically) no gradient
                worst = max(worst, np.abs(grows[i, other] + sm[i, other] * tot).max() / scale)
                wsum = max(wsum, abs(grows[i].sum()) / scale)
        print(f"large {tag}: last utterance d logits rows vs float64 softmax form {worst:.3g}, row sums {wsum:.3g}")
        assert worst <= TOL_F64 and wsum <= TOL_F64, (worst, wsum)
    del x, xs, loss, sloss
    _free()


@pytest.mark.parametrize("route", ["band", "lattice"])
@pytest.mark.parametrize("shape", list(SHAPES31))
def test_rnnt_loss_pruned_past_2_31(ft, dev, shape, route, monkeypatch):
    monkeypatch.setenv("FTR_PRUNED_ROUTE", route)
    B, r, C = SHAPES31[shape]
    fn = lambda x, sym, ranges, bd: ft.rnnt_loss_pruned(x, sym, ranges, BLANK, bd, delay_penalty=0.05, reduction="none")
    _loss_case(ft, dev, B, r, C, 1 << 31, fn, f"rnnt_loss_pruned {shape} {route}")


@pytest.mark.parametrize("shape", list(SHAPES31))
def test_hat_loss_pruned_past_2_31(ft, dev, shape):
    B, r, C = SHAPES31[shape]
    fn = lambda x, sym, ranges, bd: ft.hat_loss_pruned(x, sym, ranges, BLANK, bd, reduction="none")
    _loss_case(ft, dev, B, r, C, 1 << 31, fn, f"hat_loss_pruned {shape}", pin=False)


@pytest.mark.parametrize("shape", list(SHAPES31))
def test_multiblank_loss_pruned_past_2_31(ft, dev, shape):
    B, r, C = SHAPES31[shape]
    fn = lambda x, sym, ranges, bd: ft.rnnt_loss_multiblank_pruned(x, sym, ranges, BLANK, BIG_BLANKS, bd, sigma=0.05, reduction="none")
    _loss_case(ft, dev, B, r, C, 1 << 31, fn, f"rnnt_loss_multiblank_pruned {shape}", pin=False)


def test_rnnt_loss_joint_past_2_31(ft, dev):
    """The unpruned joint [B, T, S+1, C]: r = S + 1 = 25, C = 512, B = 22 (utterance 20 straddles 2^31)."""
    fn = lambda x, sym, ranges, bd: ft.rnnt_loss(x, sym, BLANK, boundary=bd, delay_penalty=0.05, reduction="none")
    _loss_case(ft, dev, 22, S + 1, 512, 1 << 31, fn, "rnnt_loss joint", identity=True)


def test_rnnt_loss_pruned_past_2_32(ft, dev):
    """4.45e9 elements: B = 53, utterance 51 straddles 2^32."""
    fn = lambda x, sym, ranges, bd: ft.rnnt_loss_pruned(x, sym, ranges, BLANK, bd, delay_penalty=0.05, reduction="none")
    _loss_case(ft, dev, 53, 5, 2048, 1 << 32, fn, "rnnt_loss_pruned past 2^32")


@pytest.mark.parametrize("dense", [False, True])
def test_do_rnnt_pruning_past_2_31(ft, dev, dense):
    """The gather (lm_pruned, and am_pruned with dense=True, have 2.26e9 elements) and its backward with dense random
    upstream gradients.  The gather copies: bit equality; the backward sums r rows (d am) and a segment (d lm)."""
    B, r, C = 27, 5, 2048
    per = T * r * C
    idx = _straddler(B, per, 1 << 31)
    _need_or_skip(dev, 4, (B, per), extra=4 * 4 * B * T * C)
    sym, bd, ranges, w, g = _inputs(ft, dev, B, r, C, 23)
    am = torch.randn((B, T, C), generator=g, device=dev).requires_grad_(True)
    lm = torch.randn((B, S + 1, C), generator=g, device=dev).requires_grad_(True)
    am_p, lm_p = ft.do_rnnt_pruning(am, lm, ranges, dense=dense)
    assert lm_p.numel() > (1 << 31) and am_p.is_contiguous() == dense
    ga = _logits((B, T, r, C), g, dev); gl = _logits((B, T, r, C), g, dev)
    torch.autograd.backward([am_p, lm_p], [ga, gl])
    ams = am.detach()[idx].clone().requires_grad_(True); lms = lm.detach()[idx].clone().requires_grad_(True)
    sam_p, slm_p = ft.do_rnnt_pruning(ams, lms, ranges[idx], dense=dense)
    torch.autograd.backward([sam_p, slm_p], [_pick(ga, idx), _pick(gl, idx)])
    for j, i in enumerate(idx):
        assert torch.equal(lm_p.detach()[i], slm_p.detach()[j]) and torch.equal(am_p.detach()[i], sam_p.detach()[j]), i
    _compare(dict(d_am=(am.grad[idx], ams.grad), d_lm=(lm.grad[idx], lms.grad)), f"do_rnnt_pruning dense={dense}")
    # the last utterance against the definition: the gather exactly, d am = sum over k in float64
    b = B - 1
    ts, ks = _sample_rows(bd[b].cpu().numpy(), T, r, 3)
    rg = ranges[b].cpu().numpy()
    for t, k in zip(ts, ks):
        assert torch.equal(lm_p.detach()[b, int(t), int(k)], lm.detach()[b, int(rg[t, k])])
        assert torch.equal(am_p.detach()[b, int(t), int(k)], am.detach()[b, int(t)])
    want = torch.stack([ga[b, int(t)].double().sum(0) for t in ts]).cpu().numpy()
    got = torch.stack([am.grad[b, int(t)] for t in ts]).double().cpu().numpy()
    e = _nrel(got, want)
    print(f"large do_rnnt_pruning dense={dense}: last utterance d am rows vs float64 {e:.3g}")
    assert e <= TOL_F64
    assert bool(torch.isfinite(am.grad).all()) and bool(torch.isfinite(lm.grad).all())
    del am, lm, am_p, lm_p, ga, gl, ams, lms, sam_p, slm_p
    _free()


def test_row_count_bound_is_an_invalid_argument(ft, dev):
    """include/ftr.h: element counts are size_t, the number of [B,T,s_range] rows stays below 2^31.  The bound is checked
    before anything is launched or read."""
    from tf_fast_rnnt import _lib
    t = torch.zeros(64, device=dev)
    i = torch.zeros(64, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    with pytest.raises(_lib.FtrError):
        _lib.call("ftr_pruned_logprobs_fwd_f32", t.data_ptr(), i.data_ptr(), i.data_ptr(), None, 0, 0.0, t.data_ptr(), t.data_ptr(),
                  t.data_ptr(), 1 << 16, 1 << 14, 4, 4, 2, 0, st)
    with pytest.raises(_lib.FtrError):
        _lib.call("ftr_do_pruning_f32", t.data_ptr(), t.data_ptr(), i.data_ptr(), None, t.data_ptr(), 1 << 16, 1 << 14, 5, 4, 2, st)
    torch.cuda.synchronize()
