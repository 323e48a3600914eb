"""bfloat16 / float16 joiner logits through the pruned loss path (rnnt_loss_pruned, hat_loss_pruned, the log-prob
builders, the alignment, and the unpruned forms that run on identity ranges).

The definition under test: a 16-bit `logits` tensor means the float32 tensor `logits.float()` (exact); lse, px / py, the
recursion and the loss are float32 as before; the gradient is computed in float32 and rounded once, to nearest-even, into
the dtype of `logits`.  So the references are the existing oracles ON THE UP-CONVERTED VALUES, the loss keeps the project's
tolerance (helpers.assert_parity, 1e-4), and a gradient element g may differ from the float64-recursion reference g64 by

    |g - g64| <= u |g64| + a + 1e-4 max|g64|

u = unit roundoff of the storage type (2^-8 bf16, 2^-11 fp16), a = half the fp16 subnormal spacing (2^-25; 0 for bf16, whose
exponent range is float32's), and the last term the float32 budget every gradient test of this project uses.  All three
are derived, none is measured.  reduction="sum" keeps the gradient elements O(1), well inside fp16's range.

Shapes: B=2 T=12 S=5 r=3, utterance 1 ragged (t_end 9, s_end 3); C crosses every path of the kernels: 8 (a partly filled
wave), 36 (C % 4 == 0, C % 8 != 0), 37 (scalar path), 500 (c3's vocabulary), 512 (one exactly full register quad), 520 (a
ragged second quad), 2048 (the largest register-resident row), 2056 (the two-pass kernel)."""
import numpy as np
import pytest
import torch

from helpers import assert_parity, max_rel

pytestmark = pytest.mark.gpu

B, T, S, R = 2, 12, 5, 3
BOUNDARY = np.array([[0, 0, S, T], [0, 0, 3, 9]], np.int32)
DTYPES = {"bf16": (torch.bfloat16, 2.0 ** -8, 0.0), "fp16": (torch.float16, 2.0 ** -11, 2.0 ** -25)}
ROUTES = ["band", "lattice"]
# (C, blank is the last column?, rnnt_type, hat): every C, both blanks, both types and both normalisations occur, and each
# case runs with both dtypes on both routes
CASES = [(8, False, "regular", False), (36, True, "modified", False), (37, False, "regular", True),
         (37, True, "modified", False), (500, True, "regular", False), (500, False, "modified", True),
         (512, False, "modified", True), (520, True, "regular", False), (2048, False, "modified", False),
         (2056, True, "regular", True)]


@pytest.fixture(autouse=True)
def _route_unset(monkeypatch):
    monkeypatch.delenv("FTR_PRUNED_ROUTE", raising=False)
    monkeypatch.delenv("FTR_BAND_IMPL", raising=False)


def _set_route(monkeypatch, route):
    monkeypatch.setenv("FTR_PRUNED_ROUTE", "lattice" if route == "lattice" else "band")


def band_ranges():
    """A band built by hand: ranges[b,t,0] climbs from 0 to s_end + 1 - r over the utterance's frames, steps <= 1."""
    rg = np.zeros((B, T, R), np.int32)
    for b in range(B):
        top, te = max(int(BOUNDARY[b, 2]) + 1 - R, 0), int(BOUNDARY[b, 3])
        s0 = np.minimum((np.arange(T) * top + te - 2) // max(te - 1, 1), top)
        rg[b] = s0[:, None] + np.arange(R)[None, :]
    return rg


_INPUTS = {}


def inputs(C, dtype_name, blank_last, s1=R):
    """(x16 cpu tensor [B,T,s1,C], symbols, blank): standard normal x 3 rounded to the 16-bit type.  One symbol sits in the
    last column of a lane's 4-vector (column 3).  Cached, never modified."""
    key = (C, dtype_name, blank_last, s1)
    if key not in _INPUTS:
        rng = np.random.default_rng(1000 + C)
        x = torch.from_numpy((3.0 * rng.standard_normal((B, T, s1, C))).astype(np.float32)).to(DTYPES[dtype_name][0])
        blank = C - 1 if blank_last else 0
        sym = rng.integers(1, C - 1, (B, S)).astype(np.int32)
        sym[:, 0] = 3
        _INPUTS[key] = (x, sym, blank)
    return _INPUTS[key]


_REFS = {}


def reference(oracle, C, dtype_name, blank_last, rnnt_type, hat):
    """(loss32, loss64, g64) of the sum-reduced loss on x16.float(), computed once per input."""
    key = (C, dtype_name, blank_last, rnnt_type, hat)
    if key in _REFS:
        return _REFS[key]
    x16, sym, blank = inputs(C, dtype_name, blank_last)
    rg = band_ranges()
    if not hat:
        x32 = x16.float().numpy()
        l32, _ = oracle.rnnt_loss_pruned_grad(x32, sym, rg, blank, BOUNDARY, rnnt_type, reduction="sum")
        l64, g64 = oracle.rnnt_loss_pruned_grad(x32, sym, rg, blank, BOUNDARY, rnnt_type, reduction="sum", dtype=np.float64)
        out = (float(l32), float(l64), np.asarray(g64, np.float64))
    else:
        import hat_restatement as H
        res = []
        for dt in (torch.float32, torch.float64):
            x = x16.to(dt).requires_grad_(True)
            px, py = H.get_hat_logprobs_pruned_torch(x, torch.from_numpy(sym), torch.from_numpy(rg), blank,
                                                     torch.from_numpy(BOUNDARY), rnnt_type)
            loss = H.lattice_loss_torch(px, py, BOUNDARY, rnnt_type).sum()
            loss.backward()
            res.append((float(loss.detach()), x.grad.numpy().astype(np.float64)))
        out = (res[0][0], res[1][0], res[1][1])
    _REFS[key] = out
    return out


def check_grad(g, g64, dtype_name, what):
    _, u, a = DTYPES[dtype_name]
    g = g.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all(), what
    bound = u * np.abs(g64) + a + 1e-4 * np.abs(g64).max()
    err = np.abs(g - g64)
    worst = float((err / bound).max())
    print(f"{what}: max |g - g64| / bound = {worst:.3g}, max |g64| = {np.abs(g64).max():.3g}")
    assert worst <= 1.0, f"{what}: gradient error is {worst:.3g} x its bound"
    te = int(BOUNDARY[1, 3])      # outside the boundary (the frames from t_end on) zeros stay zeros, exactly
    assert (g64[1, te:] == 0).all() and (g[1, te:] == 0).all(), f"{what}: gradient in the frames from t_end on"


def run_loss(ft, x, sym, rg, blank, rnnt_type, hat):
    """loss (sum) and d loss / d x for a device tensor x (made a leaf here)."""
    dev = x.device
    x = x.detach().requires_grad_(True)
    f = ft.hat_loss_pruned if hat else ft.rnnt_loss_pruned
    loss = f(x, torch.from_numpy(sym).to(dev), torch.from_numpy(rg).to(dev), blank, torch.from_numpy(BOUNDARY).to(dev),
             rnnt_type=rnnt_type, reduction="sum")
    loss.backward()
    return loss, x.grad


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("C,blank_last,rnnt_type,hat", CASES)
def test_pruned_loss_and_gradient(ft, dev, oracle, C, blank_last, rnnt_type, hat, dtype_name, route, monkeypatch):
    _set_route(monkeypatch, route)
    x16, sym, blank = inputs(C, dtype_name, blank_last)
    l32, l64, g64 = reference(oracle, C, dtype_name, blank_last, rnnt_type, hat)
    loss, g = run_loss(ft, x16.to(dev), sym, band_ranges(), blank, rnnt_type, hat)
    assert loss.dtype == torch.float32 and g.dtype == x16.dtype and g.shape == x16.shape
    assert_parity(loss.item(), l32, l64, tol=1e-4, what="loss")
    check_grad(g, g64, dtype_name, f"C={C} {dtype_name} {route} {rnnt_type} hat={hat}")


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("C,rnnt_type", [(36, "regular"), (500, "modified"), (37, "constrained"), (2056, "regular")])
def test_logprobs_pruned(ft, dev, oracle, C, rnnt_type, dtype_name):
    x16, sym, blank = inputs(C, dtype_name, True)
    rg = band_ranges()
    px, py = ft.get_rnnt_logprobs_pruned(x16.to(dev), torch.from_numpy(sym).to(dev), torch.from_numpy(rg).to(dev), blank,
                                         torch.from_numpy(BOUNDARY).to(dev), rnnt_type)
    assert px.dtype == torch.float32 and py.dtype == torch.float32
    opx, opy = oracle.get_rnnt_logprobs_pruned(x16.float().numpy(), sym, rg, blank, BOUNDARY, rnnt_type)
    assert max_rel(px.cpu().numpy(), opx) <= 1e-4 and max_rel(py.cpu().numpy(), opy) <= 1e-4   # max_rel: same -inf pattern


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("C,hat", [(36, False), (500, False), (37, True)])
def test_logprobs_joint(ft, dev, oracle, C, hat, dtype_name):
    """Unpruned logits [B,T,S+1,C]: identity ranges through the same kernels."""
    x16, sym, blank = inputs(C, dtype_name, False, s1=S + 1)
    bd = torch.from_numpy(BOUNDARY).to(dev)
    if hat:
        import hat_restatement as H
        px, py = ft.get_hat_logprobs_joint(x16.to(dev), torch.from_numpy(sym).to(dev), blank, bd)
        opx, opy = H.get_hat_logprobs_joint_torch(x16.double(), torch.from_numpy(sym), blank, torch.from_numpy(BOUNDARY))
        opx, opy = opx.numpy(), opy.numpy()
    else:
        px, py = ft.get_rnnt_logprobs_joint(x16.to(dev), torch.from_numpy(sym).to(dev), blank, bd)
        opx, opy = oracle.get_rnnt_logprobs_joint(x16.float().numpy(), sym, blank, BOUNDARY)
    assert px.dtype == torch.float32 and py.dtype == torch.float32
    assert max_rel(px.cpu().numpy(), opx) <= 1e-4 and max_rel(py.cpu().numpy(), opy) <= 1e-4


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_unpruned_loss(ft, dev, oracle, dtype_name):
    """rnnt_loss / hat_loss on 16-bit joiner logits: loss float32, gradient in the input dtype, close to the float32 run
    on the up-converted tensor (both go through the kernels checked above)."""
    x16, sym, blank = inputs(36, dtype_name, False, s1=S + 1)
    symd, bd = torch.from_numpy(sym).to(dev), torch.from_numpy(BOUNDARY).to(dev)
    ref = float(oracle.rnnt_loss(x16.float().numpy(), sym, blank, BOUNDARY, reduction="sum"))
    for f, want in ((ft.rnnt_loss, ref), (ft.hat_loss, None)):
        x = x16.to(dev).requires_grad_(True)
        loss = f(x, symd, blank, bd, reduction="sum")
        loss.backward()
        x32 = x16.to(dev).float().requires_grad_(True)
        loss32 = f(x32, symd, blank, bd, reduction="sum")
        loss32.backward()
        assert loss.dtype == torch.float32 and x.grad.dtype == x16.dtype
        if want is not None:
            assert abs(loss.item() - want) <= 1e-4 * abs(want)
        assert abs(loss.item() - loss32.item()) <= 1e-4 * abs(loss32.item())
        check_grad(x.grad, x32.grad.cpu().numpy().astype(np.float64), dtype_name, f.__name__)


def _path_scores(px, py, b, modified):
    """Scores of all monotone paths of utterance b, float64."""
    sb, tb, se, te = [int(v) for v in BOUNDARY[b]]
    out = []

    def walk(s, t, acc):
        if s == se and t == te:
            out.append(acc)
            return
        if t < te:
            walk(s, t + 1, acc + float(py[b, s, t]))
        if s < se and (not modified or t < te):
            walk(s + 1, t + 1 if modified else t, acc + float(px[b, s, t]))

    walk(sb, tb, 0.0)
    return np.sort(np.array([v for v in out if np.isfinite(v)]))[::-1]


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("rnnt_type", ["regular", "modified"])
def test_alignment(ft, dev, oracle, rnnt_type, dtype_name):
    import viterbi_restatement as V
    x16, sym, blank = inputs(36, dtype_name, True)
    rg = band_ranges()
    # the float32 best path must win by more than 1e-3, so that no summation order can flip it (checked here, on the CPU)
    opx, opy = oracle.get_rnnt_logprobs_pruned(x16.float().numpy(), sym, rg, blank, BOUNDARY, rnnt_type)
    for b in range(B):
        sc = _path_scores(opx, opy, b, rnnt_type != "regular")
        assert len(sc) >= 2 and sc[0] - sc[1] > 1e-3, f"utterance {b}: best path leads by {sc[0] - sc[1]:.3g} only"
    args = (torch.from_numpy(sym).to(dev), torch.from_numpy(rg).to(dev), blank, torch.from_numpy(BOUNDARY).to(dev), rnnt_type)
    score16, frames16 = ft.rnnt_alignment_pruned(x16.to(dev), *args)
    score32, frames32 = ft.rnnt_alignment_pruned(x16.to(dev).float(), *args)
    assert torch.equal(frames16, frames32)
    assert np.array_equal(frames16.cpu().numpy(), V.viterbi(opx, opy, BOUNDARY)[1])
    assert max_rel(score16.cpu().numpy(), score32.cpu().numpy()) <= 1e-5


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("C", [36, 500])
@pytest.mark.parametrize("layout", ["odd_offset", "slice"])
def test_layouts(ft, dev, oracle, layout, C, dtype_name, route, monkeypatch):
    """A contiguous tensor whose storage starts at an odd element (its base is only 2-byte aligned: no 8-byte access may be
    made) and a non-contiguous slice of a wider tensor."""
    _set_route(monkeypatch, route)
    x16, sym, blank = inputs(C, dtype_name, True)
    l32, l64, g64 = reference(oracle, C, dtype_name, True, "regular", False)
    n = x16.numel()
    if layout == "odd_offset":
        base = torch.zeros(n + 9, dtype=x16.dtype, device=dev)
        x = base[1:1 + n].view(B, T, R, C)
        x.copy_(x16)
        assert x.is_contiguous() and x.data_ptr() % 4 == 2
    else:
        big = torch.full((B, T, R, C + 12), 7.0, dtype=x16.dtype, device=dev)
        big[..., :C] = x16.to(dev)
        x = big[:, :, :, :C]
        assert not x.is_contiguous()
    loss, g = run_loss(ft, x, sym, band_ranges(), blank, "regular", False)
    assert loss.dtype == torch.float32 and g.dtype == x16.dtype and g.shape == x16.shape
    assert_parity(loss.item(), l32, l64, tol=1e-4, what="loss")
    check_grad(g, g64, dtype_name, f"{layout} C={C} {dtype_name} {route}")
    if layout == "odd_offset":
        assert float(base[0]) == 0 and (base[1 + n:] == 0).all()     # the input's neighbours are untouched


@pytest.mark.parametrize("route", ROUTES)
def test_float32_is_untouched_by_16bit_calls(ft, dev, route, monkeypatch):
    """The same float32 call before and after 16-bit calls in one process: bit-identical loss and gradient."""
    _set_route(monkeypatch, route)
    x16, sym, blank = inputs(500, "bf16", True)
    x32 = x16.float().to(dev) * 1.37       # not representable in 16 bits
    rg = band_ranges()
    for hat in (False, True):
        before = run_loss(ft, x32, sym, rg, blank, "regular", hat)
        for name in DTYPES:
            run_loss(ft, inputs(500, name, True)[0].to(dev), sym, rg, blank, "regular", hat)
        after = run_loss(ft, x32, sym, rg, blank, "regular", hat)
        assert before[1].dtype == torch.float32
        assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


def test_out_of_scope_ops_still_refuse_16bit(ft, dev):
    x16, sym, blank = inputs(36, "bf16", True)
    symd, bd = torch.from_numpy(sym).to(dev), torch.from_numpy(BOUNDARY).to(dev)
    rg = torch.from_numpy(band_ranges()).to(dev)
    am = torch.zeros((B, T, 36), dtype=torch.bfloat16, device=dev)
    lm = torch.zeros((B, S + 1, 36), dtype=torch.bfloat16, device=dev)
    with pytest.raises(TypeError):
        ft.do_rnnt_pruning(am, lm, rg)
    with pytest.raises(TypeError):
        ft.rnnt_loss_simple(lm, am, symd, blank, bd)
    with pytest.raises(TypeError):
        ft.rnnt_loss_multiblank_pruned(x16.to(dev), symd, rg, blank, ((1, 2),), bd)
    with pytest.raises(TypeError):
        ft.rnnt_loss_tdt_pruned(x16.to(dev), symd, rg, blank, (0, 1), bd)
    with pytest.raises(TypeError):
        ft.rnnt_loss_pruned(x16.to(dev).double(), symd, rg, blank, bd)
