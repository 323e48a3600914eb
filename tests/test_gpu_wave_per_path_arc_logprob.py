"""rnnt_path_logprob_pruned against a plain float64 torch restatement on logits.float().double(): log_softmax (HAT: logsigmoid
and a masked log_softmax), a Python loop over the path's arcs, autograd.  B = 2, T = 12, S = 5, s_range = 3, utterance 1 ragged.
Bounds: logprob 4 x the error of the SAME restatement in float32, floored at 2^-20 |want|; a gradient element u |want| +
m 2^-24 |up|, u the dtype's unit roundoff, m = 4 x the float32 restatement's worst ratio.  Figures are printed (PATHERR) before
they are asserted.  Three band rows hold at most TWO symbol arcs and a frame's blank arc: the hand path has two in one frame."""
import json

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

B, T, S, R = 2, 12, 5, 3
DTYPES = {"f32": (torch.float32, 2.0 ** -24), "bf16": (torch.bfloat16, 2.0 ** -8), "fp16": (torch.float16, 2.0 ** -11)}
VOCABS = [8, 36, 37, 260, 2052]   # fewer quads than lanes; vector path, partial wave; element by element; first NQ = 2; past the registers
RAGGED = [[0, 0, 5, 12], [0, 0, 3, 9]]
OFFSET = [[1, 2, 5, 12], [0, 0, 3, 9]]
S0 = [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3]
HAND = [[1, 1, 5, 8, 11], [1, 1, 8, 0, 0]]      # regular: two symbols in frame 1, one in the utterance's last frame
STRICT = [[1, 2, 5, 8, 11], [1, 2, 8, 0, 0]]    # strictly increasing: a path of either type
UP = [1.5, -0.75]
NINF = float("-inf")


def band():
    return (torch.tensor(S0)[None, :, None] + torch.arange(R)[None, None, :]).expand(B, T, R).contiguous().to(torch.int32)


def inputs(C, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + C)
    x = (2.0 * torch.randn((B, T, R, C), generator=g)).to(dtype)
    blank = C - 3
    sym = torch.randint(0, C, (B, S), generator=g)
    sym[sym == blank] = 0                      # HAT gives a symbol that is the blank no mass
    return x, sym.to(torch.int32), blank


def arcs_of(frames, ranges, bd, modified):
    """[(t, k, is_blank, s)] of one utterance's path, or None when it is not a path"""
    sb, tb, se, te = bd
    f = [int(v) for v in frames[sb:se]]
    if any(not tb <= v < te for v in f) or any(b < a or (modified and b == a) for a, b in zip(f, f[1:])):
        return None
    nodes = [(sb + i, v, False) for i, v in enumerate(f)]
    for t in range(tb, te):
        if not (modified and t in f):
            nodes.append((sb + sum(v < t if modified else v <= t for v in f), t, True))
    out = []
    for s, t, is_blank in nodes:
        slots = [k for k in range(ranges.shape[1]) if int(ranges[t, k]) == s]
        if not slots:
            return None
        out.append((t, slots[0], is_blank, s))
    return out


def restate(x, sym, ranges, frames, bd, blank, modified, hat):
    """logprob [B] in the dtype of x (float64 or float32), differentiable"""
    C = x.shape[-1]
    if hat:
        mask = torch.arange(C) == blank
        lp_sym = F.logsigmoid(-x[..., blank:blank + 1]) + torch.log_softmax(x.masked_fill(mask, NINF), -1)
        lp_blank = F.logsigmoid(x)
    else:
        lp_sym = lp_blank = torch.log_softmax(x, -1)
    out = []
    for b in range(x.shape[0]):
        arcs = arcs_of(frames[b], ranges[b], bd[b], modified)
        if arcs is None:
            out.append(x.new_tensor(NINF))
            continue
        terms = [lp_blank[b, t, k, blank] if is_blank else lp_sym[b, t, k, min(max(int(sym[b, s]), 0), C - 1)] for t, k, is_blank, s in arcs]
        out.append(torch.stack(terms).sum() if terms else x.new_tensor(0.0))
    return torch.stack(out)


def restate_grad(x, *args):
    x = x.clone().requires_grad_(True)
    lp = restate(x, *args)
    live = torch.isfinite(lp.detach())
    g = torch.autograd.grad((lp[live] * x.new_tensor(UP)[live]).sum(), x)[0] if live.any() else torch.zeros_like(x)
    return lp.detach(), g


def run(ft, dev, x, sym, ranges, frames, bd, blank, typ, fact):
    xd = x.to(dev).requires_grad_(True)
    lp = ft.rnnt_path_logprob_pruned(xd, sym.to(dev), ranges.to(dev), blank, torch.as_tensor(frames).to(dev),
                                     None if bd is None else torch.tensor(bd, dtype=torch.int32, device=dev), typ, fact)
    lp.backward(torch.tensor(UP, device=dev))
    assert lp.dtype == torch.float32 and xd.grad.dtype == x.dtype
    return lp.detach().cpu(), xd.grad.cpu()


def bounds(x, sym, ranges, frames, bd, blank, typ, fact, u):
    """(want, gwant, tol_lp [B], tol_grad like x) from the float64 and float32 restatements of the same inputs"""
    args = (sym, ranges, torch.as_tensor(frames), bd, blank, typ == "modified", fact == "hat")
    want, gwant = restate_grad(x.float().double(), *args)
    lp32, g32 = restate_grad(x.float(), *args)
    up = torch.tensor(UP, dtype=torch.float64).abs().view(-1, 1, 1, 1)
    own_lp = (lp32.double() - want).abs()
    own_g = ((g32.double() - gwant).abs() / (2.0 ** -24 * up)).max().item()
    tol_lp = torch.maximum(4 * own_lp, 2.0 ** -20 * want.abs())
    return want, gwant, tol_lp, u * gwant.abs() + 4 * own_g * 2.0 ** -24 * up, own_lp, own_g


def check(ft, dev, x, sym, ranges, frames, bd, blank, typ, fact, u, tag):
    want, gwant, tol_lp, tol_g, own_lp, own_g = bounds(x, sym, ranges, frames, bd, blank, typ, fact, u)
    lp, g = run(ft, dev, x, sym, ranges, frames, bd, blank, typ, fact)
    err_lp, err_g = (lp.double() - want).abs(), (g.double() - gwant).abs()
    print("PATHERR", json.dumps(dict(case=tag, lp_err=err_lp.max().item(), lp_own32=own_lp.max().item(), lp_tol=tol_lp.min().item(),
                                     grad_ratio=(err_g / tol_g.clamp_min(1e-300)).max().item(), grad_own32_units=own_g)))
    assert torch.isfinite(want).all() and (err_lp <= tol_lp).all(), (tag, lp, want, tol_lp)
    assert (err_g <= tol_g).all(), (tag, (err_g / tol_g.clamp_min(1e-300)).max())
    return lp, g, gwant


def best_path(ft, dev, x, sym, ranges, bd, blank, typ):
    score, frames = ft.rnnt_alignment_pruned(x.to(dev), sym.to(dev), ranges.to(dev), blank, torch.tensor(bd, dtype=torch.int32, device=dev), typ)
    return score.cpu(), frames.cpu()


@pytest.mark.parametrize("C", VOCABS)
@pytest.mark.parametrize("typ", ["regular", "modified"])
@pytest.mark.parametrize("fact", ["softmax", "hat"])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_parity_with_float64(ft, dev, dt, fact, typ, C):
    dtype, u = DTYPES[dt]
    x, sym, blank = inputs(C, dtype)
    ranges = band()
    tag = f"{dt}-{fact}-{typ}-C{C}"
    for name, bd in (("ragged", RAGGED), ("offset", OFFSET)):        # the model's own best path, s_begin = 1 / t_begin = 2 too
        score, frames = best_path(ft, dev, x, sym, ranges, bd, blank, typ)
        lp, _, _ = check(ft, dev, x, sym, ranges, frames, bd, blank, typ, fact, u, f"{tag}-best-{name}")
        if typ == "regular" and fact == "softmax":                   # two float32 routes to the same float64 value
            tol = bounds(x, sym, ranges, frames, bd, blank, typ, fact, u)[2]
            print("PATHERR", json.dumps(dict(case=f"{tag}-score-{name}", diff=(lp - score).abs().max().item(), tol=tol.min().item())))
            assert ((lp.double() - score.double()).abs() <= tol).all(), (tag, lp, score, tol)
    hand = STRICT if typ == "modified" else HAND
    lp, g, gwant = check(ft, dev, x, sym, ranges, hand, RAGGED, blank, typ, fact, u, f"{tag}-hand")
    off = (gwant == 0).all(-1)     # every row off the path is an exact zero, and is not read: NaN there changes nothing
    assert off.sum() >= B * T * R - B * (S + T) and torch.equal(g[off], torch.zeros_like(g[off]))
    xn = x.clone()
    xn[off] = float("nan")
    lpn, gn = run(ft, dev, xn, sym, ranges, hand, RAGGED, blank, typ, fact)
    assert torch.isfinite(lpn).all() and torch.equal(lpn, lp) and torch.equal(gn, g)
    perm = [2, 0, 1]               # ranges that are no band (rows permuted, the logits with them): the same rows are found
    lpp, gp = run(ft, dev, x[:, :, perm].contiguous(), sym, ranges[:, :, perm].contiguous(), hand, RAGGED, blank, typ, fact)
    assert torch.equal(lpp, lp) and torch.equal(gp, g[:, :, perm])


def _invalid(kind):
    """(frames, ranges, rnnt_type, the utterance that is hit) -- starting from the strictly increasing path"""
    frames, ranges, typ, hit = [list(STRICT[0]), list(STRICT[1])], band(), "regular", 0
    if kind == "decreasing":
        frames[0][2] = 1
    elif kind == "equal_modified":
        frames, typ = [list(HAND[0]), list(STRICT[1])], "modified"
    elif kind == "t_end_of_tensor":
        frames[0][4] = T                      # == t_end == T: the frame after the tensor's last
    elif kind == "t_end_ragged":
        frames[1][2], hit = 9, 1
    elif kind == "absent_row":
        ranges[0, 3] = torch.tensor([3, 4, 5], dtype=torch.int32)    # the blank arc of frame 3 leaves row 2
    return frames, ranges, typ, hit


@pytest.mark.parametrize("kind", ["decreasing", "equal_modified", "t_end_of_tensor", "t_end_ragged", "absent_row"])
@pytest.mark.parametrize("C", [36, 37])
def test_invalid_path_is_minus_inf_for_that_utterance_only(ft, dev, kind, C):
    x, sym, blank = inputs(C, torch.float32)
    frames, ranges, typ, hit = _invalid(kind)
    want = restate(x.double(), sym, ranges, torch.tensor(frames), RAGGED, blank, typ == "modified", False)
    assert want[hit] == NINF and torch.isfinite(want[1 - hit])        # exactly that utterance, by the restatement
    lp, g = run(ft, dev, x, sym, ranges, frames, RAGGED, blank, typ, "softmax")
    good_lp, good_g = run(ft, dev, x, sym, band(), STRICT, RAGGED, blank, typ, "softmax")
    assert lp[hit] == NINF and torch.equal(g[hit], torch.zeros_like(g[hit]))
    assert torch.equal(lp[1 - hit], good_lp[1 - hit]) and torch.equal(g[1 - hit], good_g[1 - hit])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_determinism_capture_refusals_and_views(ft, dev, dt):
    dtype, _ = DTYPES[dt]
    x, sym, blank = inputs(260, dtype)
    sym, ranges, frames = sym.to(dev), band().to(dev), torch.tensor(HAND, device=dev)
    bd, up = torch.tensor(RAGGED, dtype=torch.int32, device=dev), torch.tensor(UP, device=dev)
    xs = x.to(dev)

    def step(src=xs):
        xin = src.detach().requires_grad_(True)    # the leaf is made inside the step and only detached results leave it:
        lp = ft.rnnt_path_logprob_pruned(xin, sym, ranges, blank, frames, bd)    # DESIGN.md section 4e, "Graph capture"
        return lp.detach(), torch.autograd.grad(lp, xin, up)[0]

    eager = step()
    assert all(torch.equal(a, b) for a, b in zip(eager, step()))
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(eager, captured))
    # a strided view and a 16-bit base at an odd element give the values of their contiguous copy
    wide = torch.zeros((B, T, R, 2 * 260), dtype=dtype, device=dev)
    wide[..., ::2] = xs
    views = [wide[..., ::2]]
    if dtype != torch.float32:
        buf = torch.zeros(xs.numel() + 1, dtype=dtype, device=dev)
        buf[1:] = xs.reshape(-1)
        views.append(buf[1:].view(B, T, R, 260))
    for v in views:
        assert all(torch.equal(a, b) for a, b in zip(eager, step(v)))
    inverted = torch.tensor([[3, 0, 2, 12], [0, 5, 3, 4]], dtype=torch.int32, device=dev)    # no arcs at all
    assert torch.equal(ft.rnnt_path_logprob_pruned(xs, sym, ranges, blank, frames, inverted).cpu(), torch.zeros(B))
    call = lambda **kw: ft.rnnt_path_logprob_pruned(kw.pop("x", xs), sym, ranges, blank, kw.pop("frames", frames), bd, **kw)
    for kw, match in ((dict(rnnt_type="constrained"), "regular path with strictly increasing frames"), (dict(factorization="tdt"), "factorization"),
                      (dict(frames=frames[:, :4]), "frames must have the shape")):
        with pytest.raises(ValueError, match=match):
            call(**kw)
    with pytest.raises(TypeError, match="float32, bfloat16 or float16"):
        call(x=xs.double())
