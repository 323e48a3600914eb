"""Memory geometry of caller tensors: every public op, forward and backward, fed views instead of fresh allocations.

The rest of the suite hands the kernels fresh, contiguous, 16-byte-aligned tensors.  A training loop hands them slices of
packed batches, outputs of ``torch.split``, permuted and expanded tensors, int64 index tensors.  ``relayout`` rebuilds a
tensor with the same VALUES in one of these layouts:

  off1/off2/off3  a contiguous view 1, 2 or 3 elements into a larger buffer: ``.contiguous()`` in the wrappers passes it
                  through unchanged and the kernel gets a base pointer that is 4-byte but not 16-byte aligned (the f4u
                  accesses of csrc/ftr_common.h; for int32 ``ranges`` the scalar branch of do_pruning_bwd_lm_kernel)
  perm            a non-contiguous permutation of a buffer laid out in the reverse dimension order
  slice           ``wide[..., :n]`` of a buffer with a longer last dimension
  i64             int64 copies of the integer tensors (symbols, ranges, boundary)
  expand          stride 0 (separate tests below: equal rows of lm, the am_pruned view of do_rnnt_pruning, upstream gradients)

The comparison point is the same call on fresh contiguous 16-byte-aligned clones (layout "aligned").  The values are
identical and no kernel chooses a summation order by the alignment of a float operand, so outputs and gradients must match
BIT FOR BIT, and a gradient must have its input's shape.  No op needed the normwise fallback.

Two things are pinned so that the two runs of a pair take the same code: FTR_GEMM_TUNE=off (the library otherwise swaps
the rocBLAS kernel of a shape at its second call, which changes the summation order between ANY two calls, aligned or
not), and, in the smoothed tests only, torch's deterministic ``index_add_`` (the [C]-sized unigram statistic of the
smoothed backward is a torch op that otherwise adds with atomics in arbitrary order).
"""
import functools

import numpy as np
import pytest
import torch

from helpers import synthetic

pytestmark = pytest.mark.gpu

B, S, R = 3, 9, 4
# C: 12 (vector rows, one quad per lane), 501 (scalar rows: 4-byte-aligned rows even in an aligned tensor), 516 (vector rows,
# more than 64 quads + the two-sweep kernels); T: 36 and 33 (the fused d am kernel's T % 4 rule); the last shape is the
# smallest one of test_fused_builder_matches_library_gemm_route (fused builder) and is also run on the segmented band route.
SHAPES = [(36, 12), (33, 501), (36, 516), (33, 516)]
LAYOUTS = ["off1", "off2", "off3", "perm", "slice", "i64"]
BIG_BLANKS = ((1, 2), (2, 4), (3, 8))
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _same_gemm_kernel_in_both_runs(monkeypatch):
    monkeypatch.setenv("FTR_GEMM_TUNE", "off")
    monkeypatch.delenv("FTR_PRUNED_ROUTE", raising=False)
    monkeypatch.delenv("FTR_BAND_IMPL", raising=False)


# ------------------------------------------------------------------------------------------------------------ layouts
def relayout(t, layout):
    """`t`'s values in the given layout (see the module docstring); the result shares no memory with `t`."""
    n, shape = t.numel(), tuple(t.shape)
    if layout == "i64":
        layout = "aligned"
        if t.dtype == torch.int32:
            t = t.to(torch.int64)
    if layout == "aligned":
        v = t.clone(memory_format=torch.contiguous_format)
        assert v.is_contiguous() and v.storage_offset() == 0 and v.data_ptr() % 16 == 0
    elif layout in ("off1", "off2", "off3"):
        k = int(layout[3])
        buf = torch.empty(n + 8, dtype=t.dtype, device=t.device)
        assert buf.data_ptr() % 16 == 0
        v = buf[k:k + n].view(shape)
        v.copy_(t)
        assert v.is_contiguous() and v.storage_offset() == k
        if t.element_size() == 4:
            assert v.data_ptr() % 16 != 0 and v.data_ptr() % 4 == 0
    elif layout == "perm":
        if t.dim() >= 2 and sum(s > 1 for s in shape) >= 2:
            dims = tuple(reversed(range(t.dim())))
            v = torch.empty(tuple(shape[d] for d in dims), dtype=t.dtype, device=t.device).permute(dims)
        else:                       # nothing to permute: every other element of a buffer twice as long
            v = torch.empty(2 * max(n, 1), dtype=t.dtype, device=t.device)[::2][:n].view(shape) if t.dim() <= 1 else \
                torch.empty(shape + (2,), dtype=t.dtype, device=t.device)[..., 0]
        v.copy_(t)
        assert tuple(v.shape) == shape and (n <= 1 or not v.is_contiguous())
    elif layout == "slice":
        if t.dim() == 0:
            return relayout(t, "perm")
        wide = torch.empty(shape[:-1] + (shape[-1] + 3,), dtype=t.dtype, device=t.device)
        v = wide[..., :shape[-1]]
        v.copy_(t)
        assert tuple(v.shape) == shape and (n == shape[-1] or not v.is_contiguous())
    else:
        raise ValueError(layout)
    assert torch.equal(v.to(t.dtype) if v.dtype != t.dtype else v, t)
    return v.detach()


def _bits(a):
    a = a.detach().contiguous()
    return a.view(torch.int32) if a.dtype == torch.float32 else a


def assert_bit_identical(got, ref, what):
    assert len(got) == len(ref), what
    for i, (g, r) in enumerate(zip(got, ref)):
        assert tuple(g.shape) == tuple(r.shape) and g.dtype == r.dtype, f"{what}[{i}]: {tuple(g.shape)} {g.dtype} vs {tuple(r.shape)} {r.dtype}"
        if not torch.equal(_bits(g), _bits(r)):
            d = (g.double() - r.double()).abs()
            raise AssertionError(f"{what}[{i}]: not bit-identical to the aligned contiguous run: "
                                 f"{int((_bits(g) != _bits(r)).sum())} of {g.numel()} elements differ, max|d| = {float(torch.nan_to_num(d).max()):.3g}")


def _upstream(shape, i):
    g = torch.Generator(device="cpu").manual_seed(4242 + i)
    return torch.randn(tuple(shape), generator=g).to(DEV)


def execute(fn, tensors, diff, layout, up_layout):
    """fn(**tensors) with every tensor in `layout`; backward into the tensors named in `diff` with a random upstream
    gradient in `up_layout` handed to the autograd node as it is ("sum": the stride-0 gradients that
    ``sum(o.sum()).backward()`` produces; its aligned twin is a dense tensor of ones).  Returns outputs + gradients."""
    leaves = {}
    for k, v in tensors.items():
        v = relayout(v, layout)
        leaves[k] = v.requires_grad_(True) if k in diff else v
    outs = fn(**leaves)
    outs = [outs] if isinstance(outs, torch.Tensor) else list(outs)
    fouts = [o for o in outs if o.requires_grad]
    assert bool(fouts) == bool(diff)
    if fouts:
        if up_layout == "sum":
            sum(o.sum() for o in fouts).backward()
        elif up_layout == "ones":
            torch.autograd.backward(fouts, [torch.ones_like(o, memory_format=torch.contiguous_format) for o in fouts])
        else:
            torch.autograd.backward(fouts, [relayout(_upstream(o.shape, i), up_layout) for i, o in enumerate(fouts)])
    grads = []
    for k in diff:
        g = leaves[k].grad
        assert g is not None and tuple(g.shape) == tuple(leaves[k].shape), f"gradient of {k}: {None if g is None else tuple(g.shape)}"
        grads.append(g)
    torch.cuda.synchronize()
    return [o.detach() for o in outs] + grads


def check(fn, tensors, diff=(), layout="aligned", up_layout="aligned", what=""):
    ref = execute(fn, tensors, diff, "aligned", "ones" if up_layout == "sum" else "aligned")
    got = execute(fn, tensors, diff, layout, up_layout)
    assert_bit_identical(got, ref, f"{what} [{layout}, upstream {up_layout}]")
    return got


def check_all(fn, tensors, diff, layout, what):
    """The layout on the inputs (dense aligned upstream); for "perm" also the node's two upstream cases: a permuted
    upstream gradient and the stride-0 one of ``(px.sum() + py.sum()).backward()``, on aligned inputs."""
    got = check(fn, tensors, diff, layout, "aligned", what)
    if diff and layout == "perm":
        check(fn, tensors, diff, "aligned", "perm", what)
        check(fn, tensors, diff, "aligned", "sum", what)
    return got


# --------------------------------------------------------------------------------------------------------------- data
@functools.lru_cache(maxsize=None)
def _data(T, C):
    import tf_fast_rnnt as ft
    d = synthetic(7000 + T + C, B, T, S, C, ragged=True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    am, lm, sym, bd = t(d["am"]), t(d["lm"]), t(d["symbols"]), t(d["boundary"])
    blank = d["termination_symbol"]
    o = dict(am=am, lm=lm, sym=sym, bd=bd, blank=blank)
    for name, rt in (("reg", "regular"), ("mod", "modified")):
        px, py = ft.get_rnnt_logprobs(lm, am, sym, blank, rnnt_type=rt, boundary=bd)
        _, (gx, gy) = ft.rnnt_loss_simple(lm, am, sym, blank, boundary=bd, rnnt_type=rt, reduction="sum", calc_gradients=True)
        ranges = ft.get_rnnt_prune_ranges(gx, gy, bd, R)
        o[name] = dict(px=px.detach(), py=py.detach(), gx=gx, gy=gy, ranges=ranges)
    g = torch.Generator(device="cpu").manual_seed(T * 1000 + C)
    o["logits"] = (torch.randn((B, T, R, C), generator=g) * 2).to(DEV)
    o["joint"] = (torch.randn((B, T, S + 1, min(C, 20)), generator=g) * 2).to(DEV)
    o["sym_joint"] = sym % (min(C, 20) - 1)
    o["sym_mb"] = 4 + sym % (C - 5)                     # in [4, C-2]: not a blank of BIG_BLANKS with blank = 0
    o["py_mb"] = (torch.randn((B, 1 + len(BIG_BLANKS), S + 1, T), generator=g) - 1.0).to(DEV)
    return o


shape_layout = pytest.mark.parametrize("layout", LAYOUTS)
shapes = pytest.mark.parametrize("T,C", SHAPES)
types = pytest.mark.parametrize("rnnt_type", ["regular", "modified"])


def test_relayout_builds_what_it_says(dev):
    x = torch.arange(3 * 5 * 7, dtype=torch.float32, device=dev).reshape(3, 5, 7)
    i = torch.arange(12, dtype=torch.int32, device=dev).reshape(3, 4)
    for k in (1, 2, 3):
        v = relayout(x, f"off{k}")
        assert v.data_ptr() % 16 == 4 * k and v.is_contiguous() and torch.equal(v, x)
        assert relayout(i, f"off{k}").data_ptr() % 16 == 4 * k
    assert not relayout(x, "perm").is_contiguous() and not relayout(x, "slice").is_contiguous()
    assert not relayout(i, "perm").is_contiguous() and not relayout(x[0, 0], "perm").is_contiguous()
    assert relayout(i, "i64").dtype == torch.int64 and relayout(x, "i64").dtype == torch.float32


# ---------------------------------------------------------------------------------------------------- recursion family
@shape_layout
@types
@pytest.mark.parametrize("T", [33, 36])
def test_mutual_information_recursion(ft, dev, T, rnnt_type, layout):
    L = _data(T, 12)["reg" if rnnt_type == "regular" else "mod"]
    fn = lambda px, py, bd: (lambda r: (r[0], *r[1]))(ft.mutual_information_recursion(px, py, bd, calc_gradients=True))
    check_all(fn, dict(px=L["px"], py=L["py"], bd=_data(T, 12)["bd"]), ("px", "py"), layout, "mutual_information_recursion")


@shape_layout
@pytest.mark.parametrize("T", [33, 36])
def test_mutual_information_recursion_multiblank(ft, dev, T, layout):
    D = _data(T, 12)
    fn = lambda px, py, bd: (lambda r: (r[0], *r[1]))(ft.mutual_information_recursion_multiblank(px, py, (1, 2, 4, 8), bd, calc_gradients=True))
    check_all(fn, dict(px=D["reg"]["px"], py=D["py_mb"], bd=D["bd"]), ("px", "py"), layout, "mutual_information_recursion_multiblank")


@shape_layout
@types
def test_mutual_information_viterbi(ft, dev, rnnt_type, layout):
    D = _data(33, 12)
    L = D["reg" if rnnt_type == "regular" else "mod"]
    check_all(lambda px, py, bd: ft.mutual_information_viterbi(px, py, bd), dict(px=L["px"], py=L["py"], bd=D["bd"]), (), layout, "viterbi")


@pytest.mark.parametrize("layout", [l for l in LAYOUTS if l != "i64"])     # the op is registered for int32 only
@pytest.mark.parametrize("cols", [33, 64, 130])
def test_cummin(ft, dev, cols, layout):
    x = torch.randint(-50, 50, (7, cols), generator=torch.Generator(device="cpu").manual_seed(cols), dtype=torch.int32).to(dev)
    got = check_all(ft.cummin, dict(x=x), (), layout, "cummin")
    assert torch.equal(got[0], torch.cummin(x.long(), dim=1).values.int())


# ---------------------------------------------------------------------------------------------- simple / smoothed family
@shape_layout
@types
@shapes
def test_get_rnnt_logprobs(ft, dev, T, C, rnnt_type, layout):
    D = _data(T, C)
    fn = lambda lm, am, sym, bd: ft.get_rnnt_logprobs(lm, am, sym, D["blank"], rnnt_type=rnnt_type, boundary=bd)
    check_all(fn, dict(lm=D["lm"], am=D["am"], sym=D["sym"], bd=D["bd"]), ("lm", "am"), layout, "get_rnnt_logprobs")


@shape_layout
@pytest.mark.parametrize("bwd", ["library", "fused"])
@types
@shapes
def test_rnnt_loss_simple(ft, dev, T, C, rnnt_type, bwd, layout, monkeypatch):
    """calc_gradients=True; both routes of the backward towards am (the fused one needs C % 4 == 0 and has a T % 4 rule,
    FTR_BUILDER_BWD=fused falls back to the library route where it does not apply)."""
    monkeypatch.setenv("FTR_BUILDER_BWD", bwd)
    D = _data(T, C)

    def fn(lm, am, sym, bd):
        loss, (gx, gy) = ft.rnnt_loss_simple(lm, am, sym, D["blank"], boundary=bd, rnnt_type=rnnt_type, delay_penalty=0.1,
                                             reduction="none", calc_gradients=True)
        return loss, gx, gy
    check_all(fn, dict(lm=D["lm"], am=D["am"], sym=D["sym"], bd=D["bd"]), ("lm", "am"), layout, "rnnt_loss_simple")


@pytest.fixture
def deterministic_torch_ops():
    torch.use_deterministic_algorithms(True, warn_only=True)
    yield
    torch.use_deterministic_algorithms(False)


@shape_layout
@pytest.mark.parametrize("op", ["logprobs", "loss"])
@shapes
def test_smoothed(ft, dev, T, C, op, layout, deterministic_torch_ops):
    D = _data(T, C)

    def fn(lm, am, sym, bd):
        if op == "logprobs":
            return ft.get_rnnt_logprobs_smoothed(lm, am, sym, D["blank"], lm_only_scale=0.1, am_only_scale=0.2, boundary=bd)
        loss, (gx, gy) = ft.rnnt_loss_smoothed(lm, am, sym, D["blank"], lm_only_scale=0.1, am_only_scale=0.2, boundary=bd,
                                               delay_penalty=0.1, reduction="none", calc_gradients=True)
        return loss, gx, gy
    check_all(fn, dict(lm=D["lm"], am=D["am"], sym=D["sym"], bd=D["bd"]), ("lm", "am"), layout, f"smoothed {op}")


# ------------------------------------------------------------------------------------------------------- prune family
@shape_layout
@types
@pytest.mark.parametrize("T", [33, 36])
def test_get_rnnt_prune_ranges(ft, dev, T, rnnt_type, layout):
    D = _data(T, 12)
    L = D["reg" if rnnt_type == "regular" else "mod"]
    got = check_all(lambda gx, gy, bd: ft.get_rnnt_prune_ranges(gx, gy, bd, R), dict(gx=L["gx"], gy=L["gy"], bd=D["bd"]), (), layout,
                    "get_rnnt_prune_ranges")
    assert got[0].dtype == torch.int32 and torch.equal(got[0], L["ranges"])


@shape_layout
@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("r", [4, 5])
@shapes
def test_do_rnnt_pruning(ft, dev, T, C, r, dense, layout):
    """Forward and backward.  C = 501 takes do_pruning_bwd_lm_kernel, whose scan of `ranges` switches between 16-byte and
    scalar loads on the alignment of each utterance's rows: with T * r = 132 or 144 every utterance of an aligned tensor
    takes the 16-byte branch, with T * r = 165 or 180 (r = 5) some do, and at offsets 1..3 all take the scalar one."""
    D = _data(T, C)
    ranges = ft.get_rnnt_prune_ranges(D["reg"]["gx"], D["reg"]["gy"], D["bd"], r)
    fn = lambda am, lm, ranges: ft.do_rnnt_pruning(am, lm, ranges, dense=dense)
    got = check_all(fn, dict(am=D["am"], lm=D["lm"], ranges=ranges), ("am", "lm"), layout, "do_rnnt_pruning")
    assert got[0].is_contiguous() == dense


PRUNED_ROUTES = ["band", "segments", "lattice"]


def _set_route(monkeypatch, route):
    """As test_gpu_pipeline.py selects them; "segments" is the band route through mi_band_seg.hip."""
    monkeypatch.setenv("FTR_PRUNED_ROUTE", "lattice" if route == "lattice" else "band")
    if route == "segments":
        monkeypatch.setenv("FTR_BAND_IMPL", "segments")


@shape_layout
@pytest.mark.parametrize("hat", [False, True])
@types
@shapes
def test_pruned_logprobs(ft, dev, T, C, rnnt_type, hat, layout):
    D = _data(T, C)
    f = ft.get_hat_logprobs_pruned if hat else ft.get_rnnt_logprobs_pruned
    fn = lambda logits, sym, ranges, bd: f(logits, sym, ranges, D["blank"], bd, rnnt_type=rnnt_type)
    tensors = dict(logits=D["logits"], sym=D["sym"], ranges=D["reg" if rnnt_type == "regular" else "mod"]["ranges"], bd=D["bd"])
    check_all(fn, tensors, ("logits",), layout, "hat pruned logprobs" if hat else "pruned logprobs")


@shape_layout
@pytest.mark.parametrize("route", PRUNED_ROUTES)
@pytest.mark.parametrize("hat", [False, True])
@types
@shapes
def test_pruned_loss(ft, dev, T, C, rnnt_type, hat, route, layout, monkeypatch):
    _set_route(monkeypatch, route)
    D = _data(T, C)
    f = ft.hat_loss_pruned if hat else ft.rnnt_loss_pruned
    seen = []

    def fn(logits, sym, ranges, bd):
        loss = f(logits, sym, ranges, D["blank"], bd, rnnt_type=rnnt_type, delay_penalty=0.1, reduction="none")
        seen.append(loss.grad_fn.band)
        return loss
    tensors = dict(logits=D["logits"], sym=D["sym"], ranges=D["reg" if rnnt_type == "regular" else "mod"]["ranges"], bd=D["bd"])
    check_all(fn, tensors, ("logits",), layout, f"pruned loss hat={hat} {route}")
    assert all(b == (route != "lattice") for b in seen), seen      # every copy of the ranges took the route of the original


def test_band_mark_survives_dtype_and_layout_copies(ft, dev):
    """rnnt_loss.py, _pruned_inputs: the int32 contiguous copy that the wrapper makes of a MARKED int64 / non-contiguous
    ranges tensor keeps the mark (no device-side check, hence no host read: the call stays capturable), an offset view
    passes through as the same object, and an unmarked copy is recognised as a band by its data.  Same route, same bits."""
    from tf_fast_rnnt.rnnt_loss import _band_mark_valid, _mark_band, _pruned_inputs
    D = _data(36, 12)
    ranges = D["reg"]["ranges"]
    assert _band_mark_valid(ranges)
    ref = None
    for layout in ("aligned", "i64", "off1", "perm", "slice"):
        for marked in (False, True):
            rg = relayout(ranges, layout)
            assert not _band_mark_valid(rg)
            if marked:
                _mark_band(rg)
                _, inner, _ = _pruned_inputs(D["logits"], D["sym"], rg, D["bd"])
                assert inner.dtype == torch.int32 and inner.is_contiguous() and _band_mark_valid(inner), (layout, marked)
                assert (inner is rg) == (layout in ("aligned", "off1"))
            x = D["logits"].clone().requires_grad_(True)
            loss = ft.rnnt_loss_pruned(x, D["sym"], rg, D["blank"], D["bd"], reduction="none")
            assert loss.grad_fn.band is True, (layout, marked)
            loss.sum().backward()
            out = [loss.detach(), x.grad]
            if ref is None:
                ref = out
            assert_bit_identical(out, ref, f"ranges {layout} marked={marked}")


@shape_layout
@pytest.mark.parametrize("op", ["joint_logprobs", "rnnt_loss", "hat_loss"])
@types
@pytest.mark.parametrize("T", [33, 36])
def test_joint(ft, dev, T, rnnt_type, op, layout):
    D = _data(T, 12)
    Cj = D["joint"].shape[3]

    def fn(logits, sym, bd):
        if op == "joint_logprobs":
            return ft.get_rnnt_logprobs_joint(logits, sym, Cj - 1, boundary=bd, rnnt_type=rnnt_type)
        f = ft.rnnt_loss if op == "rnnt_loss" else ft.hat_loss
        return f(logits, sym, Cj - 1, boundary=bd, rnnt_type=rnnt_type, delay_penalty=0.1, reduction="none")
    check_all(fn, dict(logits=D["joint"], sym=D["sym_joint"], bd=D["bd"]), ("logits",), layout, op)


@shape_layout
@pytest.mark.parametrize("op", ["logprobs", "loss"])
@shapes
def test_multiblank_pruned(ft, dev, T, C, op, layout):
    D = _data(T, C)

    def fn(logits, sym, ranges, bd):
        if op == "logprobs":
            return ft.get_rnnt_logprobs_multiblank_pruned(logits, sym, ranges, 0, BIG_BLANKS, bd, sigma=0.05)
        return ft.rnnt_loss_multiblank_pruned(logits, sym, ranges, 0, BIG_BLANKS, bd, sigma=0.05, delay_penalty=0.1, reduction="none")
    tensors = dict(logits=D["logits"], sym=D["sym_mb"], ranges=D["reg"]["ranges"], bd=D["bd"])
    check_all(fn, tensors, ("logits",), layout, f"multiblank {op}")


@shape_layout
@types
@shapes
def test_rnnt_alignment_pruned(ft, dev, T, C, rnnt_type, layout):
    D = _data(T, C)
    fn = lambda logits, sym, ranges, bd: ft.rnnt_alignment_pruned(logits, sym, ranges, D["blank"], bd, rnnt_type=rnnt_type)
    tensors = dict(logits=D["logits"], sym=D["sym"], ranges=D["reg" if rnnt_type == "regular" else "mod"]["ranges"], bd=D["bd"])
    got = check_all(fn, tensors, (), layout, "rnnt_alignment_pruned")
    assert got[1].dtype == torch.int32


# ----------------------------------------------------------------------------------------------------------- stride 0
def _grads(fn, leaves):
    leaves = [v.detach().requires_grad_(True) for v in leaves]
    outs = fn(*leaves)
    outs = [outs] if isinstance(outs, torch.Tensor) else list(outs)
    fouts = [o for o in outs if o.requires_grad]
    torch.autograd.backward(fouts, [_upstream(o.shape, i) for i, o in enumerate(fouts)])
    for v in leaves:
        assert tuple(v.grad.shape) == tuple(v.shape)
    torch.cuda.synchronize()
    return [o.detach() for o in outs] + [v.grad for v in leaves]


@pytest.mark.parametrize("which", ["lm_batch", "am_frames"])
@shapes
def test_expanded_inputs_of_the_simple_family(ft, dev, T, C, which, deterministic_torch_ops):
    """lm with the same rows for every utterance (``lm[:1].expand``: stride 0 along the batch), am with the same row for
    every frame (stride 0 along T), against the materialised tensors: builder, simple and smoothed loss, prune gather."""
    D = _data(T, C)
    if which == "lm_batch":
        lm_e, am_e = D["lm"][:1].expand(B, S + 1, C), D["am"]
    else:
        lm_e, am_e = D["lm"], D["am"][:, :1].expand(B, T, C)
    assert 0 in lm_e.stride() + am_e.stride()
    lm_d, am_d = relayout(lm_e, "aligned"), relayout(am_e, "aligned")
    sym, bd, blank, ranges = D["sym"], D["bd"], D["blank"], D["reg"]["ranges"]
    fns = dict(
        logprobs=lambda lm, am: ft.get_rnnt_logprobs(lm, am, sym, blank, boundary=bd),
        simple=lambda lm, am: ft.rnnt_loss_simple(lm, am, sym, blank, boundary=bd, reduction="none"),
        smoothed=lambda lm, am: ft.rnnt_loss_smoothed(lm, am, sym, blank, lm_only_scale=0.1, am_only_scale=0.2, boundary=bd, reduction="none"),
        pruning=lambda lm, am: ft.do_rnnt_pruning(am, lm, ranges),
        pruning_dense=lambda lm, am: ft.do_rnnt_pruning(am, lm, ranges, dense=True))
    for name, fn in fns.items():
        assert_bit_identical(_grads(fn, [lm_e, am_e]), _grads(fn, [lm_d, am_d]), f"{name} with {which} expanded")


@pytest.mark.parametrize("route", PRUNED_ROUTES)
@shapes
def test_am_pruned_view_through_the_joiner_and_back(ft, dev, T, C, route, monkeypatch):
    """The stride-0 am_pruned that do_rnnt_pruning returns: (a) consumed by ``am_pruned + lm_pruned`` and the pruned loss,
    the gradient flowing back through the gather's backward, against the dense=True tensors; (b) fed to the pruned loss
    as the logits themselves, against its materialised copy."""
    _set_route(monkeypatch, route)
    D = _data(T, C)
    sym, bd, blank, ranges = D["sym"], D["bd"], D["blank"], D["reg"]["ranges"]

    def step(dense):
        def fn(am, lm):
            am_p, lm_p = ft.do_rnnt_pruning(am, lm, ranges, dense=dense)
            assert am_p.is_contiguous() == dense and (dense or am_p.stride(2) == 0)
            return ft.rnnt_loss_pruned(torch.tanh(am_p + lm_p), sym, ranges, blank, bd, delay_penalty=0.1, reduction="none")
        return _grads(fn, [D["am"], D["lm"]])
    assert_bit_identical(step(False), step(True), "joiner on the am_pruned view")

    am_p, _ = ft.do_rnnt_pruning(D["am"], D["lm"], ranges)
    fn = lambda x: ft.rnnt_loss_pruned(x, sym, ranges, blank, bd, reduction="none")
    assert_bit_identical(_grads(fn, [am_p]), _grads(fn, [am_p.contiguous()]), "am_pruned view as logits")


@pytest.mark.parametrize("dense", [False, True])
@shapes
def test_do_rnnt_pruning_backward_with_stride0_upstream(ft, dev, T, C, dense):
    """Upstream gradients of the gather that are themselves stride-0: the ones of ``(am_p.sum() + lm_p.sum()).backward()``,
    a gradient expanded along s_range (what the am_pruned view's own consumers send back), and one and the same tensor for
    both outputs (the joiner's ``am_pruned + lm_pruned``: the fused branch of the segmented backward)."""
    D = _data(T, C)
    ranges = D["reg"]["ranges"]
    g3 = _upstream((B, T, 1, C), 0).expand(B, T, R, C)
    g4 = _upstream((B, T, R, C), 1)
    cases = dict(sum=lambda a, l: (a.sum() + l.sum()).backward(),
                 expanded=lambda a, l: torch.autograd.backward([a, l], [g3, g4]),
                 same=lambda a, l: torch.autograd.backward([a, l], [g4, g4]))
    dense_twin = dict(sum=lambda a, l: torch.autograd.backward([a, l], [torch.ones((B, T, R, C), device=dev)] * 2),
                      expanded=lambda a, l: torch.autograd.backward([a, l], [g3.contiguous(), g4.clone()]),
                      same=lambda a, l: torch.autograd.backward([a, l], [g4.clone(), g4.clone()]))

    def run(back):
        am = D["am"].clone().requires_grad_(True); lm = D["lm"].clone().requires_grad_(True)
        back(*ft.do_rnnt_pruning(am, lm, ranges, dense=dense))
        assert am.grad.shape == am.shape and lm.grad.shape == lm.shape
        return [am.grad, lm.grad]
    for name in cases:
        # ("same": FUSE takes d am from the registers that hold the r rows, in the k order of do_pruning_bwd_am_kernel)
        assert_bit_identical(run(cases[name]), run(dense_twin[name]), f"do_rnnt_pruning backward, upstream {name}")
