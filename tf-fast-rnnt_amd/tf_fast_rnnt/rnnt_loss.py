"""The Python op surface of tf_fast_rnnt on MI355X: same names, keyword signatures, defaults and return
conventions as the reference's ``tf_fast_rnnt/python/tf_fast_rnnt/rnnt_loss.py`` (cited per function
as ``rnnt_loss.py:<lines>``), on torch tensors resident in HBM.

What runs where:
* ``mutual_information_recursion`` (every loss ends there), ``get_rnnt_prune_ranges``,
  ``do_rnnt_pruning``, ``get_rnnt_logprobs_pruned`` / ``rnnt_loss_pruned``: hand-written HIP behind the
  C ABI (include/ftr.h);
* ``get_rnnt_logprobs`` / ``rnnt_loss_simple``: hand-written HIP prologue, epilogue and backward kernels around
  the normaliser GEMM (rocBLAS behind ftr_normalizer_gemm_f32);
* ``get_rnnt_logprobs_smoothed`` / ``rnnt_loss_smoothed``: the same native kernels with the LM-only / AM-only
  terms folded in; only the [C]- and [rows]-sized batch statistics (unigram mean, two matvecs) are torch ops;
* ``get_rnnt_logprobs_joint`` / ``rnnt_loss`` (unpruned, joiner logits [B,T,S+1,C]): the pruned builder's kernels
  with identity ranges (s_range = S+1).
* ``get_hat_logprobs_pruned`` / ``get_hat_logprobs_joint`` / ``hat_loss_pruned`` / ``hat_loss`` (MI355X addition, no
  reference counterpart): the same kernels and routes with the HAT normalisation of the joiner output.
* ``rnnt_kd_loss_pruned`` (MI355X addition, no reference counterpart): knowledge distillation on the pruned band, two
  stream kernels of its own (include/ftr_kd.h, csrc/pruned_kd.hip); ``rnnt_kd_loss_pruned_factored``: the same for HAT and
  TDT rows and with node weights (include/ftr_kd_fact.h, the same kernels in their other two row forms);
  ``rnnt_kd_loss_pruned_topk``: the same loss from a stored top-K teacher on the teacher's own ranges (include/ftr_kd_topk.h,
  csrc/pruned_kd_topk.hip), ``rnnt_kd_topk_teacher`` (plain torch) writes that cache.

Reference bugs that are NOT reproduced: ``rnnt_loss_simple(reduction="mean")``
raises NameError there (rnnt_loss.py:331) -- here it is the mean; ``boundary=None`` works; the
non-regular ``rnnt_type`` values do not hit the shape error of rnnt_loss.py:211/440/1324 (the
normalisers are used unpadded, as upstream k2 does).
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import ctypes
import os
import weakref

import torch

from . import _lib
from .mutual_information import (_as_boundary, _ptr, _require_gpu, _stream_ptr, band_forward_backward, band_multiblank_forward_backward,
                                 band_multiblank_supported, band_tdt_forward_backward, band_tdt_supported, band_viterbi_supported, cummin, mb_forward_backward, mi_forward_backward,
                                 mutual_information_recursion, mutual_information_viterbi, mutual_information_viterbi_tdt, mutual_information_viterbi_tdt_band,
                                 tdt_forward_backward)

_NEG_INF = float("-inf")
# tf.math.nextafter(0., 1.) : smallest positive float32 subnormal (rnnt_loss.py:181,1272,1280)
_TINY = 1.401298464324817e-45


def tune_normalizer_gemms(enable: bool = True, filename: Optional[str] = None, search: bool = True, when: str = "second") -> None:
    """The dense contractions of the simple / smoothed builders that stay library f32 GEMMs (the two transposes of the
    normaliser product in the backward; also the forward one when C % 4 != 0, rnnt_loss.py:180-182) go through
    ``ftr_normalizer_gemm_f32`` (csrc/normalizer_gemm.hip): rocBLAS with the kernel chosen by MEASUREMENT -- rocBLAS' own
    choice for these shapes runs at 62-77 TFLOP/s on MI355X, its best candidate at ~100 (104/90/84 -> 65/62/60 us at B=32
    T=1000 S=200 C=500).  By default the library times the candidates at the second call with a shape (~0.2 s, never inside
    a stream capture), so a loop with fixed shapes gets the fast kernel from its second step on without calling anything
    and a ragged loop is never held up.  This function only moves that switch (the environment variable FTR_GEMM_TUNE):
    ``enable=False`` or ``search=False`` -> "off" (shapes already measured keep their kernel), ``when`` = "first" | "second".
    ``filename`` is accepted for compatibility and ignored (the choices live in the process; see
    ``normalizer_gemm_choice`` / ``set_normalizer_gemm_choice`` to carry one over)."""
    if when not in ("first", "second"):
        raise ValueError("when must be 'first' or 'second'")
    os.environ["FTR_GEMM_TUNE"] = when if (enable and search) else "off"


def normalizer_gemm_choice(kind: int, B: int, T: int, S: int, C: int):
    """What the library chose for the GEMM ``kind`` (0 forward product, 1 towards lm, 2 towards am) of this shape on the
    current device: None if the shape has not run, else dict(solution, us, us_default, candidates) -- solution 0 is
    rocBLAS' own choice, candidates -1 means not measured yet."""
    sol, cand = ctypes.c_int(0), ctypes.c_int(0)
    us, usd = ctypes.c_float(0), ctypes.c_float(0)
    if not _lib.lib().ftr_normalizer_gemm_choice(int(kind), int(B), int(T), int(S) + 1, int(C), ctypes.byref(sol), ctypes.byref(us),
                                                  ctypes.byref(usd), ctypes.byref(cand)):
        return None
    return dict(solution=sol.value, us=us.value, us_default=usd.value, candidates=cand.value)


def set_normalizer_gemm_choice(kind: int, B: int, T: int, S: int, C: int, solution: int) -> None:
    """Fixes the rocBLAS solution index for a shape without measuring (a choice recorded by an earlier process)."""
    _lib.call("ftr_normalizer_gemm_set_choice", int(kind), int(B), int(T), int(S) + 1, int(C), int(solution))


def _gemm(kind: int, x: torch.Tensor, y: torch.Tensor, B: int, T: int, S: int, C: int, st) -> torch.Tensor:
    """ftr_normalizer_gemm_f32: kind 0 lm_probs . am_probs^T -> [B,S+1,T]; 1 W . am_probs -> [B,S+1,C]; 2 W^T . lm_probs -> [B,T,C]."""
    shape = ((B, S + 1, T), (B, S + 1, C), (B, T, C))[kind]
    out = torch.empty(shape, dtype=torch.float32, device=x.device)
    _lib.call("ftr_normalizer_gemm_f32", kind, _ptr(x), _ptr(y), _ptr(out), B, T, S + 1, C, st)
    return out


def _check_type(rnnt_type: str) -> None:
    if rnnt_type not in ("regular", "modified", "constrained"):
        raise ValueError(f"rnnt_type should be ('regular' | 'modified' | 'constrained'), given {rnnt_type}")


def _i64(t: torch.Tensor) -> torch.Tensor:
    return t if t.dtype == torch.int64 else t.to(torch.int64)


def fix_for_boundary(px: torch.Tensor, boundary: Optional[torch.Tensor] = None) -> torch.Tensor:
    """rnnt_loss.py:28-61: px[b, :, boundary[b,3]] = -inf (regular type only)."""
    if boundary is None:
        return px
    B, S, T1 = px.shape
    idx = _i64(boundary[:, 3]).reshape(B, 1, 1).expand(B, S, 1)
    return px.scatter(2, idx, _NEG_INF)


def _use_fused_builder(C: int) -> bool:
    """The f32-MFMA builder kernel (csrc/simple_fused.hip) unless the size is outside its domain (C % 4 != 0) or
    FTR_BUILDER_GEMM=library asks for the library-GEMM route (A/B comparisons)."""
    return os.environ.get("FTR_BUILDER_GEMM", "fused") != "library" and bool(_lib.lib().ftr_simple_logprobs_fused_supported(int(C)))


# (B, T, S, C) -> is the fused d am kernel the faster route on MI355X?  The six measured points behind `auto` below.
_FUSED_BWD_MEASURED = {
    (32, 512, 100, 500): True,      # c2
    (32, 1000, 200, 500): True,     # c3
    (32, 2000, 300, 1024): True,    # c4
    (8, 8000, 1000, 512): True,     # c5
    (16, 3000, 600, 768): True,
    (8, 1000, 200, 256): True,
}


def _use_fused_builder_bwd(T: int, C: int, B: int = 1) -> bool:
    """The fused d am kernel (W^T lm_probs + the scatter by symbol inside one kernel, csrc/simple_fused.hip, with the W that
    the W kernel has just written as its operand: `damp` [B,T,C] is never allocated) against library GEMM kind 2 (measured
    kernel choice) + epilogue kernel.  Measured on MI355X, us, fused / library (profiles/fused_bwd_am_w.md): inside the step
    c3 104 / 61 + 59, c5 813 / 477 + 367, c4 (smoothed) 528 against 545 for the kernel that formed W itself; alone, simple
    loss (scripts/fused_bwd_bench.py) c2 37 / 46, c3 96 / 119, c4 461 / 573, c5 767 / 824, B16 T3000 S600 C768 511 / 581,
    B8 T1000 S200 C256 29 / 36.  The fused kernel wins at every point, from C = 256 to 1024 and from 128 to 4096 tiles, so
    the default ("auto") takes it wherever it applies (T % 4 == 0, C % 4 == 0; B does not enter the rule: it enters the
    kernel's own choice of column tiling).  FTR_BUILDER_BWD=fused / library force a route (A/B comparisons and the
    route-vs-route tests); outside the kernel's domain every mode takes the library route."""
    mode = os.environ.get("FTR_BUILDER_BWD", "auto")
    if mode == "library" or not _use_fused_builder(C) or not _lib.lib().ftr_simple_logprobs_fused_bwd_supported(int(T), int(C)):
        return False
    return True


def _live_scratch(d_lm: torch.Tensor, B: int, S: int) -> torch.Tensor:
    """The table of live frame intervals [B,S+1,2] (int32, include/ftr_live.h) in the first bytes of d_lm's own storage: the W
    kernel writes it, the fused d am kernel reads it, and only then does the last kernel of the backward (ftr_*_logprobs_bwd_lm_f32,
    same stream) write d_lm [B,S+1,C], every element of it.  C >= 4 on the fused route, so the table fits; no allocation."""
    return d_lm.view(-1)[:2 * B * (S + 1)].view(torch.int32).view(B, S + 1, 2)


def _simple_builder(amc, lmc, symbols, am_probs, lm_probs, am_max, lm_max, boundary, blank, delay_penalty, px, py,
                    B, T, S, C, modified, st):
    """normalisers + px / py of get_rnnt_logprobs (rnnt_loss.py:180-221): one fused launch, or library GEMM + epilogue.
    Returns the product [B,S+1,T] (the backward's W kernel reads it)."""
    if _use_fused_builder(C):
        prod = torch.empty((B, S + 1, T), dtype=torch.float32, device=amc.device)
        _lib.call("ftr_simple_logprobs_fused_fwd_f32", _ptr(amc), _ptr(lmc), _ptr(symbols), _ptr(am_probs), _ptr(lm_probs),
                  _ptr(am_max), _ptr(lm_max), _ptr(boundary), int(blank), float(delay_penalty), _ptr(px), _ptr(py),
                  _ptr(prod), B, T, S, C, int(modified), st)
        return prod
    prod = _gemm(0, lm_probs, am_probs, B, T, S, C, st)                                               # :180-182
    _lib.call("ftr_simple_logprobs_fwd_f32", _ptr(amc), _ptr(lmc), _ptr(symbols), _ptr(prod), _ptr(am_max),
              _ptr(lm_max), _ptr(boundary), int(blank), float(delay_penalty), _ptr(px), _ptr(py),
              B, T, S, C, int(modified), st)
    return prod


def _simple_forward(lm, am, symbols, termination_symbol, boundary, modified, delay_penalty):
    """Forward of the simple builder (rnnt_loss.py:175-221).  Returns px, py and what the backward needs."""
    B, T, C = am.shape
    S = lm.shape[1] - 1
    T1 = T if modified else T + 1
    amc = am.detach().contiguous(); lmc = lm.detach().contiguous()
    dev = amc.device
    am_probs = torch.empty_like(amc); lm_probs = torch.empty_like(lmc)
    am_max = torch.empty((B, T), dtype=torch.float32, device=dev)
    lm_max = torch.empty((B, S + 1), dtype=torch.float32, device=dev)
    px = torch.empty((B, S, T1), dtype=torch.float32, device=dev)
    py = torch.empty((B, S + 1, T), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        st = _stream_ptr(amc)
        _lib.call("ftr_rowmax_exp_pair_f32", _ptr(amc), _ptr(am_probs), _ptr(am_max), B * T,              # :175-178
                  _ptr(lmc), _ptr(lm_probs), _ptr(lm_max), B * (S + 1), C, st)
        prod = _simple_builder(amc, lmc, symbols, am_probs, lm_probs, am_max, lm_max, boundary, termination_symbol,
                               delay_penalty, px, py, B, T, S, C, modified, st)
    return px, py, (am_probs, lm_probs, prod, symbols, boundary), (int(termination_symbol), int(modified))


def _simple_backward(saved, meta, gpx, gpy, scale=None, stride=0, mul=1.0):
    """Hand-written backward of the simple builder; gpx / gpy are d/d px, d/d py, multiplied on the fly by
    (scale ? scale[b * stride] : 1) * mul (the upstream gradient of the loss that owns the occupancies)."""
    am_probs, lm_probs, prod, symbols, boundary = saved
    blank, modified = meta
    B, T, C = am_probs.shape
    S = lm_probs.shape[1] - 1
    dev = am_probs.device
    gpx = gpx.contiguous(); gpy = gpy.contiguous()
    W = torch.empty_like(prod)
    rsx = torch.empty((B, S + 1), dtype=torch.float32, device=dev)
    rsy = torch.empty((B, S + 1), dtype=torch.float32, device=dev)
    d_am = torch.empty_like(am_probs); d_lm = torch.empty_like(lm_probs)
    fused = _use_fused_builder_bwd(T, C, B)
    with torch.cuda.device(dev):
        st = _stream_ptr(am_probs)
        if fused:     # W and, per row, the frame interval outside which it and the occupancies are exact zeros
            live = _live_scratch(d_lm, B, S)
            _lib.call("ftr_simple_logprobs_bwd_w_live_f32", _ptr(gpx), _ptr(gpy), _ptr(scale), stride, mul,
                      _ptr(prod), _ptr(boundary), _ptr(W), _ptr(rsx), _ptr(rsy), _ptr(live), B, T, S, modified, st)
        else:
            _lib.call("ftr_simple_logprobs_bwd_w_scaled_f32", _ptr(gpx), _ptr(gpy), _ptr(scale), stride, mul,
                      _ptr(prod), _ptr(boundary), _ptr(W), _ptr(rsx), _ptr(rsy), B, T, S, modified, st)
        dlmp = _gemm(1, W, am_probs, B, T, S, C, st)         # [B,S+1,C]
        if fused:                                              # W^T lm_probs inside the d am kernel, over the live row chunks only
            _lib.call("ftr_simple_logprobs_fused_bwd_am_live_f32", _ptr(gpx), _ptr(gpy), _ptr(scale), stride, mul,
                      _ptr(W), _ptr(live), _ptr(lm_probs), _ptr(am_probs), _ptr(symbols), _ptr(boundary), blank, _ptr(d_am),
                      B, T, S, C, modified, st)
        else:
            damp = _gemm(2, W, lm_probs, B, T, S, C, st)    # [B,T,C]
            _lib.call("ftr_simple_logprobs_bwd_am_scaled_f32", _ptr(gpx), _ptr(gpy), _ptr(scale), stride, mul,
                      _ptr(damp), _ptr(am_probs), _ptr(symbols), _ptr(boundary), blank, _ptr(d_am), B, T, S, C,
                      modified, st)
        _lib.call("ftr_simple_logprobs_bwd_lm_f32", _ptr(dlmp), _ptr(lm_probs), _ptr(symbols), _ptr(rsx), _ptr(rsy),
                  blank, _ptr(d_lm), B, S, C, st)
    return d_lm, d_am


class _SimpleLogprobs(torch.autograd.Function):
    """get_rnnt_logprobs (+ fix_for_boundary + delay penalty) for regular/modified: native prologue and
    epilogue kernels around the normaliser GEMM (ftr_normalizer_gemm_f32 -> rocBLAS), hand-written backward."""

    @staticmethod
    def forward(ctx, lm, am, symbols, termination_symbol, boundary, modified, delay_penalty):
        px, py, saved, meta = _simple_forward(lm, am, symbols, termination_symbol, boundary, modified, delay_penalty)
        ctx.save_for_backward(*saved)
        ctx.meta = meta
        return px, py

    @staticmethod
    def backward(ctx, gpx, gpy):
        d_lm, d_am = _simple_backward(ctx.saved_tensors, ctx.meta, gpx, gpy)
        return d_lm, d_am, None, None, None, None, None


class _SimpleLoss(torch.autograd.Function):
    """rnnt_loss_simple for regular/modified as ONE graph node: builder kernels + GEMM, recursion forward + backward
    (occupancies), native loss reduction; backward() feeds the occupancies with the upstream gradient folded in on
    the fly (ftr_simple_logprobs_bwd_*_scaled_f32) -- no framework-side pass over a lattice anywhere."""

    @staticmethod
    def forward(ctx, lm, am, symbols, termination_symbol, boundary, modified, delay_penalty, code, want_occupancies):
        px, py, saved, meta = _simple_forward(lm, am, symbols, termination_symbol, boundary, modified, delay_penalty)
        # the recursion backward (occupancies) only when somebody wants them: the caller (calc_gradients) or autograd
        need = bool(want_occupancies) or ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        if need:      # the loss tail rides along with the recursion's backward launch
            ans, px_grad, py_grad, loss = mi_forward_backward(px, py, boundary, True, ans_grad_is_one=True, loss_code=code)
        else:
            ans, px_grad, py_grad = mi_forward_backward(px, py, boundary, False, ans_grad_is_one=True)
            loss = _negated_reduce_native(ans, code)
        shape_x, shape_y = px.shape, py.shape
        del px, py
        if need:
            ctx.save_for_backward(*saved, px_grad, py_grad)
        else:
            px_grad = torch.zeros(shape_x, dtype=torch.float32, device=loss.device)
            py_grad = torch.zeros(shape_y, dtype=torch.float32, device=loss.device)
        ctx.meta = meta
        ctx.code = int(code)
        ctx.mark_non_differentiable(px_grad, py_grad)
        ctx.set_materialize_grads(False)          # no zero tensors for the two occupancy outputs in backward
        return loss, px_grad, py_grad

    @staticmethod
    def backward(ctx, g_loss, _g1, _g2):
        if g_loss is None:
            return (None,) * 9
        *saved, px_grad, py_grad = ctx.saved_tensors
        scale, stride, mul = _upstream_scale(g_loss, ctx.code, px_grad.shape[0])
        d_lm, d_am = _simple_backward(saved, ctx.meta, px_grad, py_grad, scale, stride, mul)
        return d_lm, d_am, None, None, None, None, None, None, None


def _check_simple_inputs(lm, am, symbols, termination_symbol):
    _require_gpu(am, "am"); _require_gpu(lm, "lm")
    if am.dtype != torch.float32 or lm.dtype != torch.float32:
        raise TypeError("am and lm must be float32")
    B, T, C = am.shape
    S = lm.shape[1] - 1
    if lm.shape[0] != B or lm.shape[2] != C:
        raise ValueError(f"lm {tuple(lm.shape)} and am {tuple(am.shape)} disagree")
    symbols = torch.as_tensor(symbols, device=am.device)
    if tuple(symbols.shape) != (B, S):
        raise ValueError(f"symbols must have shape {(B, S)}, got {tuple(symbols.shape)}")
    if not 0 <= int(termination_symbol) < C:
        raise ValueError(f"termination_symbol {termination_symbol} not in [0, {C})")
    return symbols.to(torch.int32).contiguous()


def _simple_logprobs_native(lm, am, symbols, termination_symbol, rnnt_type, boundary, delay_penalty=0.0):
    symbols = _check_simple_inputs(lm, am, symbols, termination_symbol)
    boundary = _as_boundary(boundary, am.shape[0], am.device)
    px, py = _SimpleLogprobs.apply(lm, am, symbols, termination_symbol, boundary, rnnt_type != "regular",
                                   _penalty(delay_penalty))
    if rnnt_type == "constrained":
        px = px + py[:, 1:, :]
    return px, py


def get_rnnt_logprobs(
    lm: torch.Tensor,
    am: torch.Tensor,
    symbols: torch.Tensor,
    termination_symbol: int,
    rnnt_type: str = "regular",
    boundary: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """rnnt_loss.py:63-223.  lm [B,S+1,C], am [B,T,C], symbols [B,S] -> px [B,S,T+1|T], py [B,S+1,T].
    Native (HIP) prologue/epilogue around one library GEMM; differentiable w.r.t. lm and am."""
    _check_type(rnnt_type)
    return _simple_logprobs_native(lm, am, symbols, termination_symbol, rnnt_type, boundary)


def _penalty(delay_penalty) -> float:
    """The delay penalty as the lattice writers take it: 0.0 switches it off, as any value that is not positive does."""
    return float(delay_penalty) if delay_penalty > 0.0 else 0.0


def _apply_delay_penalty(px, boundary, rnnt_type, delay_penalty):
    """rnnt_loss.py:305-321 (also :518-534, :1097-1114, :1461-1478): float64 offsets, cast to px.dtype."""
    if not delay_penalty > 0.0:
        return px
    B, S, T0 = px.shape
    T = T0 if rnnt_type != "regular" else T0 - 1
    if boundary is None:
        offset = torch.full((B,), (T - 1) / 2, dtype=torch.float64, device=px.device)
    else:
        offset = (boundary[:, 3].to(torch.float64) - 1) / 2
    penalty = offset.reshape(B, 1, 1) - torch.arange(T0, dtype=torch.float64, device=px.device).reshape(1, 1, T0)
    penalty = penalty * delay_penalty
    return px + penalty.to(px.dtype)


_REDUCTIONS = {"none": 0, "mean": 1, "sum": 2}


def _reduction_code(reduction: Optional[str]) -> int:
    if reduction not in _REDUCTIONS:
        raise ValueError(f"reduction should be ('none' | 'mean' | 'sum'), given {reduction}")
    return _REDUCTIONS[reduction]


def _reduce(negated_loss: torch.Tensor, reduction: Optional[str]) -> torch.Tensor:
    code = _reduction_code(reduction)
    if code == 0:
        return -negated_loss
    return -torch.mean(negated_loss) if code == 1 else -torch.sum(negated_loss)


def _negated_reduce_native(ans: torch.Tensor, code: int) -> torch.Tensor:
    """-ans / -mean / -sum in one native launch (the loss tail of rnnt_loss.py:333,544-546,1124-1126,1487-1489)."""
    B = ans.shape[0]
    out = torch.empty((B,) if code == 0 else (), dtype=torch.float32, device=ans.device)
    with torch.cuda.device(ans.device):
        _lib.call("ftr_negated_reduce_f32", _ptr(ans), B, code, _ptr(out), _stream_ptr(ans))
    return out


def _upstream_scale(g_loss: torch.Tensor, code: int, B: int):
    """(pointer tensor, stride, multiplier) such that d loss / d ans[b] = scale[b * stride] * mul."""
    g = g_loss.to(torch.float32).contiguous()
    return g, (1 if code == 0 else 0), (-1.0 / B if code == 1 else -1.0)


def _drive(px, py, boundary, reduction, calc_gradients):
    scores_and_grads = mutual_information_recursion(px=px, py=py, boundary=boundary, calc_gradients=calc_gradients)
    negated_loss = scores_and_grads[0] if calc_gradients else scores_and_grads
    loss = _reduce(negated_loss, reduction)
    return (loss, scores_and_grads[1]) if calc_gradients else loss


def rnnt_loss_simple(
    lm: torch.Tensor,
    am: torch.Tensor,
    symbols: torch.Tensor,
    termination_symbol: int,
    boundary: Optional[torch.Tensor] = None,
    rnnt_type: str = "regular",
    delay_penalty: float = 0.0,
    reduction: Optional[str] = "mean",
    calc_gradients: bool = False,
) -> Union[torch.Tensor, Tuple[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]]:
    """rnnt_loss.py:225-338.  Returns loss, or (loss, (px_grad, py_grad)) when ``calc_gradients``."""
    _check_type(rnnt_type)
    code = _reduction_code(reduction)
    boundary = _as_boundary(boundary, am.shape[0], am.device)
    if rnnt_type == "constrained":   # the penalty applies after px += py[:, 1:, :]  (:218-221, :305-321)
        px, py = _simple_logprobs_native(lm, am, symbols, termination_symbol, rnnt_type, boundary)
        px = _apply_delay_penalty(px, boundary, rnnt_type, delay_penalty)
        return _drive(px, py, boundary, reduction, calc_gradients)
    symbols_i = _check_simple_inputs(lm, am, symbols, termination_symbol)
    loss, px_grad, py_grad = _SimpleLoss.apply(lm, am, symbols_i, termination_symbol, boundary, rnnt_type != "regular",
                                               _penalty(delay_penalty), code, bool(calc_gradients))
    return (loss, (px_grad, py_grad)) if calc_gradients else loss


def _joint_inputs(logits, symbols) -> torch.Tensor:
    """Checks unpruned joiner logits [B,T,S+1,C] against symbols [B,S] and returns the identity ranges, ranges[b,t,:] =
    0..S: with every row in range the pruned builder IS the joint builder (its band is the lattice)."""
    _require_gpu(logits, "logits")
    if logits.dim() != 4:
        raise ValueError("logits must be [B,T,S+1,C]")
    B, T, S1, _ = logits.shape
    if tuple(torch.as_tensor(symbols).shape) != (B, S1 - 1):
        raise ValueError(f"symbols must have shape {(B, S1 - 1)}, got {tuple(torch.as_tensor(symbols).shape)}")
    ranges = torch.arange(S1, dtype=torch.int32, device=logits.device).expand(B, T, S1).contiguous()
    _mark_band(ranges)
    return ranges


def get_rnnt_logprobs_joint(
    logits: torch.Tensor,
    symbols: torch.Tensor,
    termination_symbol: int,
    boundary: Optional[torch.Tensor] = None,
    rnnt_type: str = "regular",
) -> Tuple[torch.Tensor, torch.Tensor]:
    """rnnt_loss.py:340-452.  logits [B,T,S+1,C] -> px [B,S,T+1|T], py [B,S+1,T].  Native: the streaming
    log-sum-exp + lattice writer of the pruned builder with s_range = S+1 (identity ranges), and the same
    hand-written backward (d/d logits = scattered gradient - softmax * row sum)."""
    _check_type(rnnt_type)
    return get_rnnt_logprobs_pruned(logits=logits, symbols=symbols, ranges=_joint_inputs(logits, symbols),
                                    termination_symbol=termination_symbol, boundary=boundary, rnnt_type=rnnt_type)


def get_hat_logprobs_joint(
    logits: torch.Tensor,
    symbols: torch.Tensor,
    termination_symbol: int,
    boundary: Optional[torch.Tensor] = None,
    rnnt_type: str = "regular",
) -> Tuple[torch.Tensor, torch.Tensor]:
    """HAT form of ``get_rnnt_logprobs_joint`` (MI355X addition): logits [B,T,S+1,C] -> px [B,S,T+1|T], py [B,S+1,T]
    with the normalisation of ``get_hat_logprobs_pruned``, on identity ranges.  The best path of a HAT model is
    ``mutual_information_viterbi(*get_hat_logprobs_joint(...), boundary)``."""
    _check_type(rnnt_type)
    return get_hat_logprobs_pruned(logits=logits, symbols=symbols, ranges=_joint_inputs(logits, symbols),
                                   termination_symbol=termination_symbol, boundary=boundary, rnnt_type=rnnt_type)


def rnnt_loss(
    logits: torch.Tensor,
    symbols: torch.Tensor,
    termination_symbol: int,
    boundary: Optional[torch.Tensor] = None,
    rnnt_type: str = "regular",
    delay_penalty: float = 0.0,
    reduction: Optional[str] = "mean",
    calc_gradients: bool = False,
) -> torch.Tensor:
    """rnnt_loss.py:454-551 (unpruned loss on joiner logits [B,T,S+1,C]).  Without ``calc_gradients`` this is the
    fused pruned loss with identity ranges (px/py, recursion forward+backward and d/d logits in native code)."""
    _check_type(rnnt_type)
    boundary = _as_boundary(boundary, logits.shape[0], logits.device)
    if not calc_gradients:
        return rnnt_loss_pruned(logits=logits, symbols=symbols, ranges=_joint_inputs(logits, symbols),
                                termination_symbol=termination_symbol, boundary=boundary, rnnt_type=rnnt_type,
                                delay_penalty=delay_penalty, reduction=reduction)
    px, py = get_rnnt_logprobs_joint(logits=logits, symbols=symbols, termination_symbol=termination_symbol,
                                     boundary=boundary, rnnt_type=rnnt_type)
    px = _apply_delay_penalty(px, boundary, rnnt_type, delay_penalty)
    return _drive(px, py, boundary, reduction, calc_gradients)


def _monotonic_lower_bound(x: torch.Tensor) -> torch.Tensor:
    """rnnt_loss.py:553-585: reverse -> cummin -> reverse (suffix minimum).  int32, last axis."""
    squeeze = x.dim() == 1
    x2 = x.reshape(1, -1) if squeeze else x
    out = cummin(torch.flip(x2.to(torch.int32), dims=(-1,)).contiguous())
    out = torch.flip(out, dims=(-1,))
    return out[0] if squeeze else out


def _adjust_pruning_lower_bound(s_begin: torch.Tensor, s_range: int) -> torch.Tensor:
    """rnnt_loss.py:587-641, op by op on top of the native ``cummin`` (the fused path used by
    ``get_rnnt_prune_ranges`` does the same arithmetic in one kernel)."""
    B, T = s_begin.shape
    ar = torch.arange(0, T, dtype=torch.int32, device=s_begin.device)
    s_begin = _monotonic_lower_bound(s_begin)
    s_begin = -(s_begin - (s_range - 1) * ar)
    s_begin = _monotonic_lower_bound(s_begin)
    s_begin = torch.clamp(s_begin, min=0)
    s_begin = -(s_begin - (s_range - 1) * ar)
    return s_begin


def get_rnnt_prune_ranges(
    px_grad: torch.Tensor,
    py_grad: torch.Tensor,
    boundary: torch.Tensor,
    s_range: int,
) -> torch.Tensor:
    """rnnt_loss.py:647-761.  Returns int32 ranges [B,T,s_range'] with s_range' = S+1 if s_range > S."""
    _require_gpu(px_grad, "px_grad"); _require_gpu(py_grad, "py_grad")
    B, S, T1 = px_grad.shape
    T = py_grad.shape[-1]
    if T1 not in (T, T + 1):
        raise ValueError(f"px_grad.shape[-1]={T1} must be T or T+1 (T={T})")
    if tuple(py_grad.shape) != (B, S + 1, T):
        raise ValueError(f"py_grad must have shape {(B, S + 1, T)}, got {tuple(py_grad.shape)}")
    if boundary is None:
        raise ValueError("get_rnnt_prune_ranges: boundary is mandatory (rnnt_loss.py:741-746)")
    s_range = int(s_range)
    r = S + 1 if s_range > S else s_range
    px_grad = px_grad.detach().to(torch.float32).contiguous()
    py_grad = py_grad.detach().to(torch.float32).contiguous()
    boundary = _as_boundary(boundary, B, px_grad.device)
    ranges = torch.empty((B, T, r), dtype=torch.int32, device=px_grad.device)
    scratch = torch.empty((B, T), dtype=torch.int32, device=px_grad.device)
    r_eff = ctypes.c_int(0)
    with torch.cuda.device(px_grad.device):
        _lib.call("ftr_prune_ranges_i32", _ptr(px_grad), _ptr(py_grad), _ptr(boundary), _ptr(ranges),
                                                   _ptr(scratch), B, S, T, T1, s_range, ctypes.byref(r_eff),
                                                   _stream_ptr(px_grad))
    assert r_eff.value == r
    # what the kernel guarantees (rnnt_loss.py:673-677): ranges[b,t,0] non-decreasing in t, inside [0, S - r + 1], and
    # ranges[b,t,k] = ranges[b,t,0] + k: a band.  The mark only saves rnnt_loss_pruned the device-side check it runs on
    # ranges tensors it has not seen (a clone, a slice, a reloaded tensor: _is_band).
    _mark_band(ranges)
    return ranges


class _DoPruning(torch.autograd.Function):
    @staticmethod
    def forward(ctx, am, lm, ranges, dense):
        B, T, r = ranges.shape
        S1, C = lm.shape[1], lm.shape[2]
        am_c = am.detach().contiguous(); lm_c = lm.detach().contiguous()
        # am_pruned[b,t,k,:] = am[b,t,:] for every k (rnnt_loss.py:803): a broadcast.  TensorFlow has no strided tensors and
        # materialises it; here it stays a stride-0 view (as k2's fast_rnnt returns it), which a joiner's `am_pruned +
        # lm_pruned` consumes by broadcasting: B*T*r*C*4 bytes less to write here and to read there.  Values, shape and the
        # gradient (the sum over r, in the fused backward below) are the reference's; .contiguous() gives the dense tensor.
        # dense=True materialises it (one more [B,T,r,C] stream written by the same kernel): for callers that write into
        # am_pruned, reshape it with .view(), or hand it to code that wants contiguous memory.
        am_p = torch.empty((B, T, r, C), dtype=am.dtype, device=am.device) if dense else am_c.unsqueeze(2).expand(B, T, r, C)
        lm_p = torch.empty((B, T, r, C), dtype=lm.dtype, device=lm.device)
        with torch.cuda.device(am.device):
            _lib.call("ftr_do_pruning_f32", _ptr(am_c), _ptr(lm_c), _ptr(ranges), _ptr(am_p) if dense else None, _ptr(lm_p),
                                                     B, T, S1, C, r, _stream_ptr(am))
        ctx.save_for_backward(ranges)
        ctx.lm_shape = tuple(lm.shape)
        return am_p, lm_p

    @staticmethod
    def backward(ctx, g_am_p, g_lm_p):
        (ranges,) = ctx.saved_tensors
        B, S1, C = ctx.lm_shape
        T, r = ranges.shape[1], ranges.shape[2]
        g_am_p = g_am_p.contiguous(); g_lm_p = g_lm_p.contiguous()
        g_am = torch.empty((B, T, C), dtype=g_am_p.dtype, device=g_am_p.device)     # broadcast <-> sum over s_range
        g_lm = torch.empty((B, S1, C), dtype=g_lm_p.dtype, device=g_lm_p.device)    # gather    <-> segment sum
        ws_bytes = int(_lib.lib().ftr_do_pruning_bwd_workspace_bytes(B, T, S1, C, r))
        ws = torch.empty(((ws_bytes + 3) // 4,), dtype=torch.float32, device=g_am_p.device) if ws_bytes else None
        with torch.cuda.device(g_am_p.device):
            _lib.call("ftr_do_pruning_bwd_ws_f32", _ptr(g_am_p), _ptr(g_lm_p), _ptr(ranges), _ptr(g_am), _ptr(g_lm),
                      B, T, S1, C, r, _ptr(ws), ws_bytes, _stream_ptr(g_am_p))
        return g_am, g_lm, None, None


def do_rnnt_pruning(am: torch.Tensor, lm: torch.Tensor, ranges: torch.Tensor, dense: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """rnnt_loss.py:763-812.  am [B,T,C], lm [B,S+1,C], ranges [B,T,s_range] -> two [B,T,s_range,C].

    ``am_pruned[b,t,k,:] = am[b,t,:]`` is a broadcast (rnnt_loss.py:803).  By default it is returned as a stride-0 VIEW of
    ``am`` (as k2's fast_rnnt returns it): same values, shape and gradient as the reference's dense tensor, and a joiner's
    ``am_pruned + lm_pruned`` reads it by broadcasting -- but it aliases ``am`` (changing ``am`` afterwards changes it),
    it cannot be written in place and ``.view(-1, C)`` refuses it.  ``dense=True`` (an extension, not in the reference's
    signature) returns the reference's materialised tensor, written by the same gather kernel; ``.contiguous()`` on the
    view gives the same thing."""
    _require_gpu(am, "am"); _require_gpu(lm, "lm"); _require_gpu(ranges, "ranges")
    if am.dtype != torch.float32 or lm.dtype != torch.float32:
        raise TypeError("am and lm must be float32")
    if ranges.shape[0] != am.shape[0] or ranges.shape[0] != lm.shape[0] or am.shape[1] != ranges.shape[1]:
        raise ValueError("do_rnnt_pruning: inconsistent shapes")
    ranges = ranges.to(torch.int32).contiguous()
    return _DoPruning.apply(am, lm, ranges, bool(dense))


# 16-bit joiner logits go through the _dt entry points (element type code, HAT as a flag); float32 keeps its _f32 ones
_LOWP_KIND = {torch.bfloat16: _lib.FTR_DTYPE_BF16, torch.float16: _lib.FTR_DTYPE_FP16}


class _DoPruningSum(torch.autograd.Function):
    """am[b,t,:] + lm[b, ranges[b,t,k], :] as one launch each way plus the segment reduction (include/ftr_prune_sum.h);
    nothing but ``ranges`` is kept for the backward."""

    @staticmethod
    def forward(ctx, am, lm, ranges):
        B, T, r = ranges.shape
        S1, C = lm.shape[1], lm.shape[2]
        am_c = am.detach().contiguous(); lm_c = lm.detach().contiguous()
        z = torch.empty((B, T, r, C), dtype=am.dtype, device=am.device)
        with torch.cuda.device(am.device):
            _lib.call("ftr_do_pruning_sum_dt", _ptr(am_c), _ptr(lm_c), _LOWP_KIND.get(am.dtype, _lib.FTR_DTYPE_F32), _ptr(ranges),
                      _ptr(z), B, T, S1, C, r, _stream_ptr(am))
        ctx.save_for_backward(ranges)
        ctx.lm_shape = tuple(lm.shape)
        return z

    @staticmethod
    def backward(ctx, g):
        (ranges,) = ctx.saved_tensors
        B, S1, C = ctx.lm_shape
        T, r = ranges.shape[1], ranges.shape[2]
        g = g.contiguous()
        g_am = torch.empty((B, T, C), dtype=g.dtype, device=g.device)      # broadcast <-> sum over s_range
        g_lm = torch.empty((B, S1, C), dtype=g.dtype, device=g.device)     # gather    <-> segment sum
        ws_bytes = int(_lib.lib().ftr_do_pruning_bwd_workspace_bytes(B, T, S1, C, r))    # float32 partial rows for every dtype
        ws = torch.empty(((ws_bytes + 3) // 4,), dtype=torch.float32, device=g.device) if ws_bytes else None
        with torch.cuda.device(g.device):
            _lib.call("ftr_do_pruning_sum_bwd_ws_dt", _ptr(g), _LOWP_KIND.get(g.dtype, _lib.FTR_DTYPE_F32), _ptr(ranges), _ptr(g_am),
                      _ptr(g_lm), B, T, S1, C, r, _ptr(ws), ws_bytes, _stream_ptr(g))
        return g_am, g_lm, None


def do_rnnt_pruning_sum(am: torch.Tensor, lm: torch.Tensor, ranges: torch.Tensor) -> torch.Tensor:
    """MI355X addition: ``sum(do_rnnt_pruning(am, lm, ranges))`` as one operation, in float32, bfloat16 or float16.

    am [B,T,C], lm [B,S+1,C] (one dtype for both), ranges [B,T,s_range] -> z [B,T,s_range,C], contiguous, in that dtype:
    ``z[b,t,k,:] = am[b,t,:] + lm[b, ranges[b,t,k], :]``, the addition every joiner starts with.  The gathered
    ``lm_pruned`` never exists: the forward writes z once, the backward reads its gradient once.  A 16-bit tensor stands
    for its exact float32 up-conversion: one float32 addition and one rounding to nearest-even per element; the gradients
    are accumulated in float32, in the order of ``do_rnnt_pruning``'s backward, and rounded once into the dtype of am / lm.
    Deterministic (no atomics), kernels only (capturable into a graph)."""
    _require_gpu(am, "am"); _require_gpu(lm, "lm"); _require_gpu(ranges, "ranges")
    if am.dtype != lm.dtype or (am.dtype != torch.float32 and am.dtype not in _LOWP_KIND):
        raise TypeError("am and lm must have the same dtype: float32, bfloat16 or float16")
    if am.dim() != 3 or lm.dim() != 3 or ranges.dim() != 3 or am.shape[2] != lm.shape[2]:
        raise ValueError("do_rnnt_pruning_sum: am [B,T,C], lm [B,S+1,C] and ranges [B,T,s_range] expected")
    if ranges.shape[0] != am.shape[0] or ranges.shape[0] != lm.shape[0] or am.shape[1] != ranges.shape[1]:
        raise ValueError("do_rnnt_pruning_sum: inconsistent shapes")
    ranges = ranges.to(torch.int32).contiguous()
    return _DoPruningSum.apply(am, lm, ranges)


_ACT_KIND = {"tanh": _lib.FTR_ACT_TANH, "relu": _lib.FTR_ACT_RELU}


class _DoPruningAct(torch.autograd.Function):
    """act(am[b,t,:] + lm[b, ranges[b,t,k], :]) (include/ftr_joiner_act.h).  ``ranges`` and the output itself are kept for
    the backward, which forms dz = g * act'(y) as it reads g and y; neither the sum nor dz is ever in memory."""

    @staticmethod
    def forward(ctx, am, lm, ranges, act):
        B, T, r = ranges.shape
        S1, C = lm.shape[1], lm.shape[2]
        am_c = am.detach().contiguous(); lm_c = lm.detach().contiguous()
        y = torch.empty((B, T, r, C), dtype=am.dtype, device=am.device)
        with torch.cuda.device(am.device):
            _lib.call("ftr_pruned_joiner_act_dt", _ptr(am_c), _ptr(lm_c), _LOWP_KIND.get(am.dtype, _lib.FTR_DTYPE_F32), act, _ptr(ranges),
                      _ptr(y), B, T, S1, C, r, _stream_ptr(am))
        ctx.save_for_backward(ranges, y)
        ctx.lm_shape = tuple(lm.shape)
        ctx.act = act
        return y

    @staticmethod
    def backward(ctx, g):
        ranges, y = ctx.saved_tensors
        B, S1, C = ctx.lm_shape
        T, r = ranges.shape[1], ranges.shape[2]
        g = g.contiguous()
        g_am = torch.empty((B, T, C), dtype=g.dtype, device=g.device)      # broadcast <-> sum over s_range
        g_lm = torch.empty((B, S1, C), dtype=g.dtype, device=g.device)     # gather    <-> segment sum
        ws_bytes = int(_lib.lib().ftr_do_pruning_bwd_workspace_bytes(B, T, S1, C, r))    # float32 partial rows for every dtype
        ws = torch.empty(((ws_bytes + 3) // 4,), dtype=torch.float32, device=g.device) if ws_bytes else None
        with torch.cuda.device(g.device):
            _lib.call("ftr_pruned_joiner_act_bwd_ws_dt", _ptr(g), _ptr(y), _LOWP_KIND.get(g.dtype, _lib.FTR_DTYPE_F32), ctx.act,
                      _ptr(ranges), _ptr(g_am), _ptr(g_lm), B, T, S1, C, r, _ptr(ws), ws_bytes, _stream_ptr(g))
        return g_am, g_lm, None, None


def do_rnnt_pruning_act(am: torch.Tensor, lm: torch.Tensor, ranges: torch.Tensor, activation: str = "tanh") -> torch.Tensor:
    """MI355X addition: ``act(do_rnnt_pruning_sum(am, lm, ranges))`` as one operation, ``activation`` "tanh" or "relu":
    what a joiner hands to its output layer, ``output_linear(do_rnnt_pruning_act(am, lm, ranges))``.

    am [B,T,C], lm [B,S+1,C] (one dtype for both: float32, bfloat16 or float16), ranges [B,T,s_range] -> y [B,T,s_range,C],
    contiguous, in that dtype: ``y[b,t,k,:] = act(am[b,t,:] + lm[b, ranges[b,t,k], :])``.  The sum is one float32 addition,
    the activation is computed in float32 and rounded once into the dtype; the sum itself is never in memory.  The backward
    keeps y (which the next layer keeps anyway) and forms ``g * (1 - y*y)`` or ``g where y > 0`` in registers as it sums:
    float32 accumulation in the order of ``do_rnnt_pruning``'s backward, one rounding into the dtype.  Deterministic (no
    atomics), kernels only (capturable into a graph)."""
    _require_gpu(am, "am"); _require_gpu(lm, "lm"); _require_gpu(ranges, "ranges")
    if am.dtype != lm.dtype or (am.dtype != torch.float32 and am.dtype not in _LOWP_KIND):
        raise TypeError("am and lm must have the same dtype: float32, bfloat16 or float16")
    if activation not in _ACT_KIND:
        raise ValueError(f"do_rnnt_pruning_act: activation must be 'tanh' or 'relu', got {activation!r}")
    if am.dim() != 3 or lm.dim() != 3 or ranges.dim() != 3 or am.shape[2] != lm.shape[2]:
        raise ValueError("do_rnnt_pruning_act: am [B,T,C], lm [B,S+1,C] and ranges [B,T,s_range] expected")
    if ranges.shape[0] != am.shape[0] or ranges.shape[0] != lm.shape[0] or am.shape[1] != ranges.shape[1]:
        raise ValueError("do_rnnt_pruning_act: inconsistent shapes")
    ranges = ranges.to(torch.int32).contiguous()
    return _DoPruningAct.apply(am, lm, ranges, _ACT_KIND[activation])


def _pruned_call(name, hat, x, head, tail):
    """One logits-reading entry point on ``x``: ``ftr_[hat_]<name>_f32(x, *head, *tail)`` for float32 logits,
    ``ftr_<name>_dt(x, kind, *head, flags, *tail)`` for bfloat16 / float16 (``tail``: the stream)."""
    kind = _LOWP_KIND.get(x.dtype)
    if kind is None:
        _lib.call(f"ftr_{'hat_' if hat else ''}{name}_f32", _ptr(x), *head, *tail)
    else:
        _lib.call(f"ftr_{name}_dt", _ptr(x), kind, *head, _lib.FTR_PRUNED_HAT if hat else 0, *tail)


def _pruned_builder_fwd(x, symbols, ranges, boundary, blank, delay_penalty, modified, hat):
    """lse [B,T,r] and the full-size px / py of the pruned builder (``hat``: the ftr_hat_* twin), one launch."""
    B, T, r, C = x.shape
    S = symbols.shape[1]
    lse = torch.empty((B, T, r), dtype=torch.float32, device=x.device)
    px = torch.empty((B, S, T if modified else T + 1), dtype=torch.float32, device=x.device)
    py = torch.empty((B, S + 1, T), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _pruned_call("pruned_logprobs_fwd", hat, x, (_ptr(symbols), _ptr(ranges), _ptr(boundary), int(blank),
                     float(delay_penalty), _ptr(lse), _ptr(px), _ptr(py), B, T, S, C, r, int(modified)), (_stream_ptr(x),))
    return lse, px, py


def _pruned_builder_bwd(x, symbols, ranges, boundary, blank, modified, lse, gpx, gpy, scale, stride, mul, band, hat):
    """d/d logits from d/d px, d/d py (``band``: band-shaped [B,T,r], else the full-size lattices), multiplied on the fly
    by (scale ? scale[b * stride] : 1) * mul; one streaming launch.  The gradient has the dtype of ``x``."""
    B, T, r, C = x.shape
    S = symbols.shape[1]
    g = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _pruned_call("pruned_band_bwd_scaled" if band else "pruned_logprobs_bwd_scaled", hat, x,
                     (_ptr(symbols), _ptr(ranges), _ptr(boundary), blank, _ptr(lse), _ptr(gpx), _ptr(gpy), _ptr(scale), stride,
                      mul, _ptr(g), B, T, S, C, r, modified), (_stream_ptr(x),))
    return g


class _PrunedLogprobs(torch.autograd.Function):
    """get_rnnt_logprobs_pruned for regular/modified as two native launches each way (``hat``: the ftr_hat_* twins,
    get_hat_logprobs_pruned)."""

    @staticmethod
    def forward(ctx, logits, symbols, ranges, termination_symbol, boundary, modified, delay_penalty, hat):
        x = logits.detach().contiguous()
        lse, px, py = _pruned_builder_fwd(x, symbols, ranges, boundary, termination_symbol, delay_penalty, modified, hat)
        ctx.save_for_backward(x, symbols, ranges, lse, boundary)
        ctx.meta = (int(termination_symbol), int(modified), bool(hat))
        return px, py

    @staticmethod
    def backward(ctx, gpx, gpy):
        x, symbols, ranges, lse, boundary = ctx.saved_tensors
        blank, modified, hat = ctx.meta
        g = _pruned_builder_bwd(x, symbols, ranges, boundary, blank, modified, lse, gpx.contiguous(), gpy.contiguous(),
                                None, 0, 1.0, False, hat)
        return g, None, None, None, None, None, None, None


def _pruned_inputs(logits, symbols, ranges, boundary, lowp=False):
    """``lowp``: bfloat16 / float16 logits are accepted too (the ordinary and HAT builders; not multi-blank, not TDT)."""
    _require_gpu(logits, "logits")
    if logits.dim() != 4:
        raise ValueError("logits must be [B,T,s_range,C]")
    if lowp and logits.dtype in _LOWP_KIND:
        pass
    elif logits.dtype != torch.float32:
        raise TypeError("logits must be float32, bfloat16 or float16" if lowp else "logits must be float32")
    B, T, r, C = logits.shape
    symbols = torch.as_tensor(symbols, device=logits.device).to(torch.int32).contiguous()
    ranges_in = ranges
    ranges = torch.as_tensor(ranges, device=logits.device).to(torch.int32).contiguous()
    if ranges is not ranges_in and isinstance(ranges_in, torch.Tensor) and _band_mark_valid(ranges_in):
        _mark_band(ranges)      # a dtype / layout / device copy of a known band is still a band
    if tuple(ranges.shape) != (B, T, r):
        raise ValueError(f"ranges must have shape {(B, T, r)}, got {tuple(ranges.shape)}")
    if symbols.dim() != 2 or symbols.shape[0] != B:
        raise ValueError("symbols must be [B,S]")
    boundary = _as_boundary(boundary, B, logits.device)
    return symbols, ranges, boundary


def get_rnnt_logprobs_pruned(
    logits: torch.Tensor,
    symbols: torch.Tensor,
    ranges: torch.Tensor,
    termination_symbol: int,
    boundary: torch.Tensor,
    rnnt_type: str = "regular",
) -> Tuple[torch.Tensor, torch.Tensor]:
    """rnnt_loss.py:853-1020.  logits [B,T,s_range,C] -> full-size px [B,S,T+1|T], py [B,S+1,T] with
    -inf outside the pruned band."""
    return _pruned_logprobs(logits, symbols, ranges, termination_symbol, boundary, rnnt_type, False)


def _pruned_logprobs(logits, symbols, ranges, termination_symbol, boundary, rnnt_type, hat):
    _check_type(rnnt_type)
    symbols, ranges, boundary = _pruned_inputs(logits, symbols, ranges, boundary, lowp=True)
    modified = rnnt_type != "regular"
    px, py = _PrunedLogprobs.apply(logits, symbols, ranges, termination_symbol, boundary, modified, 0.0, hat)
    if rnnt_type == "constrained":
        px = px + py[:, 1:, :]
    return px, py


def get_hat_logprobs_pruned(
    logits: torch.Tensor,
    symbols: torch.Tensor,
    ranges: torch.Tensor,
    termination_symbol: int,
    boundary: torch.Tensor,
    rnnt_type: str = "regular",
) -> Tuple[torch.Tensor, torch.Tensor]:
    """HAT (hybrid autoregressive transducer) form of ``get_rnnt_logprobs_pruned`` (MI355X addition, no reference
    counterpart).  The same full-size lattices (-inf outside the band, at px[:,:,T] and at the t_end column of the regular
    type), but each joiner row x = logits[b,t,k,:] is normalised as HAT does, with blank = termination_symbol:
    ``py = log sigmoid(x[blank])`` and ``px = x[sym] - logsumexp_{c != blank} x[c] - softplus(x[blank])``, so the blank
    probability is a separate Bernoulli and the symbols share the rest through a softmax over the non-blank columns.
    A symbol equal to blank gets px = -inf (and no gradient).  Needs C >= 2.  Differentiable w.r.t. ``logits``."""
    return _pruned_logprobs(logits, symbols, ranges, termination_symbol, boundary, rnnt_type, True)


def rnnt_alignment_pruned(
    logits: torch.Tensor,
    symbols: torch.Tensor,
    ranges: torch.Tensor,
    termination_symbol: int,
    boundary: Optional[torch.Tensor] = None,
    rnnt_type: str = "regular",
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Best-path alignment of the pruned joiner output (MI355X addition, no reference counterpart): the same lattice as
    ``get_rnnt_logprobs_pruned`` (full-size px / py, -inf outside the band, no delay penalty), fed to
    ``mutual_information_viterbi``.  Returns ``(score [B] float32, frames [B,S] int32)``, detached; see
    ``mutual_information_viterbi`` for their meaning (``frames[b,s]`` = the frame that emits ``symbols[b,s]``).
    Every step runs on the device with no host read, so the call can be captured into a graph.  For unpruned joiner
    logits use ``mutual_information_viterbi(*get_rnnt_logprobs_joint(...))``.

    For ``rnnt_type="regular"``, when ``ranges`` are a band with ``s_range <= 15`` (the rule of ``rnnt_loss_pruned``,
    ``FTR_PRUNED_ROUTE=lattice`` included), no lattice is built: the band builder of the loss feeds
    ``mutual_information_viterbi_tdt_band`` with moves (0,) / (1,), which returns the same bits (see there for the one
    deviation, the way a NaN travels).  Everything else takes the lattice route."""
    _check_type(rnnt_type)
    with torch.no_grad():
        symbols, ranges, boundary = _pruned_inputs(logits, symbols, ranges, boundary, lowp=True)
        B, T, r, C = logits.shape
        S = symbols.shape[1]
        if rnnt_type == "regular" and _align_band_path_ok(ranges, boundary, T, S, r, 1, 1):
            x = logits.detach().contiguous()
            lse = torch.empty((B, T, r), dtype=torch.float32, device=x.device)
            pxb = torch.empty((B, 1, T, r), dtype=torch.float32, device=x.device)
            pyb = torch.empty((B, 1, T, r), dtype=torch.float32, device=x.device)
            with torch.cuda.device(x.device):
                _pruned_call("pruned_band_fwd", False, x, (_ptr(symbols), _ptr(ranges), _ptr(boundary), int(termination_symbol), 0.0,
                             _ptr(lse), _ptr(pxb), _ptr(pyb), B, T, S, C, r, 0), (_stream_ptr(x),))
            score, frames, _, _ = mutual_information_viterbi_tdt_band(pxb, pyb, ranges, (0,), (1,), boundary, S=S)
            return score, frames
        _, px, py = _pruned_builder_fwd(logits.detach().contiguous(), symbols, ranges, boundary, termination_symbol, 0.0,
                                        rnnt_type != "regular", False)
        if rnnt_type == "constrained":
            px += py[:, 1:, :]
        return mutual_information_viterbi(px, py, boundary)


def _mark_band(ranges: torch.Tensor) -> None:
    """Remembers on the tensor object that its CURRENT contents are a band over ALL T frames, hence inside any boundary
    (the version counter catches in-place edits)."""
    ranges._ftr_band = ranges._version


def _band_mark_valid(ranges: torch.Tensor) -> bool:
    return getattr(ranges, "_ftr_band", None) == ranges._version


def _verdict_under(ranges: torch.Tensor, boundary):
    """The verdict remembered for these ranges INSIDE THE RECTANGLES OF THIS BOUNDARY (True / False), None when there is
    none: it holds for the boundary tensor object it was earned with, at the version it then had, and for nothing else."""
    version, ref, bd_version, ok = getattr(ranges, "_ftr_band_under", (None, None, None, None))
    if version == ranges._version and boundary is not None and ref() is boundary and bd_version == boundary._version:
        return ok
    return None


def _band_check(ranges: torch.Tensor, boundary) -> bool:
    """ftr_band_ranges_check_i32: one small kernel and one host read of its flag word."""
    B, T, r = ranges.shape
    flags = torch.empty((1,), dtype=torch.int32, device=ranges.device)
    with torch.cuda.device(ranges.device):
        _lib.call("ftr_band_ranges_check_i32", _ptr(ranges), _ptr(boundary), _ptr(flags), B, T, r, _stream_ptr(ranges))
    return int(flags.item()) == 0


def _is_band(ranges: torch.Tensor, boundary) -> bool:
    """Are these ranges what the band-native kernels assume (ranges[b,t,0] non-decreasing over the frames of each boundary
    rectangle, ranges[b,t,k] = ranges[b,t,0] + k)?  Decided by the DATA: a tensor that carries no valid mark (anything but
    the output of get_rnnt_prune_ranges itself: a clone, a slice, a .to(), a checkpoint) is checked once on the device
    and the verdict is remembered on the tensor, so only the first use of an unknown tensor synchronises.

    A verdict is used only for a boundary it covers.  The check runs over all T frames first: a band there is a band
    inside every rectangle, and that mark (_mark_band) is free of the boundary.  Ranges that fail it only outside the
    rectangles (the padding frames of a padded batch may step backwards) are checked a second time inside them, and that
    verdict, either way, is tied to the boundary tensor and its version (_verdict_under): the same ranges under a wider
    boundary, or under none, are looked at again.  Under stream capture an unknown pair takes the lattice route (no host
    read inside a capture)."""
    if _band_mark_valid(ranges):
        return True
    if getattr(ranges, "_ftr_not_band", None) == ranges._version:      # not a band over all T frames
        if boundary is None:
            return False
        known = _verdict_under(ranges, boundary)
        if known is not None:
            return known
    if torch.cuda.is_current_stream_capturing():
        return False
    if getattr(ranges, "_ftr_not_band", None) != ranges._version:
        if _band_check(ranges, None):
            _mark_band(ranges)
            return True
        ranges._ftr_not_band = ranges._version
        if boundary is None:
            return False
    ok = _band_check(ranges, boundary)
    ranges._ftr_band_under = (ranges._version, weakref.ref(boundary), boundary._version, ok)
    return ok


def _align_band_path_ok(ranges, boundary, T: int, S: int, r: int, N: int, Ny: int) -> bool:
    """_band_path_ok for the three alignment wrappers: the same rule and the same FTR_PRUNED_ROUTE knob, the domain of
    csrc/mi_band_viterbi.hip."""
    if os.environ.get("FTR_PRUNED_ROUTE") == "lattice":
        return False
    return band_viterbi_supported(T, S, r, N, Ny) and _is_band(ranges, boundary)


def _band_path_ok(ranges, boundary, T: int, S: int, r: int) -> bool:
    """The band-native recursion needs a band that its kernels cover (r <= 15) and ranges that ARE a band (_is_band).
    FTR_PRUNED_ROUTE=lattice (a test knob, read at call time) sends everything through the full-size lattices."""
    if os.environ.get("FTR_PRUNED_ROUTE") == "lattice":
        return False
    return _lib.lib().ftr_mutual_information_band_supported(int(T), int(S), int(r)) != 0 and _is_band(ranges, boundary)


class _PrunedLoss(torch.autograd.Function):
    """rnnt_loss_pruned for regular/modified with the whole chain native.

    Band path (ranges from get_rnnt_prune_ranges, band fits the kernel): logsumexp + band gather -> forward recursion,
    cut and backward recursion on the band [B,T,r] in one launch (ftr_mutual_information_band_ws_f32; no full-size lattice
    exists) -> in backward() one streaming kernel turns the band-shaped occupancies * upstream gradient into
    d loss / d logits.
    Lattice path (any other ranges): logsumexp + band->lattice, recursion forward / backward on the full-size lattices
    (what the reference does, rnnt_loss.py:968-1013), the same streaming kernel fed from the lattices.
    ``hat``: the ftr_hat_* twins of the three logits-reading entry points (hat_loss_pruned); the recursion is the same."""

    @staticmethod
    def forward(ctx, logits, symbols, ranges, termination_symbol, boundary, modified, delay_penalty, code, hat):
        B, T, r, C = logits.shape
        S = symbols.shape[1]
        x = logits.detach().contiguous()
        need = logits.requires_grad
        ctx.band = _band_path_ok(ranges, boundary, T, S, r)
        if ctx.band:
            lse, pxb, pyb = (torch.empty((B, T, r), dtype=torch.float32, device=x.device) for _ in range(3))
            with torch.cuda.device(x.device):
                _pruned_call("pruned_band_fwd", hat, x, (_ptr(symbols), _ptr(ranges), _ptr(boundary),
                             int(termination_symbol), float(delay_penalty), _ptr(lse), _ptr(pxb), _ptr(pyb),
                             B, T, S, C, r, int(modified)), (_stream_ptr(x),))
            ans, gxb, gyb = band_forward_backward(pxb, pyb, ranges, S, boundary, modified)
            del pxb, pyb
            if need:
                ctx.save_for_backward(x, symbols, ranges, lse, gxb, gyb, boundary)
        else:
            lse, px, py = _pruned_builder_fwd(x, symbols, ranges, boundary, termination_symbol, delay_penalty, modified, hat)
            ans, px_grad, py_grad = mi_forward_backward(px, py, boundary, need, ans_grad_is_one=True)
            del px, py
            if need:
                ctx.save_for_backward(x, symbols, ranges, lse, px_grad, py_grad, boundary)
        ctx.meta = (int(termination_symbol), int(modified), int(code), bool(hat))
        return _negated_reduce_native(ans, code)

    @staticmethod
    def backward(ctx, g_loss):
        x, symbols, ranges, lse, px_grad, py_grad, boundary = ctx.saved_tensors
        blank, modified, code, hat = ctx.meta
        scale, stride, mul = _upstream_scale(g_loss, code, x.shape[0])
        g = _pruned_builder_bwd(x, symbols, ranges, boundary, blank, modified, lse, px_grad, py_grad, scale, stride, mul,
                                ctx.band, hat)
        return g, None, None, None, None, None, None, None, None


def rnnt_loss_pruned(
    logits: torch.Tensor,
    symbols: torch.Tensor,
    ranges: torch.Tensor,
    termination_symbol: int,
    boundary: torch.Tensor = None,
    rnnt_type: str = "regular",
    delay_penalty: float = 0.0,
    reduction: Optional[str] = "mean",
    calc_gradients: bool = False,
) -> torch.Tensor:
    """rnnt_loss.py:1022-1130.  Returns the loss only (``calc_gradients`` is accepted and, as in the
    reference, only selects whether the op computes occupancies; here that follows ``requires_grad``)."""
    return _pruned_loss(logits, symbols, ranges, termination_symbol, boundary, rnnt_type, delay_penalty, reduction, False)


def _pruned_loss(logits, symbols, ranges, termination_symbol, boundary, rnnt_type, delay_penalty, reduction, hat):
    _check_type(rnnt_type)
    code = _reduction_code(reduction)
    symbols_i, ranges_i, boundary_i = _pruned_inputs(logits, symbols, ranges, boundary, lowp=True)
    if rnnt_type == "constrained":
        px, py = _pruned_logprobs(logits, symbols_i, ranges_i, termination_symbol, boundary_i, rnnt_type, hat)
        px = _apply_delay_penalty(px, boundary_i, rnnt_type, delay_penalty)
        negated_loss = mutual_information_recursion(px=px, py=py, boundary=boundary_i, calc_gradients=False)
        return _reduce(negated_loss, reduction)
    return _PrunedLoss.apply(logits, symbols_i, ranges_i, termination_symbol, boundary_i, rnnt_type != "regular",
                             _penalty(delay_penalty), code, hat)


def hat_loss_pruned(
    logits: torch.Tensor,
    symbols: torch.Tensor,
    ranges: torch.Tensor,
    termination_symbol: int,
    boundary: torch.Tensor = None,
    rnnt_type: str = "regular",
    delay_penalty: float = 0.0,
    reduction: Optional[str] = "mean",
) -> torch.Tensor:
    """HAT form of ``rnnt_loss_pruned`` (MI355X addition, no reference counterpart): the lattices of
    ``get_hat_logprobs_pruned`` through the same routes (the band-native recursion for ranges that are a band with
    r <= 15, the full-size lattices otherwise), delay penalty and reduction as there.  Prune ranges come from the
    ordinary ``rnnt_loss_simple``, as in the usual pruned HAT recipe."""
    return _pruned_loss(logits, symbols, ranges, termination_symbol, boundary, rnnt_type, delay_penalty, reduction, True)


def hat_loss(
    logits: torch.Tensor,
    symbols: torch.Tensor,
    termination_symbol: int,
    boundary: Optional[torch.Tensor] = None,
    rnnt_type: str = "regular",
    delay_penalty: float = 0.0,
    reduction: Optional[str] = "mean",
) -> torch.Tensor:
    """HAT form of ``rnnt_loss`` on unpruned joiner logits [B,T,S+1,C] (MI355X addition): ``hat_loss_pruned`` with
    identity ranges."""
    _check_type(rnnt_type)
    boundary = _as_boundary(boundary, logits.shape[0], logits.device)
    return hat_loss_pruned(logits=logits, symbols=symbols, ranges=_joint_inputs(logits, symbols),
                           termination_symbol=termination_symbol, boundary=boundary, rnnt_type=rnnt_type,
                           delay_penalty=delay_penalty, reduction=reduction)


# ---- knowledge distillation on the pruned band (MI355X addition, no reference counterpart)

_KD_MODES = {"full": _lib.FTR_KD_FULL, "collapsed": _lib.FTR_KD_COLLAPSED}
_KD_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def _kd_head(x, y):
    """(logits, kind, teacher_logits, teacher_kind) of the ftr_pruned_kd_* entry points"""
    return (_ptr(x), _LOWP_KIND.get(x.dtype, _lib.FTR_DTYPE_F32), _ptr(y), _LOWP_KIND.get(y.dtype, _lib.FTR_DTYPE_F32))


def _check_kd_dtype(name, t) -> None:
    if t.dtype not in _KD_DTYPES:
        raise TypeError(f"{name} must be float32, bfloat16 or float16, got {t.dtype}")


def _temperature_ok(temperature) -> bool:
    return 0.0 < float(temperature) < float("inf")


def _check_temperature(temperature) -> float:
    temperature = float(temperature)
    if not _temperature_ok(temperature):
        raise ValueError(f"temperature must be a finite number > 0, given {temperature}")
    return temperature


def _check_node_weights(node_weights, shape) -> None:
    """the dtype, then the shape against (B, T, s_range)"""
    if node_weights.dtype != torch.float32:
        raise TypeError(f"node_weights must be float32, got {node_weights.dtype}")
    if tuple(node_weights.shape) != tuple(shape):
        raise ValueError(f"node_weights must be [B,T,s_range] = {tuple(shape)}, got {tuple(node_weights.shape)}")


def _kd_reduce(utt, code, st):
    """the utterance losses [B] under the reduction: themselves for "none", else their mean / sum, one launch on stream ``st``"""
    if code == 0:
        return utt
    out = torch.empty((), dtype=torch.float32, device=utt.device)
    _lib.call("ftr_pruned_kd_reduce_f32", _ptr(utt), utt.shape[0], code, _ptr(out), st)
    return out


def rnnt_kd_loss_pruned(
    logits: torch.Tensor,
    teacher_logits: torch.Tensor,
    symbols: torch.Tensor,
    ranges: torch.Tensor,
    termination_symbol: int,
    boundary: Optional[torch.Tensor] = None,
    mode: str = "full",
    temperature: float = 1.0,
    reduction: Optional[str] = "mean",
) -> torch.Tensor:
    """Knowledge distillation on the pruned band (MI355X addition, no reference counterpart): the KL divergence between a
    teacher's and the student's joiner distributions at every node of the band, to be added to the transducer loss::

        loss = rnnt_loss_pruned(logits, ...) + lam * rnnt_kd_loss_pruned(logits, teacher_logits, ...)

    (``rnnt_loss_pruned_kd`` returns these two values from one pass over the student.)  ``logits`` (student) and ``teacher_logits`` are both [B,T,s_range,C], the teacher's joiner evaluated on the student's
    ``ranges``; each is float32, bfloat16 or float16, independently (a 16-bit tensor means its exact float32 values).

    Node (b,t,k) with s = ranges[b,t,k] is valid iff t_begin <= t < t_end and s_begin <= s <= s_end (``boundary[b]`` =
    (s_begin, t_begin, s_end, t_end); None = the whole lattice).  An invalid node adds nothing, gets a zero gradient
    row, and its logits are never read, so padding frames may hold anything, NaN included.

    ``mode="full"``: KL(p || q) = sum_c p_c (log p_c - log q_c) over the C columns, p = softmax(teacher / temperature),
    q = softmax(student / temperature).  ``mode="collapsed"`` (Panchapagesan et al., ICASSP 2021): the same over three
    classes -- blank, the correct next symbol ``symbols[b,s]`` (only where s < s_end and it is not the blank), and the
    rest, summed over the other columns.  Terms of teacher probability 0 are 0.  The loss is NOT multiplied by
    temperature ** 2; scale ``lam`` if you follow that convention.

    The loss of an utterance is the sum over its valid nodes; ``reduction``: "none" ([B]), "sum", or "mean" (over the
    batch).  Float32, bit-identical from run to run.  The gradient goes to ``logits`` only, in its dtype (computed in
    float32, rounded once); ``teacher_logits`` never gets one.  A NaN in a valid row makes its utterance's loss NaN; a
    student logit of -inf where the teacher has mass makes it +inf."""
    return rnnt_kd_loss_pruned_factored(logits, teacher_logits, symbols, ranges, termination_symbol, boundary,
                                        factorization="softmax", mode=mode, temperature=temperature, reduction=reduction)


_KD_FACTORIZATIONS = {"softmax": _lib.FTR_KD_FACT_SOFTMAX, "hat": _lib.FTR_KD_FACT_HAT, "tdt": _lib.FTR_KD_FACT_TDT}


class _PrunedKdLoss(torch.autograd.Function):
    """rnnt_kd_loss_pruned_factored as one node (the entries of include/ftr_kd_fact.h): forward = one pass over both tensors
    (node losses and the row normalisers the backward needs) + the per-utterance sum [+ the batch reduction]; backward = one
    streaming pass that writes d loss / d logits in the student's dtype, the upstream gradient folded in.  Neither the
    teacher nor the node weights get a gradient."""

    @staticmethod
    def forward(ctx, logits, teacher_logits, symbols, ranges, termination_symbol, boundary, mode, temperature, code, fact,
                n_dur, dur_weight, weights):
        B, T, r, C = logits.shape
        S = symbols.shape[1]
        x = logits.detach().contiguous()
        y = teacher_logits.detach().contiguous()
        planes = (4 if mode == _lib.FTR_KD_COLLAPSED else 2) + (2 if n_dur > 0 else 0)
        node = torch.empty((B, T, r), dtype=torch.float32, device=x.device)
        saved = torch.empty((planes, B, T, r), dtype=torch.float32, device=x.device)
        utt = torch.empty((B,), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            st = _stream_ptr(x)
            _lib.call("ftr_pruned_kd_fact_fwd_dt", *_kd_head(x, y), _ptr(symbols), _ptr(ranges), _ptr(boundary),
                      int(termination_symbol), float(temperature), mode, _ptr(node), _ptr(saved), _ptr(utt), B, T, S, C, r,
                      fact, n_dur, float(dur_weight), _ptr(weights), st)
            out = _kd_reduce(utt, code, st)
        if logits.requires_grad:
            ctx.save_for_backward(x, y, symbols, ranges, saved, boundary, weights)
        ctx.meta = (int(termination_symbol), mode, float(temperature), int(code), fact, n_dur, float(dur_weight))
        return out

    @staticmethod
    def backward(ctx, g_loss):
        x, y, symbols, ranges, saved, boundary, weights = ctx.saved_tensors
        blank, mode, temperature, code, fact, n_dur, dur_weight = ctx.meta
        B, T, r, C = x.shape
        scale, stride, mul = _upstream_scale(g_loss, code, B)   # its multiplier negates: this loss is not a negated score
        g = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.call("ftr_pruned_kd_fact_bwd_scaled_dt", *_kd_head(x, y), _ptr(symbols), _ptr(ranges), _ptr(boundary), blank,
                      temperature, mode, _ptr(saved), _ptr(scale), stride, -mul, _ptr(g), B, T, symbols.shape[1], C, r,
                      fact, n_dur, dur_weight, _ptr(weights), _stream_ptr(x))
        return (g,) + (None,) * 12


def rnnt_kd_loss_pruned_factored(
    logits: torch.Tensor,
    teacher_logits: torch.Tensor,
    symbols: torch.Tensor,
    ranges: torch.Tensor,
    termination_symbol: int,
    boundary: Optional[torch.Tensor] = None,
    factorization: str = "softmax",
    num_durations: int = 0,
    mode: str = "full",
    temperature: float = 1.0,
    duration_weight: float = 1.0,
    node_weights: Optional[torch.Tensor] = None,
    reduction: Optional[str] = "mean",
) -> torch.Tensor:
    """``rnnt_kd_loss_pruned`` for joiner rows that are not one softmax, and with per-node weights (MI355X addition, no
    reference counterpart).  Everything not said here -- shapes, dtypes, validity of a node, ``mode``, ``temperature`` (no
    temperature ** 2 factor), ``reduction``, NaN and -inf, no teacher gradient -- is as in ``rnnt_kd_loss_pruned``.
    Below a = student row / temperature, b = teacher row / temperature, Bk = ``termination_symbol``.

    ``factorization="softmax"``: the loss of ``rnnt_kd_loss_pruned``; without ``node_weights``, bit for bit.

    ``factorization="hat"`` (the rows of ``hat_loss_pruned``; C >= 2): the blank is a sigmoid of its own column,
    qb = sigmoid(a_Bk), and the symbols a softmax u over the columns c != Bk; pb and v likewise from the teacher.
    ``mode="full"``: KL(Bernoulli(pb) || Bernoulli(qb)) + (1 - pb) sum_{c != Bk} v_c (log v_c - log u_c).
    ``mode="collapsed"``: the KL over three classes of masses pb, (1 - pb) v_sym and (1 - pb) (1 - v_sym), the last summed
    over the columns that are neither the blank nor the correct symbol::

        loss = hat_loss_pruned(logits, ...) + lam * rnnt_kd_loss_pruned_factored(logits, teacher_logits, symbols, ranges,
                                                                                 blank, boundary, factorization="hat")

    ``factorization="tdt"`` (the rows of ``rnnt_loss_tdt_pruned`` / ``rnnt_loss_tdt_mixed_pruned``): the last dimension
    is C + N with N = ``num_durations`` in 1..5; the first C columns are the token head (``termination_symbol`` < C), the
    last N the duration head.  Node loss = KL_tok + ``duration_weight`` * KL_dur: KL_tok is the loss of
    ``rnnt_kd_loss_pruned`` in the given ``mode`` over the token columns, KL_dur always the full KL of the two duration
    softmaxes; with ``duration_weight=1`` and ``mode="full"`` that is the KL of the joint token x duration distributions.
    The logits are read where they are: no ``logits[..., :C].contiguous()``.  ``duration_weight`` must be finite and
    >= 0; with 0 the duration columns are ignored, whatever they hold, and get exact zeros.  For the other two factorizations
    ``num_durations`` must be 0::

        loss = rnnt_loss_tdt_pruned(logits, ...) + lam * rnnt_kd_loss_pruned_factored(
            logits, teacher_logits, symbols, ranges, blank, boundary, factorization="tdt", num_durations=len(durations))

    ``node_weights``: None, or a float32 [B,T,s_range] tensor on the device (made contiguous; it never gets a
    gradient).  The loss of node (b,t,k) and its gradient row are multiplied by w[b,t,k]; a weight of exactly 0 makes
    the node invalid -- its rows are not read and its loss and gradient row are zeros, whatever the rows hold -- and a
    NaN weight on an otherwise valid node makes its utterance's loss NaN.  Weights are the caller's contract (finite,
    >= 0): nothing is checked on the host and nothing synchronises.  The intended use is to distil where the student's
    own alignment is, with the detached band occupancies that ``rnnt_loss_simple(..., calc_gradients=True)`` returned as
    ``px_grad`` [B,S,T+1] / ``py_grad`` [B,S+1,T]::

        idx = ranges.long().transpose(1, 2)                                        # [B,s_range,T], rows s of the band
        w = torch.gather(py_grad.detach(), 1, idx).transpose(1, 2).contiguous()    # occupancy of the blank arc at (s,t)
        # and / or the symbol arcs: torch.gather(px_grad.detach()[:, :, :T], 1, idx.clamp(max=S - 1))
        kd = rnnt_kd_loss_pruned_factored(logits, teacher_logits, symbols, ranges, blank, boundary, node_weights=w)

    Those occupancies are the simple model's (``am + lm``) and cover the blank arcs.  The exact node occupancies of the
    joiner being trained come from ``rnnt_node_occupancy_pruned(logits, symbols, ranges, blank, boundary)``, and
    ``rnnt_loss_pruned_kd_factored(..., node_weights="occupancy")`` returns the transducer loss and this loss weighted by
    them from one pass over the student: the recommended form.
    """
    _check_kd_dtype("logits", logits)
    _check_kd_dtype("teacher_logits", teacher_logits)
    if logits.dim() != 4:
        raise ValueError("logits must be [B,T,s_range,C]")
    if tuple(teacher_logits.shape) != tuple(logits.shape):
        raise ValueError(f"teacher_logits must have the shape of logits {tuple(logits.shape)}, got {tuple(teacher_logits.shape)}")
    if factorization not in _KD_FACTORIZATIONS:
        raise ValueError(f"factorization should be ('softmax' | 'hat' | 'tdt'), given {factorization}")
    if mode not in _KD_MODES:
        raise ValueError(f"mode should be ('full' | 'collapsed'), given {mode}")
    temperature = _check_temperature(temperature)
    W = logits.shape[3]
    num_durations = int(num_durations)
    duration_weight = float(duration_weight)
    if factorization == "tdt":
        if not 1 <= num_durations <= _lib.FTR_KD_FACT_MAX_DUR:
            raise ValueError(f"num_durations must be in [1,{_lib.FTR_KD_FACT_MAX_DUR}] for factorization 'tdt', given {num_durations}")
        if num_durations >= W:
            raise ValueError(f"num_durations {num_durations} leaves no token column in rows of {W}")
        if not (0.0 <= duration_weight < float("inf")):
            raise ValueError(f"duration_weight must be a finite number >= 0, given {duration_weight}")
    elif num_durations != 0:
        raise ValueError(f"num_durations must be 0 for factorization '{factorization}', given {num_durations}")
    C = W - num_durations
    if factorization == "hat" and C < 2:
        raise ValueError(f"factorization 'hat' needs a blank and at least one other column, got C = {C}")
    code = _reduction_code(reduction)
    if not 0 <= int(termination_symbol) < C:
        raise ValueError(f"termination_symbol {termination_symbol} not in [0,{C})")
    if node_weights is not None:
        _check_node_weights(node_weights, logits.shape[:3])
    symbols, ranges, boundary = _pruned_inputs(logits, symbols, ranges, boundary, lowp=True)
    _require_gpu(teacher_logits, "teacher_logits")
    if teacher_logits.device != logits.device:
        raise ValueError("teacher_logits and logits must be on the same device")
    if node_weights is not None:
        _require_gpu(node_weights, "node_weights")
        if node_weights.device != logits.device:
            raise ValueError("node_weights and logits must be on the same device")
        node_weights = node_weights.detach().contiguous()
    return _PrunedKdLoss.apply(logits, teacher_logits, symbols, ranges, int(termination_symbol), boundary, _KD_MODES[mode],
                               temperature, code, _KD_FACTORIZATIONS[factorization], num_durations, duration_weight, node_weights)


_KD_TOPK_S = 2 ** 31 - 1   # the `S` of the ftr_pruned_kd_topk_* entries: the op takes no symbols, the boundary alone bounds s


class _PrunedKdTopkLoss(torch.autograd.Function):
    """rnnt_kd_loss_pruned_topk as one node (the entries of include/ftr_kd_topk.h): forward = one pass over the student and
    the cache (node losses and the three row normalisers the backward needs) + the per-utterance sum [+ the batch
    reduction]; backward = one streaming pass that writes d loss / d logits in the student's dtype, the upstream gradient
    folded in.  Nothing of the teacher cache, nor the node weights, gets a gradient."""

    @staticmethod
    def forward(ctx, logits, values, indices, ranges, tranges, boundary, rest, weights, temperature, code):
        B, T, r, C = logits.shape
        rt, K = values.shape[2], values.shape[3]
        x = logits.detach().contiguous()
        node = torch.empty((B, T, r), dtype=torch.float32, device=x.device)
        saved = torch.empty((3, B, T, r), dtype=torch.float32, device=x.device)
        utt = torch.empty((B,), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            st = _stream_ptr(x)
            _lib.call("ftr_pruned_kd_topk_fwd_dt", *_kd_head(x, values), _ptr(indices), _ptr(ranges), _ptr(tranges), _ptr(boundary),
                      _ptr(rest), _ptr(weights), float(temperature), _ptr(node), _ptr(saved), _ptr(utt), B, T, _KD_TOPK_S, C, r,
                      rt, K, st)
            out = _kd_reduce(utt, code, st)
        if logits.requires_grad:
            ctx.save_for_backward(x, values, indices, ranges, saved, tranges, boundary, rest, weights)
        ctx.meta = (float(temperature), int(code))
        return out

    @staticmethod
    def backward(ctx, g_loss):
        x, values, indices, ranges, saved, tranges, boundary, rest, weights = ctx.saved_tensors
        temperature, code = ctx.meta
        B, T, r, C = x.shape
        scale, stride, mul = _upstream_scale(g_loss, code, B)   # its multiplier negates: this loss is not a negated score
        g = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.call("ftr_pruned_kd_topk_bwd_scaled_dt", *_kd_head(x, values), _ptr(indices), _ptr(ranges), _ptr(tranges),
                      _ptr(boundary), _ptr(rest), _ptr(weights), temperature, _ptr(saved), _ptr(scale), stride, -mul, _ptr(g), B, T,
                      _KD_TOPK_S, C, r, values.shape[2], values.shape[3], _stream_ptr(x))
        return (g,) + (None,) * 9


def rnnt_kd_loss_pruned_topk(
    logits: torch.Tensor,
    teacher_values: torch.Tensor,
    teacher_indices: torch.Tensor,
    ranges: torch.Tensor,
    boundary: Optional[torch.Tensor] = None,
    teacher_ranges: Optional[torch.Tensor] = None,
    teacher_rest: Optional[torch.Tensor] = None,
    temperature: float = 1.0,
    node_weights: Optional[torch.Tensor] = None,
    reduction: Optional[str] = "mean",
) -> torch.Tensor:
    """``rnnt_kd_loss_pruned`` (full mode) against a STORED teacher: the top-K logits of every teacher row, their columns and,
    optionally, the mass of everything else -- a cache written by ``rnnt_kd_topk_teacher`` on the teacher's OWN prune
    ranges, read where it lies (MI355X addition, no reference counterpart).  No dense teacher tensor is built, and the
    teacher's joiner is not evaluated on the student's ranges.

    ``logits`` [B,T,s_range,C] is the student on ``ranges`` [B,T,s_range]; float32, bfloat16 or float16.
    ``teacher_values`` [B,T,r_t,K], 1 <= K <= 64: the raw teacher logits at the stored columns, float32, bfloat16 or
    float16 independently of the student (a 16-bit tensor means its exact float32 values).  ``teacher_indices``
    [B,T,r_t,K] int32: those columns, clamped into [0,C); I is the set of a row's indices.  A row with fewer than K
    entries is padded with value -inf; an index may repeat a real entry's only with value -inf.  ``teacher_ranges``
    [B,T,r_t] int32: the teacher's band, of which only ``teacher_ranges[b,t,0]`` is read -- the rows of a frame are taken to
    be consecutive, which is what ``get_rnnt_prune_ranges`` returns; None = the student's ``ranges`` (then r_t must be
    s_range).  ``teacher_rest`` [B,T,r_t] float32: logsumexp over c not in I of teacher_row[c] / temperature, the
    unnormalised mass of the columns that were not stored, AT THE TEMPERATURE OF THIS CALL; None (= -inf everywhere) is the
    renormalised top-K form, the KL against the softmax over the stored columns alone.

    Node (b,t,k) with s = ranges[b,t,k] is distilled iff it is valid as in ``rnnt_kd_loss_pruned`` (``boundary`` None =
    every frame and every s >= 0: this op takes no symbols and does not know S), its weight is not 0, and
    k' = s - teacher_ranges[b,t,0] lies in [0, r_t); its teacher row is (b,t,k').  Any other node adds nothing, gets an
    exact zero gradient row, and neither its student row nor any teacher row is read for it.  With a = student row /
    temperature, v = values / temperature, R = rest::

        L = logaddexp(logsumexp_k v_k, R);  p_k = exp(v_k - L);  p_R = exp(R - L)
        q_k = softmax(a)[idx_k];  log q_R = logsumexp_{c not in I} a_c - logsumexp_c a_c
        node loss = w * (sum_k xlogy(p_k, p_k / q_k) + xlogy(p_R, p_R / q_R))

    -- the KL between the teacher and the student, both coarsened to the K stored columns plus one "rest" class; with
    K = C it is the loss of ``rnnt_kd_loss_pruned``.  Terms of teacher mass 0 are 0; there is no temperature ** 2 factor; a
    stored column where the student has -inf gives +inf.  ``node_weights`` (None or float32 [B,T,s_range]): as in
    ``rnnt_kd_loss_pruned_factored`` -- an exact 0 takes the node out, a NaN poisons its utterance.  ``reduction`` and the
    loss of an utterance (the sum over its distilled nodes): as in ``rnnt_kd_loss_pruned``.  Float32, bit-identical from run
    to run, launches only (a step can be captured in a graph).  The gradient goes to ``logits`` only, in its dtype.

    A band that rarely overlaps the teacher's distils nothing, silently.  The number to watch is the per-utterance count of
    distilled nodes::

        t = torch.arange(T, device=ranges.device)[None, :, None]
        sb, tb, se, te = (boundary[:, i, None, None] for i in range(4))          # None: 0, 0, S, T
        valid = (t >= tb) & (t < te) & (ranges >= sb) & (ranges <= se)
        kp = ranges - teacher_ranges[:, :, :1]
        distilled = (valid & (kp >= 0) & (kp < teacher_ranges.shape[2])).sum((1, 2))    # [B]
    """
    _check_kd_dtype("logits", logits)
    _check_kd_dtype("teacher_values", teacher_values)
    if teacher_indices.dtype != torch.int32:
        raise TypeError(f"teacher_indices must be int32, got {teacher_indices.dtype}")
    for name, t in (("teacher_rest", teacher_rest), ("node_weights", node_weights)):
        if t is not None and t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {t.dtype}")
    if logits.dim() != 4:
        raise ValueError("logits must be [B,T,s_range,C]")
    B, T, r, C = logits.shape
    if teacher_values.dim() != 4 or tuple(teacher_values.shape[:2]) != (B, T) or teacher_values.shape[2] < 1:
        raise ValueError(f"teacher_values must be [B,T,r_t,K] with B, T = {B}, {T} and r_t >= 1, got {tuple(teacher_values.shape)}")
    rt, K = teacher_values.shape[2], teacher_values.shape[3]
    if not 1 <= K <= _lib.FTR_KD_TOPK_MAX_K:
        raise ValueError(f"K = {K} stored columns per row, must be in [1,{_lib.FTR_KD_TOPK_MAX_K}]")
    if tuple(teacher_indices.shape) != tuple(teacher_values.shape):
        raise ValueError(f"teacher_indices must have the shape of teacher_values {tuple(teacher_values.shape)}, got {tuple(teacher_indices.shape)}")
    if teacher_ranges is None:
        if rt != r:
            raise ValueError(f"without teacher_ranges the cache lies on the student's ranges: r_t = {rt} must be s_range = {r}")
    elif not isinstance(teacher_ranges, torch.Tensor) or tuple(teacher_ranges.shape) != (B, T, rt):
        raise ValueError(f"teacher_ranges must be a [B,T,r_t] = {(B, T, rt)} tensor")
    if teacher_rest is not None and tuple(teacher_rest.shape) != (B, T, rt):
        raise ValueError(f"teacher_rest must be [B,T,r_t] = {(B, T, rt)}, got {tuple(teacher_rest.shape)}")
    if node_weights is not None:
        _check_node_weights(node_weights, (B, T, r))   # its dtype has answered above, with teacher_rest's
    temperature = _check_temperature(temperature)
    code = _reduction_code(reduction)
    _require_gpu(logits, "logits")
    ranges = torch.as_tensor(ranges, device=logits.device).to(torch.int32).contiguous()
    if tuple(ranges.shape) != (B, T, r):
        raise ValueError(f"ranges must have shape {(B, T, r)}, got {tuple(ranges.shape)}")
    boundary = _as_boundary(boundary, B, logits.device)
    others = [("teacher_values", teacher_values), ("teacher_indices", teacher_indices), ("teacher_ranges", teacher_ranges),
              ("teacher_rest", teacher_rest), ("node_weights", node_weights)]
    for name, t in others:
        if t is not None:
            _require_gpu(t, name)
            if t.device != logits.device:
                raise ValueError(f"{name} and logits must be on the same device")
    values, indices, tranges, rest, weights = (None if t is None else t.detach().contiguous() for _, t in others)
    if tranges is not None and tranges.dtype != torch.int32:
        tranges = tranges.to(torch.int32)
    return _PrunedKdTopkLoss.apply(logits, values, indices, ranges, tranges, boundary, rest, weights, temperature, code)


def rnnt_kd_topk_teacher(teacher_logits: torch.Tensor, k: int, temperature: float = 1.0,
                         with_rest: bool = True) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """The cache ``rnnt_kd_loss_pruned_topk`` reads, from dense teacher logits [..., C] (the teacher's joiner on the teacher's
    own ranges, [B,T,r_t,C]): ``(values, indices, rest)``.  ``values`` [..., k]: the k largest raw logits of every row, in
    the dtype of ``teacher_logits``; ``indices`` [..., k] int32: their columns; ``rest`` [...] float32 (None without
    ``with_rest``): logsumexp of the other columns / ``temperature`` -- -inf when k = C -- which is only right for a loss
    evaluated at that same temperature.  Plain torch (``topk`` and a masked ``logsumexp``), any device: it runs where the
    cache is written, not in the training step."""
    k = int(k)
    C = teacher_logits.shape[-1]
    if not 1 <= k <= min(C, _lib.FTR_KD_TOPK_MAX_K):
        raise ValueError(f"k = {k} must be in [1, min(C, {_lib.FTR_KD_TOPK_MAX_K})] for rows of C = {C}")
    temperature = _check_temperature(temperature)
    with torch.no_grad():
        values, idx = torch.topk(teacher_logits, k, dim=-1)
        rest = None
        if with_rest:
            others = (teacher_logits.to(torch.float32) / temperature).scatter(-1, idx, _NEG_INF)
            rest = torch.logsumexp(others, dim=-1)
    return values, idx.to(torch.int32), rest


class _PrunedLossKd(torch.autograd.Function):
    """rnnt_loss_pruned / hat_loss_pruned (band route) and rnnt_kd_loss_pruned_factored as one node: forward = one pass over
    both tensors (node losses, the saved normalisers and the student's logsumexp) + band gather + the per-utterance sum,
    then the band recursion and the two reductions, which are the launches of the two ops; backward = one streaming pass
    that writes the sum of both gradients, each under its own upstream gradient, in the student's dtype.
    One softmax (``fact``) without weights runs through the entries of include/ftr_kd_loss.h; a HAT row, node weights
    (``weights``) or the student's own occupancies as weights (``occupancy``) through those of include/ftr_kd_loss_fact.h.
    With ``occupancy`` the row kernel runs without weights and without utterance sums, the occupancies are formed from what
    the band recursion returned, they weight the node losses in the utterance sums' own tree, and the backward takes them
    as its weights."""

    @staticmethod
    def forward(ctx, logits, teacher_logits, symbols, ranges, termination_symbol, boundary, mode, temperature, modified,
                delay_penalty, code, fact, weights, occupancy):
        B, T, r, C = logits.shape
        S = symbols.shape[1]
        x = logits.detach().contiguous()
        y = teacher_logits.detach().contiguous()
        dev = x.device
        lse, pxb, pyb, node = (torch.empty((B, T, r), dtype=torch.float32, device=dev) for _ in range(4))
        saved = torch.empty((4 if mode == _lib.FTR_KD_COLLAPSED else 2, B, T, r), dtype=torch.float32, device=dev)
        utt = torch.empty((B,), dtype=torch.float32, device=dev)
        plain = fact == _lib.FTR_KD_FACT_SOFTMAX and weights is None and not occupancy
        with torch.cuda.device(dev):
            st = _stream_ptr(x)
            _lib.call("ftr_pruned_band_kd_fwd_dt" if plain else "ftr_pruned_band_kd_fact_fwd_dt", *_kd_head(x, y), _ptr(symbols),
                      _ptr(ranges), _ptr(boundary), int(termination_symbol), float(temperature), mode, float(delay_penalty),
                      int(modified), _ptr(lse), _ptr(pxb), _ptr(pyb), _ptr(node), _ptr(saved), None if occupancy else _ptr(utt),
                      B, T, S, C, r, *(() if plain else (fact, _ptr(weights))), st)
            ans, gxb, gyb = band_forward_backward(pxb, pyb, ranges, S, boundary, modified)
            if occupancy:
                weights = _band_occupancy(gxb, gyb, ranges, boundary, S)
                _lib.call("ftr_pruned_kd_weighted_utt_sum_f32", _ptr(node), _ptr(weights), _ptr(utt), B, T, r, st)
            kd = _kd_reduce(utt, code, st)
        del pxb, pyb, node
        if logits.requires_grad:
            ctx.save_for_backward(x, y, symbols, ranges, lse, gxb, gyb, saved, boundary, weights)
        ctx.meta = (int(termination_symbol), mode, float(temperature), int(code), fact, plain)
        ctx.set_materialize_grads(False)      # a part nobody differentiates arrives as None and is not read at all
        return _negated_reduce_native(ans, code), kd

    @staticmethod
    def backward(ctx, g_loss, g_kd):
        x, y, symbols, ranges, lse, gxb, gyb, saved, boundary, weights = ctx.saved_tensors
        blank, mode, temperature, code, fact, plain = ctx.meta
        B, T, r, C = x.shape
        if g_loss is None and g_kd is None:
            return (None,) * 14
        # (pointer tensor, stride, multiplier) of each part; an absent part: multiplier 0, nothing of it is read
        ls, lstride, lmul = _upstream_scale(g_loss, code, B) if g_loss is not None else (None, 0, 0.0)
        ks, kstride, kmul = _upstream_scale(g_kd, code, B) if g_kd is not None else (None, 0, 0.0)
        g = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.call("ftr_pruned_band_kd_bwd_scaled_dt" if plain else "ftr_pruned_band_kd_fact_bwd_scaled_dt", *_kd_head(x, y),
                      _ptr(symbols), _ptr(ranges), _ptr(boundary), blank, temperature, mode, _ptr(lse), _ptr(gxb), _ptr(gyb),
                      _ptr(ls), lstride, lmul, _ptr(saved), _ptr(ks), kstride, -kmul, _ptr(g), B, T, symbols.shape[1], C, r,
                      *(() if plain else (fact, _ptr(weights))), _stream_ptr(x))   # -kmul: kd is not a negated score
        return (g,) + (None,) * 13


def rnnt_loss_pruned_kd(
    logits: torch.Tensor,
    teacher_logits: torch.Tensor,
    symbols: torch.Tensor,
    ranges: torch.Tensor,
    termination_symbol: int,
    boundary: Optional[torch.Tensor] = None,
    mode: str = "full",
    temperature: float = 1.0,
    rnnt_type: str = "regular",
    delay_penalty: float = 0.0,
    reduction: Optional[str] = "mean",
) -> Tuple[torch.Tensor, torch.Tensor]:
    """The transducer loss and the distillation loss of one student tensor in one pass (MI355X addition, no reference
    counterpart)::

        loss, kd = rnnt_loss_pruned_kd(logits, teacher_logits, symbols, ranges, blank, boundary)
        (loss + lam * kd).backward()

    ``loss`` is what ``rnnt_loss_pruned(logits, symbols, ranges, termination_symbol, boundary, rnnt_type, delay_penalty,
    reduction)`` returns and ``kd`` what ``rnnt_kd_loss_pruned(logits, teacher_logits, symbols, ranges, termination_symbol,
    boundary, mode, temperature, reduction)`` returns -- both float32, both under the one ``reduction``, both bit for bit
    -- and the argument checks, dtype rules (student and teacher float32 / bfloat16 / float16, independently; a 16-bit
    tensor means its exact float32 values) and error texts are those of the two functions.  Two outputs, not a weighted
    sum: the caller forms ``loss + lam * kd`` and logs both.

    What one pass saves: the student's row logsumexp is formed once, from the registers that hold the row for the KL (the
    composition forms it twice), and the backward writes ONE gradient tensor in the dtype of ``logits``, each part under
    its own upstream gradient, where the composition writes two and autograd adds them into a third.  The row is computed
    in float32 and rounded once, so it is not the composition's gradient bit for bit (that one rounds each part, then the
    sum).  A part that receives no gradient (``kd.backward()`` alone, ``loss.backward()`` alone) is not read at all --
    neither its occupancies or normalisers nor, for the distillation part, the teacher -- and the row is then that of the
    single op.  The teacher never gets a gradient.

    One difference in what is read: ``rnnt_kd_loss_pruned`` never reads the rows of an invalid node.  Here the STUDENT
    rows of the frames t_begin <= t < t_end whose s lies outside [s_begin, s_end] are read for the transducer loss, as
    ``rnnt_loss_pruned`` reads them (the band recursion conditions its arithmetic on the mean of all band entries of
    those frames); rows of other frames, and every teacher row of an invalid node, stay unread.  Invalid nodes get exact
    zeros in the gradient, whatever their rows hold.

    The fused kernels serve the band route of ``rnnt_loss_pruned``: ranges that are a band with s_range <= 15 (what
    ``get_rnnt_prune_ranges`` returns), ``rnnt_type`` "regular" or "modified", FTR_PRUNED_ROUTE not "lattice".  In every
    other case -- ranges that are no band, s_range >= 16, "constrained", ranges of unknown content under stream capture --
    the two existing functions are called and their two values returned unchanged.  Measured against that composition
    (profiles/kd_loss_bench_c3_c4_c5.jsonl)."""
    _check_type(rnnt_type)
    return _loss_pruned_kd(logits, teacher_logits, symbols, ranges, termination_symbol, boundary, "softmax", mode, temperature,
                           None, rnnt_type, delay_penalty, reduction)


def _loss_pruned_kd(logits, teacher_logits, symbols, ranges, termination_symbol, boundary, factorization, mode, temperature,
                    node_weights, rnnt_type, delay_penalty, reduction):
    """rnnt_loss_pruned_kd and rnnt_loss_pruned_kd_factored behind their own first checks: the fused node where it serves,
    else the functions composed.  ``node_weights``: None, a tensor or "occupancy"."""
    occupancy = isinstance(node_weights, str)
    hat = factorization == "hat"
    w = None if occupancy else node_weights
    args = (logits, symbols, ranges, termination_symbol, boundary)
    fused = rnnt_type != "constrained" and isinstance(logits, torch.Tensor) and isinstance(teacher_logits, torch.Tensor) \
        and logits.dtype in _KD_DTYPES and teacher_logits.dtype in _KD_DTYPES and logits.dim() == 4 \
        and tuple(teacher_logits.shape) == tuple(logits.shape) and logits.is_cuda and teacher_logits.is_cuda \
        and teacher_logits.device == logits.device and mode in _KD_MODES and reduction in _REDUCTIONS \
        and _temperature_ok(temperature) and 0 <= int(termination_symbol) < logits.shape[3] \
        and not (hat and logits.shape[3] < 2) and (w is None or (isinstance(w, torch.Tensor) and w.dtype == torch.float32 and w.device == logits.device
                           and tuple(w.shape) == tuple(logits.shape[:3])))
    if fused:   # everything the composed functions would refuse is refused by them below, in their words
        symbols_i, ranges_i, boundary_i = _pruned_inputs(logits, symbols, ranges, boundary, lowp=True)
        B, T, r, C = logits.shape
        if _band_path_ok(ranges_i, boundary_i, T, symbols_i.shape[1], r):
            return _PrunedLossKd.apply(logits, teacher_logits, symbols_i, ranges_i, int(termination_symbol), boundary_i,
                                       _KD_MODES[mode], float(temperature), rnnt_type != "regular", _penalty(delay_penalty),
                                       _REDUCTIONS[reduction], _KD_FACTORIZATIONS[factorization],
                                       None if w is None else w.detach().contiguous(), occupancy)
        args = (logits, symbols_i, ranges_i, termination_symbol, boundary_i)   # the verdict on the ranges travels with them
    loss = _pruned_loss(*args, rnnt_type, delay_penalty, reduction, hat)
    if occupancy:
        w = rnnt_node_occupancy_pruned(*args, factorization=factorization, rnnt_type=rnnt_type, delay_penalty=delay_penalty)
    kd = rnnt_kd_loss_pruned_factored(args[0], teacher_logits, *args[1:], factorization=factorization, mode=mode,
                                      temperature=temperature, node_weights=w, reduction=reduction)
    return loss, kd


def _band_occupancy(gxb, gyb, ranges, boundary, S):
    """occ [B,T,r] = gx + gy of the band recursion's occupancies under the masks of the band gradient kernel; one launch."""
    B, T, r = ranges.shape
    occ = torch.empty((B, T, r), dtype=torch.float32, device=gxb.device)
    with torch.cuda.device(gxb.device):
        _lib.call("ftr_band_node_occupancy_f32", _ptr(gxb), _ptr(gyb), _ptr(ranges), _ptr(boundary), _ptr(occ), B, T, S, r,
                  _stream_ptr(gxb))
    return occ


def _lattice_occupancy(px_grad, py_grad, ranges, boundary, S):
    """The same from the full-size occupancies of ``mutual_information_recursion``: px_grad [B,S,T(+1)], py_grad [B,S+1,T]
    gathered onto the band, zeros outside the boundary rectangle and outside the lattice."""
    B, T, r = ranges.shape
    s = ranges.long()
    t = torch.arange(T, device=ranges.device).reshape(1, T, 1)
    if boundary is None:
        valid = (s >= 0) & (s <= S)
    else:
        bd = boundary.long().reshape(B, 1, 1, 4)
        sb, tb, se, te = bd[..., 0].clamp(min=0), bd[..., 1].clamp(min=0), bd[..., 2].clamp(max=S), bd[..., 3].clamp(max=T)
        valid = (t >= tb) & (t < te) & (s >= sb) & (s <= se)
    idx = s.clamp(0, S).transpose(1, 2)                                         # [B,r,T], rows s of the band
    occ = torch.gather(py_grad, 1, idx).transpose(1, 2)
    if S > 0:
        gx = torch.gather(px_grad[:, :, :T], 1, idx.clamp(max=S - 1)).transpose(1, 2)
        occ = occ + torch.where(s < S, gx, torch.zeros_like(gx))
    return torch.where(valid, occ, torch.zeros_like(occ)).contiguous()


def _check_loss_kd_factorization(factorization, name):
    if factorization == "tdt":
        raise ValueError(f"{name}: factorization 'tdt' is out of scope here (its transducer gradient needs the occupancies of "
                         "every duration and its logits are float32 only); use rnnt_loss_tdt_pruned + rnnt_kd_loss_pruned_factored")
    if factorization not in ("softmax", "hat"):
        raise ValueError(f"factorization should be ('softmax' | 'hat'), given {factorization}")


def rnnt_node_occupancy_pruned(
    logits: torch.Tensor,
    symbols: torch.Tensor,
    ranges: torch.Tensor,
    termination_symbol: int,
    boundary: Optional[torch.Tensor] = None,
    factorization: str = "softmax",
    rnnt_type: str = "regular",
    delay_penalty: float = 0.0,
) -> torch.Tensor:
    """The student's own node occupancies on the pruned band (MI355X addition, no reference counterpart): float32
    [B,T,s_range], detached.  ``occ[b,t,k]`` is the probability, under the transducer loss of THIS joiner output, that an
    alignment passes through lattice node (ranges[b,t,k], t): the sum of the occupancies of the two arcs that leave the
    node, the symbol arc only where s < S -- exactly what the band gradient kernel multiplies the node's row by.  Nodes
    outside ``boundary`` or outside the lattice get exact zeros.  ``factorization="softmax"``: the loss is
    ``rnnt_loss_pruned``; ``"hat"``: ``hat_loss_pruned``; ``rnnt_type`` and ``delay_penalty`` as there.

    The intended use is as ``node_weights`` of a distillation loss: distil where the student's alignment is.
    ``rnnt_loss_pruned_kd_factored(..., node_weights="occupancy")`` does that in one pass, without this call.

    Cost on the band route (ranges that are a band with s_range <= 15, "regular" / "modified"): the band forward, the band
    recursion and one small kernel; no gradient is formed.  Everywhere else the full-size lattices are built and the
    occupancies of ``mutual_information_recursion`` gathered onto the band.  No gradient flows through the result."""
    _check_type(rnnt_type)
    _check_loss_kd_factorization(factorization, "rnnt_node_occupancy_pruned")
    hat = factorization == "hat"
    with torch.no_grad():
        symbols, ranges, boundary = _pruned_inputs(logits, symbols, ranges, boundary, lowp=True)
        B, T, r, C = logits.shape
        S = symbols.shape[1]
        if hat and C < 2:
            raise ValueError(f"factorization 'hat' needs a blank and at least one other column, got C = {C}")
        if not 0 <= int(termination_symbol) < C:
            raise ValueError(f"termination_symbol {termination_symbol} not in [0,{C})")
        x = logits.detach().contiguous()
        modified = rnnt_type != "regular"
        penalty = _penalty(delay_penalty)
        if rnnt_type != "constrained" and _band_path_ok(ranges, boundary, T, S, r):
            dev = x.device
            lse, pxb, pyb = (torch.empty((B, T, r), dtype=torch.float32, device=dev) for _ in range(3))
            with torch.cuda.device(dev):
                _pruned_call("pruned_band_fwd", hat, x, (_ptr(symbols), _ptr(ranges), _ptr(boundary), int(termination_symbol),
                             penalty, _ptr(lse), _ptr(pxb), _ptr(pyb), B, T, S, C, r, int(modified)), (_stream_ptr(x),))
            _, gxb, gyb = band_forward_backward(pxb, pyb, ranges, S, boundary, modified)
            return _band_occupancy(gxb, gyb, ranges, boundary, S)
        if rnnt_type == "constrained":
            _, px, py = _pruned_builder_fwd(x, symbols, ranges, boundary, termination_symbol, 0.0, modified, hat)
            px = _apply_delay_penalty(px + py[:, 1:, :], boundary, rnnt_type, delay_penalty)
        else:
            _, px, py = _pruned_builder_fwd(x, symbols, ranges, boundary, termination_symbol, penalty, modified, hat)
        _, px_grad, py_grad = mi_forward_backward(px, py, boundary, True, ans_grad_is_one=True)
        return _lattice_occupancy(px_grad, py_grad, ranges, boundary, S)


def rnnt_loss_pruned_kd_factored(
    logits: torch.Tensor,
    teacher_logits: torch.Tensor,
    symbols: torch.Tensor,
    ranges: torch.Tensor,
    termination_symbol: int,
    boundary: Optional[torch.Tensor] = None,
    factorization: str = "softmax",
    mode: str = "full",
    temperature: float = 1.0,
    node_weights=None,
    rnnt_type: str = "regular",
    delay_penalty: float = 0.0,
    reduction: Optional[str] = "mean",
) -> Tuple[torch.Tensor, torch.Tensor]:
    """``rnnt_loss_pruned_kd`` for HAT students and with node weights (MI355X addition, no reference counterpart): the
    transducer loss and the factored distillation loss of one student tensor in one pass::

        loss, kd = rnnt_loss_pruned_kd_factored(logits, teacher_logits, symbols, ranges, blank, boundary,
                                                factorization="hat", node_weights="occupancy")
        (loss + lam * kd).backward()

    ``factorization="softmax"``: ``loss`` is ``rnnt_loss_pruned(logits, symbols, ranges, termination_symbol, boundary,
    rnnt_type, delay_penalty, reduction)``; ``"hat"``: ``hat_loss_pruned`` of the same arguments.  ``"tdt"`` raises
    ValueError: it is out of scope here.  ``kd`` is ``rnnt_kd_loss_pruned_factored(logits, teacher_logits, symbols,
    ranges, termination_symbol, boundary, factorization=factorization, mode=mode, temperature=temperature,
    node_weights=w, reduction=reduction)``.  Both float32, both bit for bit, and the argument checks, dtype rules and
    error texts are those of the functions composed.

    ``node_weights``: None (every node weighs 1); a float32 [B,T,s_range] tensor with the semantics of
    ``rnnt_kd_loss_pruned_factored`` (it multiplies the node's distillation loss and gradient row, a weight of exactly 0
    takes the node out of the distillation, it never gets a gradient); or the string ``"occupancy"``: the weights are the
    detached node occupancies of this student under this loss, ``rnnt_node_occupancy_pruned(logits, symbols, ranges,
    termination_symbol, boundary, factorization, rnnt_type, delay_penalty)``, taken from the very recursion the loss
    runs -- ``kd`` is then, bit for bit, what ``rnnt_kd_loss_pruned_factored`` returns given that tensor.  No gradient
    flows through the occupancy weights.  With ``factorization="softmax"`` and ``node_weights=None`` this is
    ``rnnt_loss_pruned_kd``, the same kernels and the same bits.

    The gradient is one launch: the row is computed in float32 and rounded once in the dtype of ``logits``, each part under
    its own upstream gradient; a part that receives none is not read at all, and the row is then the single op's.  What is
    read is as in ``rnnt_loss_pruned_kd``, plus the weights: the student rows of the rectangle's frames are read for the
    transducer loss even where the distillation weight is 0; the teacher row of a node that is invalid or has weight 0 is
    never read, and in the backward the distillation part of such a row is skipped.

    The fused kernels serve the route of ``rnnt_loss_pruned_kd``: ranges that are a band with s_range <= 15, ``rnnt_type``
    "regular" or "modified", FTR_PRUNED_ROUTE not "lattice".  In every other case the existing functions are called and
    their values returned unchanged (the occupancy weights then come from ``rnnt_node_occupancy_pruned``).  Measured
    against that composition: DESIGN.md section 4t, profiles/kd_loss_fact_bench_c3_c4_c5.jsonl."""
    _check_type(rnnt_type)
    _check_loss_kd_factorization(factorization, "rnnt_loss_pruned_kd_factored")
    occupancy = isinstance(node_weights, str)
    if occupancy and node_weights != "occupancy":
        raise ValueError(f"node_weights should be None, a float32 [B,T,s_range] tensor or 'occupancy', given '{node_weights}'")
    return _loss_pruned_kd(logits, teacher_logits, symbols, ranges, termination_symbol, boundary, factorization, mode, temperature,
                           node_weights, rnnt_type, delay_penalty, reduction)


# ---- multi-blank transducer (MI355X addition, no reference counterpart): big blanks that advance several frames

def _big_blank_args(big_blanks, termination_symbol: int, C: int):
    """(ids, durations) as host int32 arrays for the C ABI, durations[0] = 1 being the standard blank's.  The checks are
    those of the native entry points, raised here as ValueError before anything is allocated."""
    pairs = [(int(i), int(d)) for i, d in big_blanks]
    ids = [i for i, _ in pairs]
    durs = [1] + [d for _, d in pairs]
    if len(durs) > 8:
        raise ValueError(f"at most 7 big blanks are supported, got {len(pairs)}")
    if any(d < 2 or d > 32 for d in durs[1:]) or any(b <= a for a, b in zip(durs, durs[1:])):
        raise ValueError(f"big-blank durations must be strictly increasing values in 2..32, got {durs[1:]}")
    if not 0 <= int(termination_symbol) < C:
        raise ValueError(f"termination_symbol {termination_symbol} not in [0,{C})")
    if any(i < 0 or i >= C or i == int(termination_symbol) for i in ids) or len(set(ids)) != len(ids):
        raise ValueError(f"big-blank ids must be distinct, in [0,{C}) and differ from termination_symbol, got {ids}")
    D = len(durs)
    return (ctypes.c_int32 * max(D - 1, 1))(*ids), (ctypes.c_int32 * D)(*durs), tuple(durs)


def _mb_builder_fwd(x, symbols, ranges, boundary, blank, ids, durs, D, sigma, delay_penalty):
    B, T, r, C = x.shape
    S = symbols.shape[1]
    lse = torch.empty((B, T, r), dtype=torch.float32, device=x.device)
    px = torch.empty((B, S, T + 1), dtype=torch.float32, device=x.device)
    py = torch.empty((B, D, S + 1, T), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call("ftr_multiblank_pruned_logprobs_fwd_f32", _ptr(x), _ptr(symbols), _ptr(ranges), _ptr(boundary), blank,
                  ids, durs, D, float(sigma), float(delay_penalty), _ptr(lse), _ptr(px), _ptr(py), B, T, S, C, r,
                  _stream_ptr(x))
    return lse, px, py


def _mb_band_builder_fwd(x, symbols, ranges, boundary, blank, ids, durs, D, sigma, delay_penalty):
    """_mb_builder_fwd with band-shaped px_band [B,T,r] / py_band [B,D,T,r]: no lattice is written."""
    B, T, r, C = x.shape
    S = symbols.shape[1]
    lse = torch.empty((B, T, r), dtype=torch.float32, device=x.device)
    pxb = torch.empty((B, T, r), dtype=torch.float32, device=x.device)
    pyb = torch.empty((B, D, T, r), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call("ftr_multiblank_pruned_band_fwd_f32", _ptr(x), _ptr(symbols), _ptr(ranges), _ptr(boundary), blank, ids,
                  durs, D, float(sigma), float(delay_penalty), _ptr(lse), _ptr(pxb), _ptr(pyb), B, T, S, C, r, _stream_ptr(x))
    return lse, pxb, pyb


def _mb_builder_bwd(x, symbols, ranges, boundary, blank, ids, durs, D, lse, gpx, gpy, scale, stride, mul, band=False):
    """``band``: gpx / gpy are band-shaped occupancies [B,T,r] / [B,D,T,r], else the full-size lattices."""
    B, T, r, C = x.shape
    S = symbols.shape[1]
    g = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.call("ftr_multiblank_pruned_band_bwd_scaled_f32" if band else "ftr_multiblank_pruned_logprobs_bwd_scaled_f32",
                  _ptr(x), _ptr(symbols), _ptr(ranges), _ptr(boundary), blank, ids, durs, D, _ptr(lse), _ptr(gpx), _ptr(gpy),
                  _ptr(scale), stride, mul, _ptr(g), B, T, S, C, r, _stream_ptr(x))
    return g


class _MultiblankLogprobs(torch.autograd.Function):
    """get_rnnt_logprobs_multiblank_pruned: one gather launch (after the ordinary logsumexp) and one gradient launch."""

    @staticmethod
    def forward(ctx, logits, symbols, ranges, termination_symbol, big_blanks, boundary, sigma):
        x = logits.detach().contiguous()
        ids, durs, dt = _big_blank_args(big_blanks, termination_symbol, x.shape[3])
        lse, px, py = _mb_builder_fwd(x, symbols, ranges, boundary, int(termination_symbol), ids, durs, len(dt), sigma, 0.0)
        ctx.save_for_backward(x, symbols, ranges, lse, boundary)
        ctx.meta = (int(termination_symbol), ids, durs, len(dt))
        return px, py

    @staticmethod
    def backward(ctx, gpx, gpy):
        x, symbols, ranges, lse, boundary = ctx.saved_tensors
        blank, ids, durs, D = ctx.meta
        g = _mb_builder_bwd(x, symbols, ranges, boundary, blank, ids, durs, D, lse, gpx.contiguous(), gpy.contiguous(),
                            None, 0, 1.0)
        return g, None, None, None, None, None, None


def _mb_band_path_ok(ranges, boundary, T: int, S: int, r: int, D: int) -> bool:
    """_band_path_ok for the multi-blank loss: the same rule and the same FTR_PRUNED_ROUTE knob, the multi-blank domain
    of csrc/mi_band_tdt.hip."""
    if os.environ.get("FTR_PRUNED_ROUTE") == "lattice":
        return False
    return band_multiblank_supported(T, S, r, D) and _is_band(ranges, boundary)


class _MultiblankLoss(torch.autograd.Function):
    """rnnt_loss_multiblank_pruned with the whole chain native, as _PrunedLoss.

    Band path (the ranges are a band, r <= 15): logsumexp + band gather -> multi-blank recursion, both directions and the
    occupancies, on the band [B,T,r] / [B,D,T,r] (ftr_mutual_information_band_multiblank_f32; no full-size lattice exists)
    -> in backward() one streaming kernel turns the band-shaped occupancies * upstream gradient into d loss / d logits.
    Lattice path (any other ranges, FTR_PRUNED_ROUTE=lattice): logsumexp + band->lattice, multi-blank recursion forward
    and backward on the full-size lattices, the same streaming kernel fed from the lattices."""

    @staticmethod
    def forward(ctx, logits, symbols, ranges, termination_symbol, big_blanks, boundary, sigma, delay_penalty, code):
        x = logits.detach().contiguous()
        need = logits.requires_grad
        ids, durs, dt = _big_blank_args(big_blanks, termination_symbol, x.shape[3])
        B, T, r, _ = x.shape
        S = symbols.shape[1]
        ctx.band = _mb_band_path_ok(ranges, boundary, T, S, r, len(dt))
        if ctx.band:
            lse, px, py = _mb_band_builder_fwd(x, symbols, ranges, boundary, int(termination_symbol), ids, durs, len(dt), sigma,
                                               delay_penalty)
            ans, px_grad, py_grad = band_multiblank_forward_backward(px, py, ranges, S, dt, boundary, need)
        else:
            lse, px, py = _mb_builder_fwd(x, symbols, ranges, boundary, int(termination_symbol), ids, durs, len(dt), sigma,
                                          delay_penalty)
            ans, px_grad, py_grad = mb_forward_backward(px, py, dt, boundary, need)
        del px, py
        if need:
            ctx.save_for_backward(x, symbols, ranges, lse, px_grad, py_grad, boundary)
        ctx.meta = (int(termination_symbol), ids, durs, len(dt), int(code))
        return _negated_reduce_native(ans, code)

    @staticmethod
    def backward(ctx, g_loss):
        x, symbols, ranges, lse, px_grad, py_grad, boundary = ctx.saved_tensors
        blank, ids, durs, D, code = ctx.meta
        scale, stride, mul = _upstream_scale(g_loss, code, x.shape[0])
        g = _mb_builder_bwd(x, symbols, ranges, boundary, blank, ids, durs, D, lse, px_grad, py_grad, scale, stride, mul,
                            ctx.band)
        return g, None, None, None, None, None, None, None, None


def _check_sigma(sigma) -> float:
    sigma = float(sigma)
    if not sigma >= 0.0:
        raise ValueError(f"sigma must not be negative, got {sigma}")
    return sigma


def get_rnnt_logprobs_multiblank_pruned(
    logits: torch.Tensor,
    symbols: torch.Tensor,
    ranges: torch.Tensor,
    termination_symbol: int,
    big_blanks,
    boundary: torch.Tensor,
    sigma: float = 0.0,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Multi-blank form of ``get_rnnt_logprobs_pruned`` (Xu et al., "Multi-blank Transducers for Speech Recognition",
    ICASSP 2023; MI355X addition, regular type only).  ``big_blanks`` is a sequence of ``(symbol_id, duration)`` pairs:
    ordinary vocabulary entries whose emission advances ``duration`` frames; ids distinct, in [0,C), not the
    termination_symbol; durations strictly increasing in 2..32; at most 7 pairs; ``()`` is valid.

    logits [B,T,s_range,C] -> ``px`` [B,S,T+1] and ``py`` [B,D,S+1,T] with D = 1 + len(big_blanks) and
    durations = (1, d_1, ...): ``py[b,j,s,t]`` is the log-probability of blank j at (s,t), the move to (s,t+d_j), and
    is -inf where ``t + d_j > t_end``.  Each row is normalised by the ordinary softmax over all C columns and ``sigma``
    (>= 0, the paper's logit under-normalisation) is subtracted from every log-probability.  Both are -inf outside the
    band, px also at column t_end; a symbol that is a big-blank id gets px = -inf and no gradient.  Feed them to
    ``mutual_information_recursion_multiblank(px, py, (1, d_1, ...), boundary)``.  Differentiable w.r.t. ``logits``."""
    symbols, ranges, boundary = _pruned_inputs(logits, symbols, ranges, boundary)
    return _MultiblankLogprobs.apply(logits, symbols, ranges, termination_symbol, tuple(map(tuple, big_blanks)), boundary,
                                     _check_sigma(sigma))


def get_rnnt_logprobs_multiblank_joint(
    logits: torch.Tensor,
    symbols: torch.Tensor,
    termination_symbol: int,
    big_blanks,
    boundary: Optional[torch.Tensor] = None,
    sigma: float = 0.0,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """``get_rnnt_logprobs_multiblank_pruned`` for unpruned joiner logits [B,T,S+1,C], through identity ranges."""
    ranges = _joint_inputs(logits, symbols)
    return get_rnnt_logprobs_multiblank_pruned(logits=logits, symbols=symbols, ranges=ranges,
                                               termination_symbol=termination_symbol, big_blanks=big_blanks,
                                               boundary=boundary, sigma=sigma)


def rnnt_loss_multiblank_pruned(
    logits: torch.Tensor,
    symbols: torch.Tensor,
    ranges: torch.Tensor,
    termination_symbol: int,
    big_blanks,
    boundary: torch.Tensor = None,
    sigma: float = 0.0,
    delay_penalty: float = 0.0,
    reduction: Optional[str] = "mean",
    rnnt_type: str = "regular",
) -> torch.Tensor:
    """Multi-blank transducer loss on pruned joiner logits (MI355X addition): the lattices of
    ``get_rnnt_logprobs_multiblank_pruned`` (with the delay penalty on px as in ``rnnt_loss_pruned``) through
    ``mutual_information_recursion_multiblank``, negated and reduced.  Prune ranges come from the ordinary
    ``rnnt_loss_simple``, as for ``hat_loss_pruned``.  Only ``rnnt_type="regular"`` exists; anything else raises
    ValueError.  With ``big_blanks=()`` and ``sigma=0`` this is ``rnnt_loss_pruned``.
    When ``ranges`` are a band with ``s_range <= 15`` (the rule of ``rnnt_loss_pruned``, ``FTR_PRUNED_ROUTE=lattice``
    overrides it) the same loss is computed on the band itself and no full-size lattice is allocated."""
    if rnnt_type != "regular":
        raise ValueError(f"the multi-blank loss is defined for rnnt_type 'regular' only, given {rnnt_type}")
    code = _reduction_code(reduction)
    symbols_i, ranges_i, boundary_i = _pruned_inputs(logits, symbols, ranges, boundary)
    return _MultiblankLoss.apply(logits, symbols_i, ranges_i, termination_symbol, tuple(map(tuple, big_blanks)), boundary_i,
                                 _check_sigma(sigma), _penalty(delay_penalty), code)


def rnnt_loss_multiblank(
    logits: torch.Tensor,
    symbols: torch.Tensor,
    termination_symbol: int,
    big_blanks,
    boundary: Optional[torch.Tensor] = None,
    sigma: float = 0.0,
    delay_penalty: float = 0.0,
    reduction: Optional[str] = "mean",
    rnnt_type: str = "regular",
) -> torch.Tensor:
    """``rnnt_loss_multiblank_pruned`` for unpruned joiner logits [B,T,S+1,C], through identity ranges."""
    if rnnt_type != "regular":
        raise ValueError(f"the multi-blank loss is defined for rnnt_type 'regular' only, given {rnnt_type}")
    ranges = _joint_inputs(logits, symbols)
    return rnnt_loss_multiblank_pruned(logits=logits, symbols=symbols, ranges=ranges, termination_symbol=termination_symbol,
                                       big_blanks=big_blanks, boundary=boundary, sigma=sigma, delay_penalty=delay_penalty,
                                       reduction=reduction)


# ---- token-and-duration transducer, TDT (MI355X addition, no reference counterpart): a separate duration head

def _tdt_args(durations, termination_symbol: int, width: int):
    """(host int32 array, durations, blank_durations, C) for a joiner row of ``width`` = C + N columns.  The checks are
    those of the native entry points, raised here as ValueError before anything is allocated."""
    durs = tuple(int(d) for d in durations)
    if not 1 <= len(durs) <= 5:
        raise ValueError(f"durations must hold 1..5 values, got {len(durs)}")
    if any(d < 0 or d > 16 for d in durs) or any(b <= a for a, b in zip(durs, durs[1:])):
        raise ValueError(f"durations must be strictly increasing values in 0..16, got {durs}")
    if durs[-1] < 1:
        raise ValueError(f"durations must hold a positive value, got {durs}")
    C = int(width) - len(durs)
    if C < 1:
        raise ValueError(f"logits have {width} columns, fewer than one token column and {len(durs)} duration columns")
    if not 0 <= int(termination_symbol) < C:
        raise ValueError(f"termination_symbol {termination_symbol} not in [0,{C})")
    return (ctypes.c_int32 * len(durs))(*durs), durs, tuple(d for d in durs if d > 0), C


def _tdt_builder_fwd(x, symbols, ranges, boundary, blank, arr, durs, blank_durs, C, sigma, delay_penalty):
    B, T, r, _ = x.shape
    S = symbols.shape[1]
    lse_tok = torch.empty((B, T, r), dtype=torch.float32, device=x.device)
    lse_dur = torch.empty((B, T, r), dtype=torch.float32, device=x.device)
    px = torch.empty((B, len(durs), S, T + 1), dtype=torch.float32, device=x.device)
    py = torch.empty((B, len(blank_durs), S + 1, T), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call("ftr_tdt_pruned_logprobs_fwd_f32", _ptr(x), _ptr(symbols), _ptr(ranges), _ptr(boundary), blank, arr,
                  len(durs), float(sigma), float(delay_penalty), _ptr(lse_tok), _ptr(lse_dur), _ptr(px), _ptr(py), B, T, S, C,
                  r, _stream_ptr(x))
    return lse_tok, lse_dur, px, py


def _tdt_band_builder_fwd(x, symbols, ranges, boundary, blank, arr, durs, blank_durs, C, sigma, delay_penalty):
    """_tdt_builder_fwd with band-shaped px_band [B,N,T,r] / py_band [B,Ny,T,r]: no lattice is written."""
    B, T, r, _ = x.shape
    S = symbols.shape[1]
    lse_tok = torch.empty((B, T, r), dtype=torch.float32, device=x.device)
    lse_dur = torch.empty((B, T, r), dtype=torch.float32, device=x.device)
    pxb = torch.empty((B, len(durs), T, r), dtype=torch.float32, device=x.device)
    pyb = torch.empty((B, len(blank_durs), T, r), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call("ftr_tdt_pruned_band_fwd_f32", _ptr(x), _ptr(symbols), _ptr(ranges), _ptr(boundary), blank, arr,
                  len(durs), float(sigma), float(delay_penalty), _ptr(lse_tok), _ptr(lse_dur), _ptr(pxb), _ptr(pyb), B, T, S, C,
                  r, _stream_ptr(x))
    return lse_tok, lse_dur, pxb, pyb


def _tdt_builder_bwd(x, symbols, ranges, boundary, blank, arr, N, C, sigma, delay_penalty, lse_tok, lse_dur, gpx, gpy, scale,
                     stride, mul, band=False):
    """``band``: gpx / gpy are band-shaped occupancies [B,N,T,r] / [B,Ny,T,r], else the full-size lattices."""
    B, T, r, _ = x.shape
    S = symbols.shape[1]
    g = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.call("ftr_tdt_pruned_band_bwd_scaled_f32" if band else "ftr_tdt_pruned_logprobs_bwd_scaled_f32", _ptr(x),
                  _ptr(symbols), _ptr(ranges), _ptr(boundary), blank, arr, N, float(sigma), float(delay_penalty),
                  _ptr(lse_tok), _ptr(lse_dur), _ptr(gpx), _ptr(gpy), _ptr(scale), stride, mul, _ptr(g), B, T, S, C, r, _stream_ptr(x))
    return g


class _TdtLogprobs(torch.autograd.Function):
    """get_rnnt_logprobs_tdt_pruned: the two log-sum-exps and one gather launch, one gradient launch."""

    @staticmethod
    def forward(ctx, logits, symbols, ranges, termination_symbol, durations, boundary, sigma, delay_penalty):
        x = logits.detach().contiguous()
        arr, durs, blank_durs, C = _tdt_args(durations, termination_symbol, x.shape[3])
        lse_tok, lse_dur, px, py = _tdt_builder_fwd(x, symbols, ranges, boundary, int(termination_symbol), arr, durs,
                                                    blank_durs, C, sigma, delay_penalty)
        ctx.save_for_backward(x, symbols, ranges, lse_tok, lse_dur, boundary)
        ctx.meta = (int(termination_symbol), arr, len(durs), C, sigma, delay_penalty)
        return px, py

    @staticmethod
    def backward(ctx, gpx, gpy):
        x, symbols, ranges, lse_tok, lse_dur, boundary = ctx.saved_tensors
        blank, arr, N, C, sigma, delay_penalty = ctx.meta
        g = _tdt_builder_bwd(x, symbols, ranges, boundary, blank, arr, N, C, sigma, delay_penalty, lse_tok, lse_dur,
                             gpx.contiguous(), gpy.contiguous(), None, 0, 1.0)
        return g, None, None, None, None, None, None, None


def _tdt_band_path_ok(ranges, boundary, T: int, S: int, r: int, N: int, Ny: int) -> bool:
    """_band_path_ok for the TDT loss: the same rule and the same FTR_PRUNED_ROUTE knob, the domain of
    csrc/mi_band_tdt.hip."""
    if os.environ.get("FTR_PRUNED_ROUTE") == "lattice":
        return False
    return band_tdt_supported(T, S, r, N, Ny) and _is_band(ranges, boundary)


class _TdtLoss(torch.autograd.Function):
    """rnnt_loss_tdt_pruned with the whole chain native, as _PrunedLoss.

    Band path (the ranges are a band, r <= 15): log-sum-exps + band gather -> TDT recursion, both directions and the
    occupancies, on the band [B,N|Ny,T,r] (ftr_mutual_information_band_tdt_f32; no full-size lattice exists) -> in
    backward() one streaming kernel turns the band-shaped occupancies * upstream gradient into d loss / d logits.
    Lattice path (any other ranges, FTR_PRUNED_ROUTE=lattice): log-sum-exps + band->lattice, TDT recursion forward and
    backward on the full-size lattices, the same streaming kernel fed from the lattices."""

    @staticmethod
    def forward(ctx, logits, symbols, ranges, termination_symbol, durations, boundary, sigma, delay_penalty, code):
        x = logits.detach().contiguous()
        need = logits.requires_grad
        arr, durs, blank_durs, C = _tdt_args(durations, termination_symbol, x.shape[3])
        B, T, r, _ = x.shape
        S = symbols.shape[1]
        ctx.band = _tdt_band_path_ok(ranges, boundary, T, S, r, len(durs), len(blank_durs))
        if ctx.band:
            lse_tok, lse_dur, px, py = _tdt_band_builder_fwd(x, symbols, ranges, boundary, int(termination_symbol), arr, durs,
                                                             blank_durs, C, sigma, delay_penalty)
            ans, px_grad, py_grad = band_tdt_forward_backward(px, py, ranges, S, durs, blank_durs, boundary, need)
        else:
            lse_tok, lse_dur, px, py = _tdt_builder_fwd(x, symbols, ranges, boundary, int(termination_symbol), arr, durs,
                                                        blank_durs, C, sigma, delay_penalty)
            ans, px_grad, py_grad = tdt_forward_backward(px, py, durs, blank_durs, boundary, need)
        del px, py
        if need:
            ctx.save_for_backward(x, symbols, ranges, lse_tok, lse_dur, px_grad, py_grad, boundary)
        ctx.meta = (int(termination_symbol), arr, len(durs), C, sigma, delay_penalty, int(code))
        return _negated_reduce_native(ans, code)

    @staticmethod
    def backward(ctx, g_loss):
        x, symbols, ranges, lse_tok, lse_dur, px_grad, py_grad, boundary = ctx.saved_tensors
        blank, arr, N, C, sigma, delay_penalty, code = ctx.meta
        scale, stride, mul = _upstream_scale(g_loss, code, x.shape[0])
        g = _tdt_builder_bwd(x, symbols, ranges, boundary, blank, arr, N, C, sigma, delay_penalty, lse_tok, lse_dur, px_grad,
                             py_grad, scale, stride, mul, ctx.band)
        return g, None, None, None, None, None, None, None, None


def get_rnnt_logprobs_tdt_pruned(
    logits: torch.Tensor,
    symbols: torch.Tensor,
    ranges: torch.Tensor,
    termination_symbol: int,
    durations,
    boundary: torch.Tensor,
    sigma: float = 0.0,
    delay_penalty: float = 0.0,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """TDT form of ``get_rnnt_logprobs_pruned`` (token-and-duration transducer; Xu et al., "Efficient Sequence
    Transduction by Jointly Predicting Tokens and Durations", ICML 2023; MI355X addition, regular type only).
    ``durations`` = (e_0 < ... < e_{N-1}): N = 1..5 ints in 0..16, at least one positive.

    logits [B,T,s_range,C+N]: the first C columns of a row are token logits (``termination_symbol`` among them), the last
    N duration logits, and the two heads are normalised independently: ``tok = log_softmax(row[:C]) - sigma`` (sigma >= 0,
    token head only), ``dur = log_softmax(row[C:])``.  Returns

    * ``px`` [B,N,S,T+1]: ``px[b,i,s,t] = tok[symbols[b,s]] + dur[i]``, the move (s,t) -> (s+1, t+e_i); -inf where
      ``t + e_i > t_end``, at column t_end and outside the band; ``delay_penalty`` is added as in ``rnnt_loss_pruned``,
      by source frame t;
    * ``py`` [B,Ny,S+1,T]: ``py[b,j,s,t] = tok[termination_symbol] + dur[index of d_j]``, the move (s,t) -> (s, t+d_j),
      d_j running over the positive durations (Ny = N or N - 1); -inf where ``t + d_j > t_end`` and outside the band.

    Feed them to ``mutual_information_recursion_tdt(px, py, durations, positive durations, boundary)``.  Differentiable
    w.r.t. ``logits``."""
    symbols, ranges, boundary = _pruned_inputs(logits, symbols, ranges, boundary)
    return _TdtLogprobs.apply(logits, symbols, ranges, termination_symbol, tuple(durations), boundary, _check_sigma(sigma),
                              _penalty(delay_penalty))


def get_rnnt_logprobs_tdt_joint(
    logits: torch.Tensor,
    symbols: torch.Tensor,
    termination_symbol: int,
    durations,
    boundary: Optional[torch.Tensor] = None,
    sigma: float = 0.0,
    delay_penalty: float = 0.0,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """``get_rnnt_logprobs_tdt_pruned`` for unpruned joiner logits [B,T,S+1,C+N], through identity ranges."""
    ranges = _joint_inputs(logits, symbols)
    return get_rnnt_logprobs_tdt_pruned(logits=logits, symbols=symbols, ranges=ranges, termination_symbol=termination_symbol,
                                        durations=durations, boundary=boundary, sigma=sigma, delay_penalty=delay_penalty)


def rnnt_loss_tdt_pruned(
    logits: torch.Tensor,
    symbols: torch.Tensor,
    ranges: torch.Tensor,
    termination_symbol: int,
    durations,
    boundary: torch.Tensor = None,
    sigma: float = 0.0,
    rnnt_type: str = "regular",
    delay_penalty: float = 0.0,
    reduction: Optional[str] = "mean",
) -> torch.Tensor:
    """TDT loss on pruned joiner logits [B,T,s_range,C+N] (MI355X addition): the lattices of
    ``get_rnnt_logprobs_tdt_pruned`` through ``mutual_information_recursion_tdt``, negated and reduced.  Only
    ``rnnt_type="regular"`` exists; anything else raises ValueError, as does a bad ``durations`` or a negative ``sigma``.
    When ``ranges`` are a band with ``s_range <= 15`` (the rule of ``rnnt_loss_pruned``, ``FTR_PRUNED_ROUTE=lattice``
    overrides it) the same loss is computed on the band itself and no full-size lattice is allocated.

    Prune ranges come from the ordinary ``rnnt_loss_simple``.  They guarantee a path through the band only when
    ``durations`` contains 0 and 1 (the moves of the lattice they were computed on): with other sets a path may have to
    leave the band, and an utterance without one gets a loss of +inf and zero gradients.  NeMo's ``omega``, the mix with
    the ordinary loss on the token columns, is ``rnnt_loss_tdt_mixed_pruned``."""
    if rnnt_type != "regular":
        raise ValueError(f"the TDT loss is defined for rnnt_type 'regular' only, given {rnnt_type}")
    code = _reduction_code(reduction)
    symbols_i, ranges_i, boundary_i = _pruned_inputs(logits, symbols, ranges, boundary)
    _tdt_args(durations, termination_symbol, logits.shape[3])
    return _TdtLoss.apply(logits, symbols_i, ranges_i, termination_symbol, tuple(durations), boundary_i, _check_sigma(sigma),
                          _penalty(delay_penalty), code)


def rnnt_loss_tdt(
    logits: torch.Tensor,
    symbols: torch.Tensor,
    termination_symbol: int,
    durations,
    boundary: Optional[torch.Tensor] = None,
    sigma: float = 0.0,
    rnnt_type: str = "regular",
    delay_penalty: float = 0.0,
    reduction: Optional[str] = "mean",
) -> torch.Tensor:
    """``rnnt_loss_tdt_pruned`` for unpruned joiner logits [B,T,S+1,C+N], through identity ranges."""
    if rnnt_type != "regular":
        raise ValueError(f"the TDT loss is defined for rnnt_type 'regular' only, given {rnnt_type}")
    ranges = _joint_inputs(logits, symbols)
    return rnnt_loss_tdt_pruned(logits=logits, symbols=symbols, ranges=ranges, termination_symbol=termination_symbol,
                                durations=durations, boundary=boundary, sigma=sigma, delay_penalty=delay_penalty,
                                reduction=reduction)


# ---- the TDT loss mixed with the ordinary loss on the token head (NeMo's omega; include/ftr_tdt_mix.h)

def _check_omega(omega) -> float:
    omega = float(omega)
    if not 0.0 <= omega <= 1.0:        # NaN fails both comparisons
        raise ValueError(f"omega must be in [0, 1], given {omega}")
    return omega


def _tdt_mix_builder_fwd(x, symbols, ranges, boundary, blank, arr, durs, blank_durs, C, sigma, parts, delay_penalty, band):
    """The two log-sum-exps and one gather launch for both losses.  ``band``: band-shaped planes (px / py [B,N|Ny,T,r],
    px0 / py0 [B,T,r]), else the lattices.  Only the planes of ``parts`` exist; the others are None."""
    B, T, r, _ = x.shape
    S = symbols.shape[1]
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)
    lse_tok, lse_dur = new(B, T, r), new(B, T, r)
    px = py = px0 = py0 = None
    if parts & _lib.FTR_TDT_MIX_TDT:
        px = new(B, len(durs), T, r) if band else new(B, len(durs), S, T + 1)
        py = new(B, len(blank_durs), T, r) if band else new(B, len(blank_durs), S + 1, T)
    if parts & _lib.FTR_TDT_MIX_RNNT:
        px0 = new(B, T, r) if band else new(B, S, T + 1)
        py0 = new(B, T, r) if band else new(B, S + 1, T)
    with torch.cuda.device(x.device):
        _lib.call("ftr_tdt_mix_pruned_band_fwd_f32" if band else "ftr_tdt_mix_pruned_logprobs_fwd_f32", _ptr(x), _ptr(symbols),
                  _ptr(ranges), _ptr(boundary), blank, arr, len(durs), float(sigma), int(parts), float(delay_penalty),
                  _ptr(lse_tok), _ptr(lse_dur), _ptr(px), _ptr(py), _ptr(px0), _ptr(py0), B, T, S, C, r, _stream_ptr(x))
    return lse_tok, lse_dur, px, py, px0, py0


class _TdtMixedLoss(torch.autograd.Function):
    """rnnt_loss_tdt_mixed_pruned for 0 < omega <= 1, the whole chain native and on one stream: one pass over the logits
    builds the operands of both losses (the ordinary one shares lse_tok), the TDT recursion and the ordinary recursion run
    back to back (band route: ftr_mutual_information_band_tdt_f32 and ftr_mutual_information_band_ws_f32; lattice route:
    the full-size twins), ``ans = (1 - omega) ans_tdt + omega ans0`` is formed on the device, and backward() is one
    launch that turns both sets of occupancies into d loss / d logits.  omega == 1 builds and runs the ordinary part only.
    ``omega`` is a host float: which branch a call takes is decided on the host, so a captured step keeps its branch."""

    @staticmethod
    def forward(ctx, logits, symbols, ranges, termination_symbol, durations, omega, boundary, sigma, delay_penalty, code):
        x = logits.detach().contiguous()
        need = logits.requires_grad
        arr, durs, blank_durs, C = _tdt_args(durations, termination_symbol, x.shape[3])
        B, T, r, _ = x.shape
        S = symbols.shape[1]
        blank = int(termination_symbol)
        tdt = omega < 1.0
        parts = _lib.FTR_TDT_MIX_RNNT | (_lib.FTR_TDT_MIX_TDT if tdt else 0)
        ctx.band = (_tdt_band_path_ok(ranges, boundary, T, S, r, len(durs), len(blank_durs))
                    and _band_path_ok(ranges, boundary, T, S, r))
        lse_tok, lse_dur, px, py, px0, py0 = _tdt_mix_builder_fwd(x, symbols, ranges, boundary, blank, arr, durs, blank_durs, C,
                                                                  sigma, parts, delay_penalty, ctx.band)
        ans_tdt = gx = gy = None
        if ctx.band:
            if tdt:
                ans_tdt, gx, gy = band_tdt_forward_backward(px, py, ranges, S, durs, blank_durs, boundary, need)
            ans0, gx0, gy0 = band_forward_backward(px0, py0, ranges, S, boundary, 0)
        else:
            if tdt:
                ans_tdt, gx, gy = tdt_forward_backward(px, py, durs, blank_durs, boundary, need)
            ans0, gx0, gy0 = mi_forward_backward(px0, py0, boundary, need, ans_grad_is_one=True)
        del px, py, px0, py0
        # both factors are finite and, where the TDT part exists, positive: -inf (no TDT path) stays -inf, no 0 * inf
        ans = torch.add(ans_tdt * (1.0 - omega), ans0, alpha=omega) if tdt else ans0
        if need:
            ctx.save_for_backward(x, symbols, ranges, lse_tok, lse_dur, gx, gy, gx0, gy0, boundary)
        ctx.meta = (blank, arr, len(durs), C, sigma, delay_penalty, int(code), omega)
        return _negated_reduce_native(ans, code)

    @staticmethod
    def backward(ctx, g_loss):
        x, symbols, ranges, lse_tok, lse_dur, gx, gy, gx0, gy0, boundary = ctx.saved_tensors
        blank, arr, N, C, sigma, delay_penalty, code, omega = ctx.meta
        scale, stride, mul = _upstream_scale(g_loss, code, x.shape[0])
        B, T, r, _ = x.shape
        S = symbols.shape[1]
        g = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.call("ftr_tdt_mix_pruned_band_bwd_scaled_f32" if ctx.band else "ftr_tdt_mix_pruned_logprobs_bwd_scaled_f32",
                      _ptr(x), _ptr(symbols), _ptr(ranges), _ptr(boundary), blank, arr, N, float(sigma), float(delay_penalty),
                      _ptr(lse_tok), _ptr(lse_dur), _ptr(gx), _ptr(gy), _ptr(gx0), _ptr(gy0), _ptr(scale), stride,
                      (1.0 - omega) * mul, omega * mul, _ptr(g), B, T, S, C, r, _stream_ptr(x))
        return g, None, None, None, None, None, None, None, None, None


def rnnt_loss_tdt_mixed_pruned(
    logits: torch.Tensor,
    symbols: torch.Tensor,
    ranges: torch.Tensor,
    termination_symbol: int,
    durations,
    omega: float,
    boundary: torch.Tensor = None,
    sigma: float = 0.0,
    delay_penalty: float = 0.0,
    reduction: Optional[str] = "mean",
) -> torch.Tensor:
    """The TDT loss mixed with the ordinary transducer loss on the token head of the same joiner rows (NeMo's ``omega``;
    MI355X addition, regular type only).  logits [B,T,s_range,C+N] float32 as for ``rnnt_loss_tdt_pruned``; per utterance

        L[b] = (1 - omega) * L_tdt[b] + omega * L_rnnt[b],        0 <= omega <= 1 (else ValueError)

    ``L_tdt`` is ``rnnt_loss_tdt_pruned(..., reduction="none")`` with the same ``durations``, ``sigma`` and ``delay_penalty``;
    ``L_rnnt`` is ``rnnt_loss_pruned(logits[..., :C], symbols, ranges, termination_symbol, boundary, "regular",
    delay_penalty, reduction="none")``: its operands are ``tok[sym]`` and ``tok[blank]`` with ``tok = log_softmax(row[:C])``,
    without ``sigma``.  This is the deterministic mix, the expectation of a per-step sampled choice between the two losses;
    it is not claimed to be bit-compatible with NeMo.  A caller that samples passes omega = 0 or 1 per step.

    Both losses come out of one pass: the ordinary loss's normaliser is the token log-sum-exp the TDT builder computes
    anyway, its operands are written by the same gather, and one gradient launch serves both, so no copy of the token
    columns and no second [B,T,s_range,C] gradient exist.  ``omega == 0`` is ``rnnt_loss_tdt_pruned`` itself,
    bit for bit.  ``omega == 1`` builds and runs the ordinary part only; the duration columns get exact zeros.  An utterance
    without a TDT path inside the band has ``L_tdt = +inf``: with ``omega < 1`` its loss is +inf and its gradient is that
    of the ordinary part alone.  The band route is taken when the ranges are a band that both band recursions cover
    (``FTR_PRUNED_ROUTE=lattice`` overrides it); otherwise both parts run on full-size lattices."""
    omega = _check_omega(omega)
    if omega == 0.0:
        return rnnt_loss_tdt_pruned(logits, symbols, ranges, termination_symbol, durations, boundary=boundary, sigma=sigma,
                                    delay_penalty=delay_penalty, reduction=reduction)
    code = _reduction_code(reduction)
    symbols_i, ranges_i, boundary_i = _pruned_inputs(logits, symbols, ranges, boundary)
    _tdt_args(durations, termination_symbol, logits.shape[3])
    return _TdtMixedLoss.apply(logits, symbols_i, ranges_i, termination_symbol, tuple(durations), omega, boundary_i,
                               _check_sigma(sigma), _penalty(delay_penalty), code)


def rnnt_loss_tdt_mixed(
    logits: torch.Tensor,
    symbols: torch.Tensor,
    termination_symbol: int,
    durations,
    omega: float,
    boundary: Optional[torch.Tensor] = None,
    sigma: float = 0.0,
    delay_penalty: float = 0.0,
    reduction: Optional[str] = "mean",
) -> torch.Tensor:
    """``rnnt_loss_tdt_mixed_pruned`` for unpruned joiner logits [B,T,S+1,C+N], through identity ranges."""
    omega = _check_omega(omega)
    ranges = _joint_inputs(logits, symbols)
    return rnnt_loss_tdt_mixed_pruned(logits=logits, symbols=symbols, ranges=ranges, termination_symbol=termination_symbol,
                                      durations=durations, omega=omega, boundary=boundary, sigma=sigma,
                                      delay_penalty=delay_penalty, reduction=reduction)


# ---- best-path alignment over the TDT and multi-blank lattices (MI355X addition, no reference counterpart)

def rnnt_alignment_tdt_pruned(
    logits: torch.Tensor,
    symbols: torch.Tensor,
    ranges: torch.Tensor,
    termination_symbol: int,
    durations,
    boundary: Optional[torch.Tensor] = None,
    sigma: float = 0.0,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Best-path alignment of a TDT model's pruned joiner output [B,T,s_range,C+N]: the lattice of
    ``get_rnnt_logprobs_tdt_pruned`` (no delay penalty) fed to ``mutual_information_viterbi_tdt``.  Returns
    ``(score [B] float32, frames [B,S], durations [B,S], blank_steps [B,T] int32)``, detached; see
    ``mutual_information_viterbi_tdt`` for their meaning: ``frames[b,s]`` is the frame that emits ``symbols[b,s]`` and
    ``durations[b,s]`` the duration it was emitted with.  As for the loss, ranges of the ordinary simple loss guarantee
    a path inside the band only when ``durations`` contains 0 and 1; an utterance without one gets score -inf and -1
    everywhere.  Every step runs on the device with no host read, so the call can be captured into a graph.  For
    unpruned joiner logits use
    ``mutual_information_viterbi_tdt(*get_rnnt_logprobs_tdt_joint(...), durations, positive durations, boundary)``.

    When ``ranges`` are a band with ``s_range <= 15`` (the rule of ``rnnt_loss_tdt_pruned``, ``FTR_PRUNED_ROUTE=lattice``
    included) and the moves number at most nine, no lattice is built: the band builder of the loss feeds
    ``mutual_information_viterbi_tdt_band``, which returns the same bits in memory and time of order T * s_range."""
    with torch.no_grad():
        symbols, ranges, boundary = _pruned_inputs(logits, symbols, ranges, boundary)
        arr, durs, blank_durs, C = _tdt_args(durations, termination_symbol, logits.shape[3])
        x = logits.detach().contiguous()
        B, T, r, _ = x.shape
        S = symbols.shape[1]
        if _align_band_path_ok(ranges, boundary, T, S, r, len(durs), len(blank_durs)):
            _, _, pxb, pyb = _tdt_band_builder_fwd(x, symbols, ranges, boundary, int(termination_symbol), arr, durs, blank_durs, C,
                                                   _check_sigma(sigma), 0.0)
            return mutual_information_viterbi_tdt_band(pxb, pyb, ranges, durs, blank_durs, boundary, S=S)
        _, _, px, py = _tdt_builder_fwd(x, symbols, ranges, boundary, int(termination_symbol), arr, durs, blank_durs, C,
                                        _check_sigma(sigma), 0.0)
        return mutual_information_viterbi_tdt(px, py, durs, blank_durs, boundary)


def rnnt_alignment_multiblank_pruned(
    logits: torch.Tensor,
    symbols: torch.Tensor,
    ranges: torch.Tensor,
    termination_symbol: int,
    big_blanks,
    boundary: Optional[torch.Tensor] = None,
    sigma: float = 0.0,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Best-path alignment of a multi-blank model's pruned joiner output [B,T,s_range,C]: the lattice of
    ``get_rnnt_logprobs_multiblank_pruned`` fed to ``mutual_information_viterbi_tdt`` with token durations ``(0,)`` and
    blank durations ``(1, d_1, ...)``.  Returns ``(score, frames, durations, blank_steps)`` as
    ``rnnt_alignment_tdt_pruned`` does; ``durations`` is 0 on every valid row (a symbol stays on its frame) and
    ``blank_steps[b,t]`` tells which blank, the standard one (1) or a big one (its duration), left frame t.  No host
    read; capturable.  Band ranges with ``s_range <= 15`` take the band route of ``rnnt_alignment_tdt_pruned`` (the band
    builder of ``rnnt_loss_multiblank_pruned``, then ``mutual_information_viterbi_tdt_band``): the same bits, no lattice."""
    with torch.no_grad():
        symbols, ranges, boundary = _pruned_inputs(logits, symbols, ranges, boundary)
        x = logits.detach().contiguous()
        ids, durs, dt = _big_blank_args(tuple(map(tuple, big_blanks)), termination_symbol, x.shape[3])
        B, T, r, _ = x.shape
        S = symbols.shape[1]
        if _align_band_path_ok(ranges, boundary, T, S, r, 1, len(dt)):
            _, pxb, pyb = _mb_band_builder_fwd(x, symbols, ranges, boundary, int(termination_symbol), ids, durs, len(dt),
                                               _check_sigma(sigma), 0.0)
            return mutual_information_viterbi_tdt_band(pxb.unsqueeze(1), pyb, ranges, (0,), dt, boundary, S=S)
        _, px, py = _mb_builder_fwd(x, symbols, ranges, boundary, int(termination_symbol), ids, durs, len(dt),
                                    _check_sigma(sigma), 0.0)
        return mutual_information_viterbi_tdt(px.unsqueeze(1), py, (0,), dt, boundary)


def _colsum_weighted(x: torch.Tensor, w: torch.Tensor, rows: int, C: int, st) -> torch.Tensor:
    """out[c] = sum_row w[row] * x[row, c] on the native two-stage kernel (deterministic)."""
    n = _lib.lib().ftr_colsum_weighted_workspace_floats(rows, C)
    ws = torch.empty((max(n, 1),), dtype=torch.float32, device=x.device)
    out = torch.empty((C,), dtype=torch.float32, device=x.device)
    _lib.call("ftr_colsum_weighted_f32", _ptr(x), _ptr(w), _ptr(out), _ptr(ws), n, rows, C, st)
    return out


def _smoothed_forward(lm, am, symbols, termination_symbol, boundary, modified, lm_only_scale, am_only_scale,
                      process_group, delay_penalty):
    """Forward of the smoothed builder on the native kernels (rnnt_loss.py:1265-1365; with the penalty block :1461-1478
    folded into the lattice writer when delay_penalty > 0).  Returns px, py and what the backward needs."""
    B, T, C = am.shape
    S = lm.shape[1] - 1
    T1 = T if modified else T + 1
    cs = 1.0 - lm_only_scale - am_only_scale                    # :1342
    ls = lm_only_scale if lm_only_scale != 0.0 else 1.0e-20       # :1346-1349
    a_s = am_only_scale if am_only_scale != 0.0 else 1.0e-20
    amc = am.detach().contiguous(); lmc = lm.detach().contiguous()
    dev = amc.device
    am_probs = torch.empty_like(amc); lm_probs = torch.empty_like(lmc)
    am_max = torch.empty((B, T), dtype=torch.float32, device=dev)
    lm_max = torch.empty((B, S + 1), dtype=torch.float32, device=dev)
    lm_sum = torch.empty((B, S + 1), dtype=torch.float32, device=dev)
    px = torch.empty((B, S, T1), dtype=torch.float32, device=dev)
    py = torch.empty((B, S + 1, T), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        st = _stream_ptr(amc)
        _lib.call("ftr_rowmax_exp_sum_f32", _ptr(lmc), _ptr(lm_probs), _ptr(lm_max), _ptr(lm_sum),
                  B * (S + 1), C, st)                                                                   # :1276-1278
        inv = (1.0 / lm_sum).contiguous()                                                               # [B,S+1]
        ratio_sum = _colsum_weighted(lm_probs, inv, B * (S + 1), C, st)                                 # [C]
        count = float(B * (S + 1))
        if process_group is not None:
            # the mean runs over the rows of EVERY shard (rnnt_loss.py:1279-1280 on the global batch), and shards may hold
            # different numbers of rows (uneven batch split, every rank padded to its own S): the local row count travels
            # in the same all-reduce as the [C] sums and the reduced count -- a device scalar, no host read -- divides them
            packed = torch.cat((ratio_sum, torch.full((1,), count, dtype=torch.float32, device=dev)))
            torch.distributed.all_reduce(packed, group=process_group)
            ratio_sum, count = packed[:C], packed[C]
        u = (ratio_sum / count + _TINY).contiguous()                                                    # :1279-1280
        # am_probs, am_max and am_probs . u in one pass over am (:1265-1268, :1281-1286)
        am_dot = torch.empty((B * T,), dtype=torch.float32, device=dev)
        _lib.call("ftr_rowmax_exp_dot_f32", _ptr(amc), _ptr(am_probs), _ptr(am_max), _ptr(u), _ptr(am_dot), B * T, C, st)
        fused = _use_fused_builder(C)
        prod = torch.empty((B, S + 1, T), dtype=torch.float32, device=dev) if fused else \
            _gemm(0, lm_probs, am_probs, B, T, S, C, st)                                                # :1270-1272
        amonly = (am_dot.log().reshape(B, T) + am_max).contiguous()                                     # :1281-1286
        ulog = u.log().contiguous()                                                                     # :1287
        lmonly = (lm_sum.log() + lm_max).contiguous()                                                   # :1288-1290
        if fused:
            _lib.call("ftr_smoothed_logprobs_fused_fwd_f32", _ptr(amc), _ptr(lmc), _ptr(symbols), _ptr(am_probs),
                      _ptr(lm_probs), _ptr(am_max), _ptr(lm_max), _ptr(lmonly), _ptr(amonly), _ptr(ulog), _ptr(boundary),
                      int(termination_symbol), float(delay_penalty), cs, ls, a_s, _ptr(px), _ptr(py), _ptr(prod),
                      B, T, S, C, int(modified), st)
        else:
            _lib.call("ftr_smoothed_logprobs_fwd_pen_f32", _ptr(amc), _ptr(lmc), _ptr(symbols), _ptr(prod), _ptr(am_max),
                      _ptr(lm_max), _ptr(lmonly), _ptr(amonly), _ptr(ulog), _ptr(boundary), int(termination_symbol),
                      float(delay_penalty), cs, ls, a_s, _ptr(px), _ptr(py), B, T, S, C, int(modified), st)
    saved = (am_probs, lm_probs, prod, symbols, boundary, inv, u, am_dot)
    meta = (int(termination_symbol), int(modified), cs, ls, a_s, count, process_group)
    return px, py, saved, meta


def _smoothed_backward(saved, meta, gpx, gpy, scale=None, stride=0, mul=1.0):
    """Hand-written backward of the smoothed builder; gpx / gpy are d/d px, d/d py, multiplied on the fly by
    (scale ? scale[b * stride] : 1) * mul (the upstream gradient of the loss that owns the occupancies)."""
    am_probs, lm_probs, prod, symbols, boundary, inv, u, am_dot = saved
    blank, modified, cs, ls, a_s, count, group = meta
    B, T, C = am_probs.shape
    S = lm_probs.shape[1] - 1
    dev = am_probs.device
    gpx = gpx.contiguous(); gpy = gpy.contiguous()
    W = torch.empty_like(prod)
    rsx = torch.empty((B, S + 1), dtype=torch.float32, device=dev)
    rsy = torch.empty((B, S + 1), dtype=torch.float32, device=dev)
    R = torch.empty((B, T), dtype=torch.float32, device=dev)
    d_am = torch.empty_like(am_probs); d_lm = torch.empty_like(lm_probs)
    fused = _use_fused_builder_bwd(T, C, B)
    with torch.cuda.device(dev):
        st = _stream_ptr(am_probs)
        if fused:     # W and, per row, the frame interval outside which it and the occupancies are exact zeros
            live = _live_scratch(d_lm, B, S)
            _lib.call("ftr_smoothed_logprobs_bwd_w_live_f32", _ptr(gpx), _ptr(gpy), _ptr(scale), stride, mul, _ptr(prod),
                      _ptr(boundary), cs, _ptr(W), _ptr(rsx), _ptr(rsy), _ptr(live), B, T, S, modified, st)
        else:
            _lib.call("ftr_smoothed_logprobs_bwd_w_scaled_f32", _ptr(gpx), _ptr(gpy), _ptr(scale), stride, mul, _ptr(prod),
                      _ptr(boundary), cs, _ptr(W), _ptr(rsx), _ptr(rsy), B, T, S, modified, st)
        dlmp = _gemm(1, W, am_probs, B, T, S, C, st)         # [B,S+1,C]
        if fused:                                              # W^T lm_probs inside the d am kernel, over the live row chunks only
            _lib.call("ftr_smoothed_logprobs_fused_bwd_am_live_f32", _ptr(gpx), _ptr(gpy), _ptr(scale), stride, mul, _ptr(W),
                      _ptr(live), _ptr(lm_probs), _ptr(am_probs), _ptr(symbols), _ptr(boundary), blank, cs + a_s, _ptr(u),
                      _ptr(am_dot), a_s, _ptr(R), _ptr(d_am), B, T, S, C, modified, st)
        else:
            damp = _gemm(2, W, lm_probs, B, T, S, C, st)    # [B,T,C]
            _lib.call("ftr_smoothed_logprobs_bwd_am_scaled_f32", _ptr(gpx), _ptr(gpy), _ptr(scale), stride, mul, _ptr(damp),
                      _ptr(am_probs), _ptr(symbols), _ptr(boundary), blank, cs + a_s, _ptr(u), _ptr(am_dot), a_s, _ptr(R),
                      _ptr(d_am), B, T, S, C, modified, st)
        # d u: through amonly_norm and through ulog
        du = _colsum_weighted(am_probs, R, B * T, C, st)
        gul = torch.zeros((C,), dtype=torch.float32, device=dev)
        if S > 0:
            gul.index_add_(0, _i64(symbols).reshape(-1), rsx[:, :S].reshape(-1))
        gul[blank] += rsy.sum()
        du = du + a_s * gul / u
        if group is not None:
            torch.distributed.all_reduce(du, group=group)
        gu = (du / count).contiguous()
        dotq = torch.empty((B, S + 1), dtype=torch.float32, device=dev)
        _lib.call("ftr_rowdot_f32", _ptr(lm_probs), _ptr(gu), _ptr(dotq), B * (S + 1), C, st)
        dotq = dotq * inv
        arow = ((-ls) * (rsx + rsy) - dotq) * inv
        arow = arow.contiguous()
        _lib.call("ftr_smoothed_logprobs_bwd_lm_f32", _ptr(dlmp), _ptr(lm_probs), _ptr(symbols), _ptr(rsx),
                  _ptr(rsy), blank, cs + ls, _ptr(arow), _ptr(inv), _ptr(gu), _ptr(d_lm), B, S, C, st)
    return d_lm, d_am


class _SmoothedLogprobs(torch.autograd.Function):
    """get_rnnt_logprobs_smoothed (+ fix_for_boundary) for regular/modified on the native builder kernels.

    Forward (rnnt_loss.py:1265-1365): out = cs (x - normalizers) + ls (lm - lmonly_norm) + as (am + ulog - amonly_norm)
    with lmonly_norm = log(rowsum lm_probs) + lm_max, u = mean_{b,s}(lm_probs / rowsum) + tiny, ulog = log u,
    amonly_norm = log(am_probs . u) + am_max.  The lattice-sized work is in ftr_smoothed_logprobs_*; the batch
    statistics ([C], [B,S+1] and [B,T] vectors, two matvecs) are torch ops on the same stream.

    Backward, with gx = gpx masked where the forward wrote -inf, gy = gpy, rsx/rsy their sums over t and
    colsum over s:
      normalizers : W = -cs (gx+gy)/(prod+tiny), two GEMMs (as in _SimpleLogprobs)
      direct      : am column sym/blank gets (cs+as) g, lm column sym/blank gets (cs+ls) g
      lmonly_norm : d lm += -ls (rsx+rsy) * lm_probs / rowsum
      amonly_norm : R[b,t] = -as colsum(gx+gy) / (am_probs . u);  d am += R am_probs u;  d u += R^T am_probs
      ulog        : d u += as (sum of rsx by symbol + sum rsy at blank) / u
      u           : gu = d u / N;  d lm += lm_probs/rowsum * (gu - (lm_probs/rowsum) . gu)
    """

    @staticmethod
    def forward(ctx, lm, am, symbols, termination_symbol, boundary, modified, lm_only_scale, am_only_scale,
                process_group):
        px, py, saved, meta = _smoothed_forward(lm, am, symbols, termination_symbol, boundary, modified, lm_only_scale,
                                                am_only_scale, process_group, 0.0)
        ctx.save_for_backward(*saved)
        ctx.meta = meta
        return px, py

    @staticmethod
    def backward(ctx, gpx, gpy):
        d_lm, d_am = _smoothed_backward(ctx.saved_tensors, ctx.meta, gpx, gpy)
        return d_lm, d_am, None, None, None, None, None, None, None


class _SmoothedLoss(torch.autograd.Function):
    """rnnt_loss_smoothed for regular/modified as ONE graph node, like _SimpleLoss: smoothed builder (penalty folded
    in) + GEMM, recursion forward + backward (occupancies), native loss reduction; backward() feeds the occupancies to
    the builder's backward kernels with the upstream gradient folded in on the fly."""

    @staticmethod
    def forward(ctx, lm, am, symbols, termination_symbol, boundary, modified, lm_only_scale, am_only_scale,
                process_group, delay_penalty, code, want_occupancies):
        px, py, saved, meta = _smoothed_forward(lm, am, symbols, termination_symbol, boundary, modified, lm_only_scale,
                                                am_only_scale, process_group, delay_penalty)
        need = bool(want_occupancies) or ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        if need:      # the loss tail rides along with the recursion's backward launch
            ans, px_grad, py_grad, loss = mi_forward_backward(px, py, boundary, True, ans_grad_is_one=True, loss_code=code)
        else:
            ans, px_grad, py_grad = mi_forward_backward(px, py, boundary, False, ans_grad_is_one=True)
            loss = _negated_reduce_native(ans, code)
        if need:
            ctx.save_for_backward(*saved, px_grad, py_grad)
        else:
            px_grad = torch.zeros_like(px); py_grad = torch.zeros_like(py)
        del px, py
        ctx.meta = meta
        ctx.code = int(code)
        ctx.mark_non_differentiable(px_grad, py_grad)
        ctx.set_materialize_grads(False)          # no zero tensors for the two occupancy outputs in backward
        return loss, px_grad, py_grad

    @staticmethod
    def backward(ctx, g_loss, _g1, _g2):
        if g_loss is None:
            return (None,) * 12
        *saved, px_grad, py_grad = ctx.saved_tensors
        scale, stride, mul = _upstream_scale(g_loss, ctx.code, px_grad.shape[0])
        d_lm, d_am = _smoothed_backward(saved, ctx.meta, px_grad, py_grad, scale, stride, mul)
        return d_lm, d_am, None, None, None, None, None, None, None, None, None, None


def get_rnnt_logprobs_smoothed(
    lm: torch.Tensor,
    am: torch.Tensor,
    symbols: torch.Tensor,
    termination_symbol: int,
    lm_only_scale: float = 0.1,
    am_only_scale: float = 0.1,
    boundary: Optional[torch.Tensor] = None,
    rnnt_type: str = "regular",
    process_group=None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """rnnt_loss.py:1132-1367, native (HIP) builder, differentiable w.r.t. lm and am.  ``process_group``
    (extension, default None = local batch only): when the batch is sharded over ranks, the batch-wide
    ``unigram_lm`` mean (rnnt_loss.py:1279-1280) is all-reduced (one [C] vector over RCCL forward, one backward)
    so every shard sees the global-batch value."""
    _check_type(rnnt_type)
    symbols = _check_simple_inputs(lm, am, symbols, termination_symbol)
    boundary = _as_boundary(boundary, am.shape[0], am.device)
    px, py = _SmoothedLogprobs.apply(lm, am, symbols, termination_symbol, boundary, rnnt_type != "regular",
                                     float(lm_only_scale), float(am_only_scale), process_group)
    if rnnt_type == "constrained":
        px = px + py[:, 1:, :]                                                                              # :1362-1363
    return px, py


def rnnt_loss_smoothed(
    lm: torch.Tensor,
    am: torch.Tensor,
    symbols: torch.Tensor,
    termination_symbol: int,
    lm_only_scale: float = 0.1,
    am_only_scale: float = 0.1,
    boundary: Optional[torch.Tensor] = None,
    rnnt_type: str = "regular",
    delay_penalty: float = 0.0,
    reduction: Optional[str] = "mean",
    calc_gradients: bool = False,
    process_group=None,
) -> Union[Tuple[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]], torch.Tensor]:
    """rnnt_loss.py:1369-1494.  regular / modified: one fused node (no framework-side pass over a lattice)."""
    _check_type(rnnt_type)
    code = _reduction_code(reduction)
    boundary = _as_boundary(boundary, am.shape[0], am.device)
    if rnnt_type == "constrained":   # the penalty applies after px += py[:, 1:, :]  (:1362-1363, :1461-1478)
        px, py = get_rnnt_logprobs_smoothed(lm=lm, am=am, symbols=symbols, termination_symbol=termination_symbol,
                                            lm_only_scale=lm_only_scale, am_only_scale=am_only_scale,
                                            boundary=boundary, rnnt_type=rnnt_type, process_group=process_group)
        px = _apply_delay_penalty(px, boundary, rnnt_type, delay_penalty)
        return _drive(px, py, boundary, reduction, calc_gradients)
    symbols_i = _check_simple_inputs(lm, am, symbols, termination_symbol)
    loss, px_grad, py_grad = _SmoothedLoss.apply(lm, am, symbols_i, termination_symbol, boundary, rnnt_type != "regular",
                                                 float(lm_only_scale), float(am_only_scale), process_group,
                                                 _penalty(delay_penalty), code, bool(calc_gradients))
    return (loss, (px_grad, py_grad)) if calc_gradients else loss
