"""Host wrappers of the native ops: ``mutual_information_recursion``, ``mutual_information_viterbi`` and ``cummin``.

Mirrors tf_fast_rnnt/python/tf_fast_rnnt/__init__.py:42-162 of the reference (op call + registered
gradient) and the op kernel it drives, ``FastRNNTOpBase::Compute``
(tf_fast_rnnt/python/csrc/tf_fast_rnnt_op.cc:48-117): allocate the ``p`` workspace and the outputs,
run the forward, and -- when gradients are wanted -- the backward seeded with ones on the same stream.
Differences from the reference, all deliberate (SURVEY.md section 7 "hard parts"):

* tensors are torch tensors on a HIP device; work is enqueued on torch's current stream and the
  host is never blocked (the reference calls cudaStreamSynchronize per op, tf_fast_rnnt_op.cc:113);
* ``boundary=None`` works (defaults to (0,0,S,T) in the kernels); the reference advertises it but
  dereferences the tensor unconditionally (mutual_information_cuda.cu:259-260);
* gradients are computed whenever autograd needs them, not only when ``calc_gradients`` is set (the
  reference back-propagates an uninitialised buffer in that case, tf_fast_rnnt_op.cc:83-98);
* for a modified-type ``px`` ([B,S,T]) ``px_grad`` has the shape of ``px`` (the reference always
  allocates [B,S,T+1], tf_fast_rnnt_op.cc:84, which cannot be multiplied into the gradient).
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import torch

from . import _lib


def _stream_ptr(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _require_gpu(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(
            f"tf_fast_rnnt: `{name}` is on {t.device}; the native ops run on a HIP GPU only "
            "(the reference registers DEVICE_GPU kernels only, tf_fast_rnnt_op.cc:131,164) and there is no CPU fallback")


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _as_boundary(boundary, B: int, device) -> Optional[torch.Tensor]:
    if boundary is None:
        return None
    boundary = torch.as_tensor(boundary, device=device)
    if boundary.dtype != torch.int32:
        boundary = boundary.to(torch.int32)
    if tuple(boundary.shape) != (B, 4):
        raise ValueError(f"boundary must have shape ({B}, 4), got {tuple(boundary.shape)}")
    return boundary.contiguous()


class _Workspace:
    """ONE cached forward->backward workspace per (device, stream), sized by CAPACITY, not by shape: a training loop pads
    every batch to its own maximum, so (B, S, T) change from step to step and a cache keyed on the exact shape would
    allocate and initialise a workspace per step.  The native layout anchors the hand-off region of a launch at the END of
    the buffer it is given and grows everything else from the front (include/ftr.h, FTR_MI_WS_CLEAN), so one buffer of
    (largest data part seen) + (largest hand-off part seen) floats serves every shape seen so far; its tail is zeroed when
    the buffer is (re)allocated -- on growth only -- and every launch leaves its hand-off region zero again, so every
    launch gets FTR_MI_WS_CLEAN and no memset node.  Safe because every user of the workspace in this package runs the
    forward and the backward launch back to back on one stream (the occupancies, not the workspace, are what autograd
    keeps).  Under stream capture the cache is bypassed (a graph owns its allocations).

    If a launch ever times out waiting for a producer (ftr_mutual_information_status bit 0: cannot happen unless a
    workgroup never ran) its `ans` is NaN and the hand-off region is left dirty: call ``clear_workspace_cache()`` (or
    ``check_workspace_status()``, which synchronises, reads the status word and drops the dirty buffers)."""
    _cache = {}
    inits = 0      # (re)allocations so far: the tests assert that a ragged loop does not allocate per step

    def __init__(self):
        self.ws = None; self.cap = 0; self.data_max = 0; self.handoff_max = 0; self.last = None

    @classmethod
    def get(cls, L, device, B, S, T):
        st = torch.cuda.current_stream(device)
        total = L.ftr_mutual_information_workspace_floats(B, S, T)
        if torch.cuda.is_current_stream_capturing():
            return torch.empty(total, dtype=torch.float32, device=device), total, 0
        key = (device.index, st.cuda_stream)
        w = cls._cache.get(key)
        if w is None:
            if len(cls._cache) >= 4:           # a handful of (device, stream) pairs; do not hoard HBM beyond that
                cls._cache.pop(next(iter(cls._cache)))
            w = cls._cache[key] = _Workspace()
        handoff = L.ftr_mutual_information_handoff_floats(B, S, T)
        data = total - handoff
        if w.ws is None or data > w.data_max or handoff > w.handoff_max:
            # grow with some headroom so that a slowly rising maximum does not reallocate every few steps
            w.data_max = max(w.data_max, data + data // 8 if w.ws is not None else data)
            w.handoff_max = max(w.handoff_max, handoff + handoff // 8 if w.ws is not None else handoff)
            w.cap = w.data_max + w.handoff_max + 8
            w.ws = None                        # release before allocating the larger one
            w.ws = torch.empty(w.cap, dtype=torch.float32, device=device)
            w.ws[w.cap - w.handoff_max - 8:].zero_()     # every shape's hand-off region lies inside this tail
            cls.inits += 1
        w.last = (B, S, T)
        return w.ws, w.cap, _lib.FTR_MI_WS_CLEAN


def clear_workspace_cache() -> None:
    """Drops the cached recursion workspaces (they are re-created on demand)."""
    _Workspace._cache.clear()


def check_workspace_status() -> int:
    """Synchronises and reads the sticky status word of every cached workspace (ftr_mutual_information_status): returns
    the OR of them and drops the workspaces that report a problem, so that the next launch starts from a clean one.
    0 = fine.  Diagnostic: a non-zero value means a launch gave up waiting for a producer and answered NaN."""
    import ctypes
    L = _lib.lib()
    bad = 0
    for key, w in list(_Workspace._cache.items()):
        if w.ws is None or w.last is None:
            continue
        B, S, T = w.last
        st = ctypes.c_int(-1)
        with torch.cuda.device(w.ws.device):
            _lib.call("ftr_mutual_information_status", w.ws.data_ptr(), w.cap, B, S, T, ctypes.byref(st), None, key[1])
        if st.value != 0:
            bad |= st.value
            del _Workspace._cache[key]
    return bad


def _lattice_inputs(px: torch.Tensor, py: torch.Tensor):
    """Validation of the ordinary lattice's entries.  Returns (px, py, B, S, T, modified) with px and py contiguous."""
    _require_gpu(px, "px"); _require_gpu(py, "py")
    if px.dtype != torch.float32 or py.dtype != torch.float32:
        raise TypeError("px and py must be float32 (op registration: tf_fast_rnnt_op.cc:27-34)")
    if px.dim() != 3 or py.dim() != 3:
        raise ValueError("px and py must be 3-dimensional")
    B, S, T1 = px.shape
    T = py.shape[2]
    if T1 not in (T, T + 1):
        raise ValueError(f"px.shape[-1]={T1} must be T or T+1 with T=py.shape[-1]={T}")
    if tuple(py.shape) != (B, S + 1, T):
        raise ValueError(f"py must have shape {(B, S + 1, T)}, got {tuple(py.shape)}")
    modified = int(T1 == T)
    return px.contiguous(), py.contiguous(), B, S, T, modified


def mi_forward_backward(px: torch.Tensor, py: torch.Tensor, boundary: Optional[torch.Tensor],
                        need_grads: bool, ans_grad: Optional[torch.Tensor] = None,
                        return_ans_grad_check: bool = False, ans_grad_is_one: bool = False, loss_code: Optional[int] = None):
    """FastRNNTOpBase::Compute on raw tensors (no autograd).  Returns (ans, px_grad|None, py_grad|None[, check]).
    ``loss_code`` (0 none / 1 mean / 2 sum, with ``ans_grad_is_one`` and ``need_grads``): the backward launch also writes the
    negated / reduced loss (ftr_mutual_information_bwd_loss_ws_f32) and it is returned as a fourth element."""
    px, py, B, S, T, modified = _lattice_inputs(px, py)
    boundary = _as_boundary(boundary, B, px.device)
    L = _lib.lib()
    with torch.cuda.device(px.device):
        st = _stream_ptr(px)
        ws, ws_floats, flags = _Workspace.get(L, px.device, B, S, T)
        ans = torch.empty((B,), dtype=torch.float32, device=px.device)
        _lib.call("ftr_mutual_information_fwd_ws_f32", _ptr(px), _ptr(py), _ptr(boundary), _ptr(ws), ws_floats, flags,
                                                       _ptr(ans), B, S, T, modified, st)
        if not need_grads:
            return (ans, None, None, None) if return_ans_grad_check else (ans, None, None)
        px_grad = torch.empty_like(px)
        py_grad = torch.empty_like(py)
        # ans_grad := 1 like the op (tf_fast_rnnt_op.cc:104-107); the kernel overwrites it with
        # p_grad[s_begin,t_begin] as the reference's self-check does (overwrite_ans_grad = true, :109-110)
        if ans_grad_is_one:
            ag, overwrite = None, 0          # NULL ans_grad = ones, no self-check write-back: one launch less
        else:
            ag = torch.ones((B,), dtype=torch.float32, device=px.device) if ans_grad is None else ans_grad.to(torch.float32).contiguous().clone()
            overwrite = 1
        if loss_code is not None and ans_grad_is_one and not return_ans_grad_check:
            loss = torch.empty((B,) if loss_code == 0 else (), dtype=torch.float32, device=px.device)
            _lib.call("ftr_mutual_information_bwd_loss_ws_f32", _ptr(px), _ptr(py), _ptr(boundary), _ptr(ws), ws_floats, flags,
                      _ptr(px_grad), _ptr(py_grad), _ptr(ans), int(loss_code), _ptr(loss), B, S, T, modified, st)
            return ans, px_grad, py_grad, loss
        # p_grad = NULL: the reference's [B,S+1,T+1] gradient lattice (tf_fast_rnnt_op.cc:90-91) never exists here
        _lib.call("ftr_mutual_information_bwd_ws_f32", _ptr(px), _ptr(py), _ptr(boundary), _ptr(ws), ws_floats, flags,
                                                       None, _ptr(px_grad), _ptr(py_grad), _ptr(ag), overwrite,
                                                       B, S, T, modified, st)
    return (ans, px_grad, py_grad, ag) if return_ans_grad_check else (ans, px_grad, py_grad)


class _Occupancies(torch.autograd.Function):
    """Op "FastRNNTLoss" + its registered gradient (__init__.py:154-162), for every lattice: ``raw(px, py, need)`` is the
    forward / backward pair on raw tensors, ``name`` the public function's."""

    @staticmethod
    def forward(ctx, px, py, calc_gradients, name, raw):
        need = bool(calc_gradients) or px.requires_grad or py.requires_grad
        ans, px_grad, py_grad = raw(px.detach(), py.detach(), need)
        if need:
            ctx.save_for_backward(px_grad, py_grad)
        ctx.have_grads = need
        ctx.name = name
        if px_grad is None:
            px_grad = torch.zeros_like(px)
            py_grad = torch.zeros_like(py)
        ctx.mark_non_differentiable(px_grad, py_grad)
        ctx.set_materialize_grads(False)          # no zero tensors for the two occupancy outputs in backward
        return ans, px_grad, py_grad

    @staticmethod
    def backward(ctx, g_ans, _g1, _g2):
        if not ctx.have_grads:
            raise RuntimeError(f"{ctx.name}: backward without saved occupancies")
        if g_ans is None:
            return None, None, None, None, None
        # _RNNTLossGrad: ans_grad * gradpx, ans_grad * gradpy, broadcast over each occupancy's own rank
        gx, gy = (g_ans.reshape((-1,) + (1,) * (o.dim() - 1)) * o for o in ctx.saved_tensors)
        return gx, gy, None, None, None


def mutual_information_recursion(
    px: torch.Tensor,
    py: torch.Tensor,
    boundary: Optional[torch.Tensor] = None,
    calc_gradients: bool = False,
) -> Union[Tuple[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]], torch.Tensor]:
    """Same contract as the reference's ``mutual_information_recursion`` (__init__.py:42-149).

    px: [B,S,T+1] (regular) or [B,S,T] (modified); py: [B,S+1,T]; boundary: int32 [B,4] rows
    (s_begin, t_begin, s_end, t_end) or None.  Returns ``ans`` [B] with
    ``p[b,s,t] = log_add(p[b,s-1,t(+off)] + px[b,s-1,t(+off)], p[b,s,t-1] + py[b,s,t-1])``,
    ``ans[b] = p[b,s_end,t_end]``; with ``calc_gradients`` also ``(px_grad, py_grad)``, the occupation
    probabilities (gradient of ``ans.sum()``).  Differentiable w.r.t. px and py.
    """
    ans, px_grad, py_grad = _Occupancies.apply(px, py, calc_gradients, "mutual_information_recursion",
                                               lambda x, y, need: mi_forward_backward(x, y, boundary, need))
    return (ans, (px_grad, py_grad)) if calc_gradients else ans


def _check_durations(durations) -> Tuple[int, ...]:
    durs = tuple(int(d) for d in durations)
    if not 1 <= len(durs) <= 8:
        raise ValueError(f"durations must hold 1..8 values, got {len(durs)}")
    if any(d < 1 or d > 32 for d in durs) or any(b <= a for a, b in zip(durs, durs[1:])):
        raise ValueError(f"durations must be strictly increasing values in 1..32, got {durs}")
    return durs


def mb_forward_backward(px: torch.Tensor, py: torch.Tensor, durations, boundary: Optional[torch.Tensor], need_grads: bool):
    """The multi-blank recursion on raw tensors (no autograd): forward and, when wanted, the backward seeded with ones,
    back to back on torch's current stream.  Returns (ans, px_grad|None, py_grad|None)."""
    import ctypes
    _require_gpu(px, "px"); _require_gpu(py, "py")
    if px.dtype != torch.float32 or py.dtype != torch.float32:
        raise TypeError("px and py must be float32")
    durs = _check_durations(durations)
    D = len(durs)
    if px.dim() != 3 or py.dim() != 4:
        raise ValueError("px must be [B,S,T+1] and py [B,D,S+1,T]")
    B, S, T1 = px.shape
    T = py.shape[3]
    if T1 != T + 1:
        raise ValueError(f"px.shape[-1]={T1} must be T+1 with T=py.shape[-1]={T} (regular type only)")
    if tuple(py.shape) != (B, D, S + 1, T):
        raise ValueError(f"py must have shape {(B, D, S + 1, T)}, got {tuple(py.shape)}")
    px = px.contiguous(); py = py.contiguous()
    boundary = _as_boundary(boundary, B, px.device)
    dur_arr = (ctypes.c_int32 * D)(*durs)       # read by the launch itself: no device copy, no host synchronisation
    L = _lib.lib()
    with torch.cuda.device(px.device):
        st = _stream_ptr(px)
        nws = L.ftr_mutual_information_multiblank_workspace_floats(B, S, T)
        ws = torch.empty((max(nws, 2) + 1) // 2, dtype=torch.float64, device=px.device)
        ans = torch.empty((B,), dtype=torch.float32, device=px.device)
        _lib.call("ftr_mutual_information_multiblank_fwd_f32", _ptr(px), _ptr(py), _ptr(boundary), dur_arr, D, _ptr(ws), nws,
                  _ptr(ans), B, S, T, st)
        if not need_grads:
            return ans, None, None
        px_grad = torch.empty_like(px)
        py_grad = torch.empty_like(py)
        _lib.call("ftr_mutual_information_multiblank_bwd_f32", _ptr(px), _ptr(py), _ptr(boundary), dur_arr, D, _ptr(ws), nws,
                  None, _ptr(px_grad), _ptr(py_grad), B, S, T, st)
    return ans, px_grad, py_grad


def mutual_information_recursion_multiblank(
    px: torch.Tensor,
    py: torch.Tensor,
    durations,
    boundary: Optional[torch.Tensor] = None,
    calc_gradients: bool = False,
) -> Union[Tuple[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]], torch.Tensor]:
    """``mutual_information_recursion`` over a lattice with big blanks (multi-blank transducer; MI355X addition, no
    reference counterpart; csrc/mi_multiblank.hip).  Regular type only.

    px: [B,S,T+1]; py: [B,D,S+1,T], ``py[b,j,s,t]`` being the log-probability of the move (s,t) -> (s,t+durations[j]);
    durations: D = 1..8 strictly increasing ints in 1..32 (they need not contain 1); boundary: int32 [B,4] or None.

        p[s,t] = logadd(p[s-1,t] + px[s-1,t], logadd_j p[s,t-d_j] + py[j,s,t-d_j]),   p[s_begin,t_begin] = 0

    Moves that would leave the boundary rectangle are ignored whatever value they carry.  Returns ``ans`` [B] =
    ``p[s_end,t_end]`` (-inf when no path exists; the gradients are then zero, never NaN); with ``calc_gradients`` also
    ``(px_grad, py_grad)``, the occupancies, in the shapes of px and py and zero outside the rectangle.  With
    ``durations=(1,)`` and ``py[:,None]`` this is the lattice of ``mutual_information_recursion``.  Differentiable
    w.r.t. px and py; asynchronous on torch's current stream, no host read (capturable)."""
    durations = tuple(durations)
    ans, px_grad, py_grad = _Occupancies.apply(px, py, calc_gradients, "mutual_information_recursion_multiblank",
                                               lambda x, y, need: mb_forward_backward(x, y, durations, boundary, need))
    return (ans, (px_grad, py_grad)) if calc_gradients else ans


def _check_tdt_moves(token_durations, blank_durations, blank_hi: int = 16,
                     max_moves: int = 10) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    """``max_moves``: 10 for the recursions, lattice (mi_rowlane.h, MAXM) and band; 9 for the alignment (MAXM_ALIGN)."""
    tok = tuple(int(d) for d in token_durations)
    blk = tuple(int(d) for d in blank_durations)
    for name, v, lo, hi in (("token_durations", tok, 0, 16), ("blank_durations", blk, 1, blank_hi)):
        if len(v) < 1:
            raise ValueError(f"{name} must hold at least one value")
        if any(d < lo or d > hi for d in v) or any(b <= a for a, b in zip(v, v[1:])):
            raise ValueError(f"{name} must be strictly increasing values in {lo}..{hi}, got {v}")
    if len(tok) + len(blk) > max_moves:
        raise ValueError(f"token_durations and blank_durations hold {len(tok) + len(blk)} moves together, at most {max_moves} are supported")
    return tok, blk


def _duration_lattice_inputs(px: torch.Tensor, py: torch.Tensor, token_durations, blank_durations, blank_hi: int,
                             max_moves: int = 10):
    """Validation of the TDT-shaped entries and the host arrays the launches read.  Returns
    (px, py, B, S, T, tok, blk, tok_arr, blk_arr) with px and py contiguous."""
    import ctypes
    _require_gpu(px, "px"); _require_gpu(py, "py")
    if px.dtype != torch.float32 or py.dtype != torch.float32:
        raise TypeError("px and py must be float32")
    tok, blk = _check_tdt_moves(token_durations, blank_durations, blank_hi, max_moves)
    Dx, Dy = len(tok), len(blk)
    if px.dim() != 4 or py.dim() != 4:
        raise ValueError("px must be [B,Dx,S,T+1] and py [B,Dy,S+1,T]")
    B, _, S, T1 = px.shape
    T = py.shape[3]
    if T1 != T + 1:
        raise ValueError(f"px.shape[-1]={T1} must be T+1 with T=py.shape[-1]={T} (regular type only)")
    if tuple(px.shape) != (B, Dx, S, T + 1):
        raise ValueError(f"px must have shape {(B, Dx, S, T + 1)}, got {tuple(px.shape)}")
    if tuple(py.shape) != (B, Dy, S + 1, T):
        raise ValueError(f"py must have shape {(B, Dy, S + 1, T)}, got {tuple(py.shape)}")
    tok_arr = (ctypes.c_int32 * Dx)(*tok)       # read by the launch itself: no device copy, no host synchronisation
    blk_arr = (ctypes.c_int32 * Dy)(*blk)
    return px.contiguous(), py.contiguous(), B, S, T, tok, blk, tok_arr, blk_arr


def tdt_forward_backward(px: torch.Tensor, py: torch.Tensor, token_durations, blank_durations,
                         boundary: Optional[torch.Tensor], need_grads: bool):
    """The TDT recursion on raw tensors (no autograd): forward and, when wanted, the backward seeded with ones, back to
    back on torch's current stream.  Returns (ans, px_grad|None, py_grad|None)."""
    px, py, B, S, T, tok, blk, tok_arr, blk_arr = _duration_lattice_inputs(px, py, token_durations, blank_durations, 16)
    Dx, Dy = len(tok), len(blk)
    boundary = _as_boundary(boundary, B, px.device)
    L = _lib.lib()
    with torch.cuda.device(px.device):
        st = _stream_ptr(px)
        nws = L.ftr_mutual_information_tdt_workspace_floats(B, S, T)
        ws = torch.empty((max(nws, 2) + 1) // 2, dtype=torch.float64, device=px.device)
        ans = torch.empty((B,), dtype=torch.float32, device=px.device)
        _lib.call("ftr_mutual_information_tdt_fwd_f32", _ptr(px), _ptr(py), _ptr(boundary), tok_arr, Dx, blk_arr, Dy,
                  _ptr(ws), nws, _ptr(ans), B, S, T, st)
        if not need_grads:
            return ans, None, None
        px_grad = torch.empty_like(px)
        py_grad = torch.empty_like(py)
        _lib.call("ftr_mutual_information_tdt_bwd_f32", _ptr(px), _ptr(py), _ptr(boundary), tok_arr, Dx, blk_arr, Dy,
                  _ptr(ws), nws, None, _ptr(px_grad), _ptr(py_grad), B, S, T, st)
    return ans, px_grad, py_grad


def mutual_information_recursion_tdt(
    px: torch.Tensor,
    py: torch.Tensor,
    token_durations,
    blank_durations,
    boundary: Optional[torch.Tensor] = None,
    calc_gradients: bool = False,
) -> Union[Tuple[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]], torch.Tensor]:
    """``mutual_information_recursion`` over the lattice of the token-and-duration transducer (TDT; Xu et al., "Efficient
    Sequence Transduction by Jointly Predicting Tokens and Durations", ICML 2023; MI355X addition, no reference
    counterpart; csrc/mi_tdt.hip): every move, symbol or blank, also says how many frames it advances.  Regular type only.

    px: [B,Dx,S,T+1], ``px[b,i,s,t]`` being the log-probability of the move (s,t) -> (s+1,t+token_durations[i]);
    py: [B,Dy,S+1,T], ``py[b,j,s,t]`` that of the move (s,t) -> (s,t+blank_durations[j]).  token_durations: Dx >= 1
    strictly increasing ints in 0..16; blank_durations: Dy >= 1 strictly increasing ints in 1..16; Dx + Dy <= 10;
    boundary: int32 [B,4] or None.

        p[s,t] = logadd(logadd_i p[s-1,t-e_i] + px[i,s-1,t-e_i], logadd_j p[s,t-d_j] + py[j,s,t-d_j]),  p[s_begin,t_begin] = 0

    Moves that would leave the boundary rectangle are ignored whatever value they carry.  Returns ``ans`` [B] =
    ``p[s_end,t_end]`` (-inf when no path exists; the gradients are then zero, never NaN; 0 for an inverted rectangle);
    with ``calc_gradients`` also ``(px_grad, py_grad)``, the occupancies, in the shapes of px and py and zero outside
    the rectangle.  With ``token_durations=(0,)`` this is ``mutual_information_recursion_multiblank``, with ``(0,)`` and
    ``(1,)`` the lattice of ``mutual_information_recursion``.  Differentiable w.r.t. px and py; asynchronous on torch's
    current stream, no host read (capturable)."""
    tok, blk = tuple(token_durations), tuple(blank_durations)
    ans, px_grad, py_grad = _Occupancies.apply(px, py, calc_gradients, "mutual_information_recursion_tdt",
                                               lambda x, y, need: tdt_forward_backward(x, y, tok, blk, boundary, need))
    return (ans, (px_grad, py_grad)) if calc_gradients else ans


def band_forward_backward(px_band: torch.Tensor, py_band: torch.Tensor, ranges: torch.Tensor, S: int,
                          boundary: Optional[torch.Tensor], modified):
    """The ordinary recursion on band-shaped operands [B,T,r], raw tensors (no autograd): forward recursion, cut and backward
    recursion in one launch on torch's current stream; its workspace (none for the LDS-resident kernel) is a local and goes
    with the return.  Returns (ans, gx_band, gy_band); the occupancies are seeded with ones.  ``ranges`` must be a band the
    kernels cover (the caller's business: _band_path_ok of rnnt_loss.py)."""
    B, T, r = px_band.shape
    dev = px_band.device
    ans = torch.empty((B,), dtype=torch.float32, device=dev)
    gx = torch.empty_like(px_band)
    gy = torch.empty_like(py_band)
    with torch.cuda.device(dev):
        nws = _lib.lib().ftr_mutual_information_band_workspace_floats(B, T, int(S), r)   # 0: the LDS-resident kernel
        ws = torch.empty((nws,), dtype=torch.float32, device=dev) if nws else None
        _lib.call("ftr_mutual_information_band_ws_f32", _ptr(px_band), _ptr(py_band), _ptr(ranges), _ptr(boundary), _ptr(ws), nws,
                  _ptr(ans), _ptr(gx), _ptr(gy), B, T, int(S), r, int(modified), _stream_ptr(px_band))
    return ans, gx, gy


def band_tdt_supported(T: int, S: int, r: int, N: int, Ny: int) -> bool:
    """Does the band-native TDT recursion (csrc/mi_band_tdt.hip) cover these sizes?"""
    return _lib.lib().ftr_mutual_information_band_tdt_supported(int(T), int(S), int(r), int(N), int(Ny)) != 0


def band_tdt_forward_backward(px_band: torch.Tensor, py_band: torch.Tensor, ranges: torch.Tensor, S: int, token_durations,
                              blank_durations, boundary: Optional[torch.Tensor], need_grads: bool):
    """The TDT recursion on band-shaped operands, raw tensors (no autograd): one chain launch for both directions and
    one occupancy launch on torch's current stream.  Returns (ans, gx_band|None, gy_band|None); the occupancies are
    seeded with ones.  ``ranges`` must be a band (the caller's business: _is_band of rnnt_loss.py)."""
    import ctypes
    tok, blk = _check_tdt_moves(token_durations, blank_durations, 16)
    N, Ny = len(tok), len(blk)
    B, _, T, r = px_band.shape
    tok_arr = (ctypes.c_int32 * N)(*tok)        # read by the launch itself: no device copy, no host synchronisation
    blk_arr = (ctypes.c_int32 * Ny)(*blk)
    L = _lib.lib()
    with torch.cuda.device(px_band.device):
        st = _stream_ptr(px_band)
        nws = L.ftr_mutual_information_band_tdt_workspace_floats(B, T, int(S), r, N, Ny)
        ws = torch.empty((max(nws, 2) + 1) // 2, dtype=torch.float64, device=px_band.device)
        ans = torch.empty((B,), dtype=torch.float32, device=px_band.device)
        gx = torch.empty_like(px_band) if need_grads else None
        gy = torch.empty_like(py_band) if need_grads else None
        _lib.call("ftr_mutual_information_band_tdt_f32", _ptr(px_band), _ptr(py_band), _ptr(ranges), _ptr(boundary), tok_arr, N,
                  blk_arr, Ny, _ptr(ws), nws, _ptr(ans), _ptr(gx), _ptr(gy), B, T, int(S), r, st)
        _lib.band_tdt_recursions += 1
    return ans, gx, gy


class _BandTdtRecursion(torch.autograd.Function):
    """mutual_information_recursion_tdt_band: the occupancies are computed with the answer whenever an operand needs a
    gradient, and backward() scales them by the upstream gradient."""

    @staticmethod
    def forward(ctx, px_band, py_band, ranges, S, tok, blk, boundary):
        need = px_band.requires_grad or py_band.requires_grad
        ans, gx, gy = band_tdt_forward_backward(px_band.detach().contiguous(), py_band.detach().contiguous(), ranges, S, tok,
                                                blk, boundary, need)
        if need:
            ctx.save_for_backward(gx, gy)
        return ans

    @staticmethod
    def backward(ctx, g_ans):
        gx, gy = ctx.saved_tensors
        g = g_ans.reshape(-1, 1, 1, 1).to(gx.dtype)
        return gx * g, gy * g, None, None, None, None, None


def mutual_information_recursion_tdt_band(
    px_band: torch.Tensor,
    py_band: torch.Tensor,
    ranges: torch.Tensor,
    durations,
    blank_durations,
    boundary: Optional[torch.Tensor] = None,
    S: Optional[int] = None,
) -> torch.Tensor:
    """``mutual_information_recursion_tdt`` on the pruned band itself (MI355X addition; csrc/mi_band_tdt.hip): nothing of
    size S*T is allocated or touched.

    px_band: [B,N,T,r] and py_band: [B,Ny,T,r], float32; element (b,i,t,k) is the log-probability of move i out of
    lattice cell (ranges[b,t,0] + k, t), i.e. what ``get_rnnt_logprobs_tdt_pruned`` puts at ``px[b,i,s,t]`` /
    ``py[b,j,s,t]`` (its -inf rules included).  ranges: int32 [B,T,r], a band as ``get_rnnt_prune_ranges`` returns it
    (``ranges[b,t,k] = ranges[b,t,0] + k``, non-decreasing over t), r <= 15.  S: the number of symbols (the lattice has
    rows 0..S); when omitted it is taken to be ``ranges.max()``, the last band row, at the price of one host read.
    durations: the N token durations,
    strictly increasing ints in 0..16, N <= 5; blank_durations: the Ny blank durations in 1..16, Ny <= 5.

    A move exists iff its source is a band cell inside the boundary rectangle and its destination is one, or the end
    cell ``(s_end, t_end)``; the frames it skips need not be in the band.  Returns ``ans`` [B] (-inf without a path;
    NaN for a band whose start decreases), equal to ``mutual_information_recursion_tdt`` on the band scattered into
    full-size lattices of -inf.  Differentiable w.r.t. px_band and py_band (the occupancies times the upstream
    gradient); asynchronous, no host read when ``S`` is given (capturable)."""
    _require_gpu(px_band, "px_band"); _require_gpu(py_band, "py_band")
    if px_band.dtype != torch.float32 or py_band.dtype != torch.float32:
        raise TypeError("px_band and py_band must be float32")
    tok, blk = _check_tdt_moves(durations, blank_durations, 16)
    if len(tok) > 5 or len(blk) > 5:
        raise ValueError("the band recursion takes at most 5 token durations and 5 blank durations")
    if px_band.dim() != 4 or py_band.dim() != 4:
        raise ValueError("px_band must be [B,N,T,r] and py_band [B,Ny,T,r]")
    B, _, T, r = px_band.shape
    if tuple(px_band.shape) != (B, len(tok), T, r) or tuple(py_band.shape) != (B, len(blk), T, r):
        raise ValueError(f"px_band must have shape {(B, len(tok), T, r)} and py_band {(B, len(blk), T, r)}, got "
                         f"{tuple(px_band.shape)} and {tuple(py_band.shape)}")
    ranges = torch.as_tensor(ranges, device=px_band.device).to(torch.int32).contiguous()
    if tuple(ranges.shape) != (B, T, r):
        raise ValueError(f"ranges must have shape {(B, T, r)}, got {tuple(ranges.shape)}")
    boundary = _as_boundary(boundary, B, px_band.device)
    if S is None:       # the last band row: one host read (give S to stay asynchronous)
        S = int(ranges.max().item()) if ranges.numel() else 0
    S = int(S)
    if S < 0 or T < 1:
        raise ValueError(f"S={S} must not be negative and T={T} must be positive")
    if not band_tdt_supported(T, S, r, len(tok), len(blk)):
        raise ValueError(f"the band recursion does not cover T={T}, S={S}, r={r} (r <= 15)")
    return _BandTdtRecursion.apply(px_band, py_band, ranges, S, tok, blk, boundary)


def band_multiblank_supported(T: int, S: int, r: int, D: int) -> bool:
    """Does the band-native multi-blank recursion (the multi-blank domain of csrc/mi_band_tdt.hip) cover these sizes?"""
    return _lib.lib().ftr_mutual_information_band_multiblank_supported(int(T), int(S), int(r), int(D)) != 0


def band_multiblank_forward_backward(px_band: torch.Tensor, py_band: torch.Tensor, ranges: torch.Tensor, S: int, durations,
                                     boundary: Optional[torch.Tensor], need_grads: bool):
    """The multi-blank recursion on band-shaped operands, raw tensors (no autograd): one chain launch for both directions
    and one occupancy launch on torch's current stream.  Returns (ans, gx_band|None, gy_band|None); the occupancies are
    seeded with ones.  ``ranges`` must be a band (the caller's business: _is_band of rnnt_loss.py)."""
    import ctypes
    durs = _check_durations(durations)
    D = len(durs)
    B, T, r = px_band.shape
    dur_arr = (ctypes.c_int32 * D)(*durs)       # read by the launch itself: no device copy, no host synchronisation
    L = _lib.lib()
    with torch.cuda.device(px_band.device):
        st = _stream_ptr(px_band)
        nws = L.ftr_mutual_information_band_multiblank_workspace_floats(B, T, int(S), r, D)
        ws = torch.empty((max(nws, 2) + 1) // 2, dtype=torch.float64, device=px_band.device)
        ans = torch.empty((B,), dtype=torch.float32, device=px_band.device)
        gx = torch.empty_like(px_band) if need_grads else None
        gy = torch.empty_like(py_band) if need_grads else None
        _lib.call("ftr_mutual_information_band_multiblank_f32", _ptr(px_band), _ptr(py_band), _ptr(ranges), _ptr(boundary),
                  dur_arr, D, _ptr(ws), nws, _ptr(ans), _ptr(gx), _ptr(gy), B, T, int(S), r, st)
        _lib.band_multiblank_recursions += 1
    return ans, gx, gy


class _BandMultiblankRecursion(torch.autograd.Function):
    """mutual_information_recursion_multiblank_band: the occupancies are computed with the answer whenever an operand
    needs a gradient, and backward() scales them by the upstream gradient."""

    @staticmethod
    def forward(ctx, px_band, py_band, ranges, S, durs, boundary):
        need = px_band.requires_grad or py_band.requires_grad
        ans, gx, gy = band_multiblank_forward_backward(px_band.detach().contiguous(), py_band.detach().contiguous(), ranges, S,
                                                       durs, boundary, need)
        if need:
            ctx.save_for_backward(gx, gy)
        return ans

    @staticmethod
    def backward(ctx, g_ans):
        gx, gy = ctx.saved_tensors
        g = g_ans.to(gx.dtype)
        return gx * g.reshape(-1, 1, 1), gy * g.reshape(-1, 1, 1, 1), None, None, None, None


def mutual_information_recursion_multiblank_band(
    px_band: torch.Tensor,
    py_band: torch.Tensor,
    ranges: torch.Tensor,
    durations,
    boundary: Optional[torch.Tensor] = None,
    S: Optional[int] = None,
) -> torch.Tensor:
    """``mutual_information_recursion_multiblank`` on the pruned band itself (MI355X addition; the multi-blank domain of
    csrc/mi_band_tdt.hip): nothing of size S*T is allocated or touched.

    px_band: [B,T,r] and py_band: [B,D,T,r], float32; element (b,t,k) / (b,j,t,k) is the log-probability of the symbol
    move / of blank j out of lattice cell (ranges[b,t,0] + k, t), i.e. what ``get_rnnt_logprobs_multiblank_pruned`` puts
    at ``px[b,s,t]`` / ``py[b,j,s,t]`` (its -inf rules included).  ranges: int32 [B,T,r], a band as
    ``get_rnnt_prune_ranges`` returns it (``ranges[b,t,k] = ranges[b,t,0] + k``, non-decreasing over t), r <= 15.  S: the
    number of symbols (the lattice has rows 0..S); when omitted it is taken to be ``ranges.max()``, the last band row, at
    the price of one host read.  durations: the D blank durations, 1..8 strictly increasing ints in 1..32 (they need not
    contain 1).

    A move exists iff its source is a band cell inside the boundary rectangle and its destination is one, or the end
    cell ``(s_end, t_end)``; the frames a blank skips need not be in the band.  Returns ``ans`` [B] (-inf without a path;
    NaN for a band whose start decreases), equal to ``mutual_information_recursion_multiblank`` on the band scattered
    into full-size lattices of -inf.  Differentiable w.r.t. px_band and py_band (the occupancies times the upstream
    gradient); asynchronous, no host read when ``S`` is given (capturable)."""
    _require_gpu(px_band, "px_band"); _require_gpu(py_band, "py_band")
    if px_band.dtype != torch.float32 or py_band.dtype != torch.float32:
        raise TypeError("px_band and py_band must be float32")
    durs = _check_durations(durations)
    if px_band.dim() != 3 or py_band.dim() != 4:
        raise ValueError("px_band must be [B,T,r] and py_band [B,D,T,r]")
    B, T, r = px_band.shape
    if tuple(py_band.shape) != (B, len(durs), T, r):
        raise ValueError(f"py_band must have shape {(B, len(durs), T, r)}, got {tuple(py_band.shape)}")
    ranges = torch.as_tensor(ranges, device=px_band.device).to(torch.int32).contiguous()
    if tuple(ranges.shape) != (B, T, r):
        raise ValueError(f"ranges must have shape {(B, T, r)}, got {tuple(ranges.shape)}")
    boundary = _as_boundary(boundary, B, px_band.device)
    if S is None:       # the last band row: one host read (give S to stay asynchronous)
        S = int(ranges.max().item()) if ranges.numel() else 0
    S = int(S)
    if S < 0 or T < 1:
        raise ValueError(f"S={S} must not be negative and T={T} must be positive")
    if not band_multiblank_supported(T, S, r, len(durs)):
        raise ValueError(f"the band recursion does not cover T={T}, S={S}, r={r} (r <= 15)")
    return _BandMultiblankRecursion.apply(px_band, py_band, ranges, S, durs, boundary)


def mutual_information_viterbi(px: torch.Tensor, py: torch.Tensor,
                               boundary: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Best-path (Viterbi) alignment over the lattice of ``mutual_information_recursion`` (MI355X addition, no reference
    counterpart; ftr_mutual_information_viterbi_f32, csrc/mi_viterbi.hip).

    Same inputs and validation as ``mutual_information_recursion``: px [B,S,T+1] (regular) or [B,S,T] (modified),
    py [B,S+1,T], float32; boundary int32 [B,4] rows (s_begin, t_begin, s_end, t_end) or None.  The recursion with
    LogAdd replaced by a select::

        a = p[s-1, t+off] + px[s-1, t+off]    (off = 0 regular, -1 modified; -inf where the recursion's guards say so)
        c = p[s, t-1] + py[s, t-1]
        take_px = (a != a) or (a >= c)        # NaN propagates, ties go to the px (symbol) move
        p[s, t] = a if take_px else c         # exactly this, not fmax

    with ``p[s_begin, t_begin] = 0``.  Returns ``(score, frames)``:

    * ``score`` [B] float32 = ``p[s_end, t_end]``, bit-identical to a float32 restatement (one add and one select per
      cell: the order of evaluation cannot change the bits);
    * ``frames`` [B,S] int32: ``frames[b,s]`` is the frame at which the best path takes the px move out of row s, i.e.
      emits ``symbols[b,s]`` (regular: (s,t)->(s+1,t), non-decreasing; modified: (s,t)->(s+1,t+1), strictly
      increasing).  Rows outside [s_begin, s_end) are -1, and the whole row is -1 when ``score[b]`` is -inf (no path)
      or NaN.  An inverted rectangle gives score 0 (as ``mutual_information_recursion``) and frames -1.

    Not differentiable: both outputs are detached.  Asynchronous on torch's current stream, no host read (capturable).
    """
    px, py, B, S, T, modified = _lattice_inputs(px.detach(), py.detach())
    boundary = _as_boundary(boundary, B, px.device)
    L = _lib.lib()
    with torch.cuda.device(px.device):
        nbytes = L.ftr_mutual_information_viterbi_workspace_bytes(B, S, T)
        ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=px.device)
        score = torch.empty((B,), dtype=torch.float32, device=px.device)
        frames = torch.empty((B, S), dtype=torch.int32, device=px.device)
        _lib.call("ftr_mutual_information_viterbi_f32", _ptr(px), _ptr(py), _ptr(boundary), _ptr(ws), nbytes,
                  _ptr(score), _ptr(frames), B, S, T, modified, _stream_ptr(px))
    return score, frames


def mutual_information_viterbi_tdt(px: torch.Tensor, py: torch.Tensor, token_durations, blank_durations,
                                   boundary: Optional[torch.Tensor] = None
                                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Best-path (Viterbi) alignment over the lattice of ``mutual_information_recursion_tdt`` (MI355X addition, no
    reference counterpart; ftr_mutual_information_viterbi_tdt_f32, csrc/mi_viterbi_tdt.hip).  ``token_durations=(0,)``
    is the multi-blank lattice, ``(0,)`` with ``(1,)`` the ordinary one.  Regular type only.

    px [B,Dx,S,T+1], py [B,Dy,S+1,T], float32, as ``mutual_information_recursion_tdt``; token_durations: Dx >= 1
    strictly increasing ints in 0..16; blank_durations: Dy >= 1 strictly increasing ints in 1..32 (a big blank may
    advance 32 frames); Dx + Dy <= 9; boundary int32 [B,4] or None.  The moves m = 0..M-1 are the token moves in list
    order, then the blank moves in list order, and for every cell but (s_begin,t_begin)::

        cand[m] = p[src_m] + op_m[src_m]      # one float32 add; src_m = (s-1, t-e_i) or (s, t-d_j); -inf when src_m
                                              # lies outside the boundary rectangle, whatever the operand holds
        best, move = cand[M-1], M-1
        for m in M-2 .. 0:
            take = (cand[m] != cand[m]) or (cand[m] >= best)
            if take: best, move = cand[m], m
        p[s, t] = best

    with ``p[s_begin, t_begin] = 0``: a NaN propagates and a tie goes to the lowest-index move (tokens before blanks,
    shorter durations before longer).  With ``(0,)`` / ``(1,)`` this is the rule of ``mutual_information_viterbi``.
    Returns ``(score, frames, durations, blank_steps)``:

    * ``score`` [B] float32 = ``p[s_end, t_end]``, bit-identical to a float32 restatement;
    * ``frames`` [B,S] int32: the source frame of the token move the best path takes out of row s (it emits
      ``symbols[b,s]`` there);
    * ``durations`` [B,S] int32: the number of frames that move advances, a member of ``token_durations``;
    * ``blank_steps`` [B,T] int32: the duration of the blank move the best path takes out of frame t, 0 when it leaves
      t by a token move or skips it.

    Rows outside [s_begin, s_end) are -1 in ``frames`` and ``durations``, frames outside [t_begin, t_end) are -1 in
    ``blank_steps``, all three are entirely -1 for an utterance whose score is -inf (no path) or NaN, and an inverted
    rectangle gives score 0 and -1 everywhere.  Not differentiable: the outputs are detached.  Asynchronous on torch's
    current stream, no host read (capturable)."""
    px, py, B, S, T, tok, blk, tok_arr, blk_arr = _duration_lattice_inputs(px.detach(), py.detach(), token_durations,
                                                                           blank_durations, 32, max_moves=9)   # a blank above 16, nine moves: this entry alone
    Dx, Dy = len(tok), len(blk)
    boundary = _as_boundary(boundary, B, px.device)
    L = _lib.lib()
    with torch.cuda.device(px.device):
        nbytes = L.ftr_mutual_information_viterbi_tdt_workspace_bytes(B, S, T)
        ws = torch.empty(((max(nbytes, 8) + 7) // 8,), dtype=torch.int64, device=px.device)
        score = torch.empty((B,), dtype=torch.float32, device=px.device)
        frames = torch.empty((B, S), dtype=torch.int32, device=px.device)
        durations = torch.empty((B, S), dtype=torch.int32, device=px.device)
        blank_steps = torch.empty((B, T), dtype=torch.int32, device=px.device)
        _lib.call("ftr_mutual_information_viterbi_tdt_f32", _ptr(px), _ptr(py), _ptr(boundary), tok_arr, Dx, blk_arr, Dy,
                  _ptr(ws), nbytes, _ptr(score), _ptr(frames), _ptr(durations), _ptr(blank_steps), B, S, T,
                  _stream_ptr(px))
    return score, frames, durations, blank_steps


def band_viterbi_supported(T: int, S: int, r: int, N: int, Ny: int) -> bool:
    """Does the band-native alignment (csrc/mi_band_viterbi.hip) cover these sizes?"""
    return _lib.lib().ftr_mutual_information_band_viterbi_supported(int(T), int(S), int(r), int(N), int(Ny)) != 0


def mutual_information_viterbi_tdt_band(px_band: torch.Tensor, py_band: torch.Tensor, ranges: torch.Tensor, token_durations,
                                        blank_durations, boundary: Optional[torch.Tensor] = None, S: Optional[int] = None
                                        ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``mutual_information_viterbi_tdt`` on the pruned band itself (MI355X addition; ftr_mutual_information_band_viterbi_f32,
    csrc/mi_band_viterbi.hip): nothing of size S*T is allocated or touched, one launch.

    px_band: [B,N,T,r] and py_band: [B,Ny,T,r], float32, ranges: int32 [B,T,r], a band with r <= 15, and S as
    ``mutual_information_recursion_tdt_band`` takes them (S omitted: ``ranges.max()``, one host read).  token_durations:
    N >= 1 strictly increasing ints in 0..16; blank_durations: Ny >= 1 strictly increasing ints in 1..32; N + Ny <= 9 (the
    domain of ``mutual_information_viterbi_tdt``).  boundary: int32 or int64 [B,4], or None.

    The cells are the band cells of the frames ``t_begin <= t < t_end`` inside the rectangle and the end cell; a move
    exists iff its source and its destination are such cells; its candidate is ``p[src] + operand`` in float32, -inf when
    it does not exist, and the select rule is that of ``mutual_information_viterbi_tdt`` (a NaN propagates, a tie goes to
    the lowest-index move).  Returns ``(score, frames, durations, blank_steps)`` with the shapes [B], [B,S], [B,S], [B,T]
    and the conventions of that function; a band whose start decreases inside the rectangle gives score NaN and -1
    everywhere.  Where the operands obey the builders' -inf rules, all four equal ``mutual_information_viterbi_tdt`` on
    the band scattered into lattices of -inf, bit for bit -- for rectangles without NaN: on the lattice a NaN also
    travels through cells outside the band, here only along moves that exist.  Not differentiable: the outputs are
    detached.  Asynchronous, no host read when ``S`` is given (capturable)."""
    import ctypes
    _require_gpu(px_band, "px_band"); _require_gpu(py_band, "py_band")
    if px_band.dtype != torch.float32 or py_band.dtype != torch.float32:
        raise TypeError("px_band and py_band must be float32")
    tok, blk = _check_tdt_moves(token_durations, blank_durations, 32, max_moves=9)
    if px_band.dim() != 4 or py_band.dim() != 4:
        raise ValueError("px_band must be [B,N,T,r] and py_band [B,Ny,T,r]")
    B, _, T, r = px_band.shape
    N, Ny = len(tok), len(blk)
    if tuple(px_band.shape) != (B, N, T, r) or tuple(py_band.shape) != (B, Ny, T, r):
        raise ValueError(f"px_band must have shape {(B, N, T, r)} and py_band {(B, Ny, T, r)}, got "
                         f"{tuple(px_band.shape)} and {tuple(py_band.shape)}")
    if py_band.device != px_band.device:
        raise ValueError("px_band and py_band must be on the same device")
    px_band = px_band.detach().contiguous(); py_band = py_band.detach().contiguous()
    ranges = torch.as_tensor(ranges, device=px_band.device).to(torch.int32).contiguous()
    if tuple(ranges.shape) != (B, T, r):
        raise ValueError(f"ranges must have shape {(B, T, r)}, got {tuple(ranges.shape)}")
    boundary = _as_boundary(boundary, B, px_band.device)
    if S is None:       # the last band row: one host read (give S to stay asynchronous)
        S = int(ranges.max().item()) if ranges.numel() else 0
    S = int(S)
    if S < 0 or T < 1:
        raise ValueError(f"S={S} must not be negative and T={T} must be positive")
    if not band_viterbi_supported(T, S, r, N, Ny):
        raise ValueError(f"the band alignment does not cover T={T}, S={S}, r={r} (r <= 15)")
    tok_arr = (ctypes.c_int32 * N)(*tok)        # read by the launch itself: no device copy, no host synchronisation
    blk_arr = (ctypes.c_int32 * Ny)(*blk)
    L = _lib.lib()
    with torch.cuda.device(px_band.device):
        nbytes = L.ftr_mutual_information_band_viterbi_workspace_bytes(B, T, S, r, N, Ny)
        ws = torch.empty(((max(nbytes, 8) + 7) // 8,), dtype=torch.int64, device=px_band.device)
        score = torch.empty((B,), dtype=torch.float32, device=px_band.device)
        frames = torch.empty((B, S), dtype=torch.int32, device=px_band.device)
        durations = torch.empty((B, S), dtype=torch.int32, device=px_band.device)
        blank_steps = torch.empty((B, T), dtype=torch.int32, device=px_band.device)
        _lib.call("ftr_mutual_information_band_viterbi_f32", _ptr(px_band), _ptr(py_band), _ptr(ranges), _ptr(boundary), tok_arr, N,
                  blk_arr, Ny, _ptr(ws), nbytes, _ptr(score), _ptr(frames), _ptr(durations), _ptr(blank_steps), B, T, S, r,
                  _stream_ptr(px_band))
    return score, frames, durations, blank_steps


def cummin(x: torch.Tensor) -> torch.Tensor:
    """Op "Cummin" (__init__.py:151-152; tf_fast_rnnt_op.cc:135-165): inclusive prefix-min along the
    last axis of an int32 [rows, cols] matrix."""
    _require_gpu(x, "x")
    if x.dim() != 2:
        raise ValueError("cummin expects a 2-D tensor")
    if x.dtype != torch.int32:
        raise TypeError("cummin expects int32 (op registration: tf_fast_rnnt_op.cc:36-38)")
    x = x.contiguous()
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.call("ftr_cummin_i32", _ptr(x), _ptr(out), x.shape[0], x.shape[1], _stream_ptr(x))
    return out
