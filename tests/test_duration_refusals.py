"""What the duration-lattice functions of tf_fast_rnnt (multi-blank, TDT, TDT-mixed, their band forms and the alignments)
answer to bad arguments, and which check answers first when two arguments are bad.  Every call is made with CPU tensors
(B=2, T=4, s_range=2, C=6, S=3; TDT rows have C + N = 8 columns) and is made twice:

* as it is: most of these functions ask for a device before they look at anything else, and the row records that;
* with the device question waived (the ``... | waived`` rows): ``_require_gpu`` answers nothing and the first thing that
  needs a device (``torch.cuda.device`` / ``current_stream``) raises a marker instead, recorded as
  ``["device", "asked for"]``.  These rows reach every check behind the device question, in its order.

The last row of every function is the call with nothing wrong: a refusal to run without a device, as it is, and the marker,
waived.  The exception types and texts are recorded in tests/golden/duration_python_refusals.json.

    python tests/test_duration_refusals.py        records the golden from the package as it stands"""
import contextlib
import json
import os
import sys
from unittest import mock

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "duration_python_refusals.json")

B, T, R, C, S = 2, 4, 2, 6, 3
F64 = torch.float64


def _x(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


def _i(*shape):
    return torch.zeros(*shape, dtype=torch.int32)


MB_LOSSES = ("rnnt_loss_multiblank_pruned", "rnnt_loss_multiblank")
MB_BUILDERS = ("get_rnnt_logprobs_multiblank_pruned", "get_rnnt_logprobs_multiblank_joint")
TDT_LOSSES = ("rnnt_loss_tdt_pruned", "rnnt_loss_tdt")
TDT_BUILDERS = ("get_rnnt_logprobs_tdt_pruned", "get_rnnt_logprobs_tdt_joint")
MIX_LOSSES = ("rnnt_loss_tdt_mixed_pruned", "rnnt_loss_tdt_mixed")
ALIGN_TDT, ALIGN_MB = "rnnt_alignment_tdt_pruned", "rnnt_alignment_multiblank_pruned"
REC_MB, REC_TDT = "mutual_information_recursion_multiblank", "mutual_information_recursion_tdt"
VIT, VIT_BAND = "mutual_information_viterbi_tdt", "mutual_information_viterbi_tdt_band"
MB_FAMILY = MB_LOSSES + MB_BUILDERS + (ALIGN_MB,)
TDT_FAMILY = TDT_LOSSES + TDT_BUILDERS + MIX_LOSSES + (ALIGN_TDT,)


def _base(func):
    """the arguments of a call with nothing wrong"""
    if func in (REC_MB, REC_MB + "_band"):
        band = func.endswith("_band")
        args = dict(px=_x(B, S, T + 1), py=_x(B, 2, S + 1, T), durations=(1, 2))
        return dict(px_band=_x(B, T, R), py_band=_x(B, 2, T, R), ranges=_i(B, T, R), durations=(1, 2), S=S) if band else args
    if func in (REC_TDT, VIT):
        return dict(px=_x(B, 2, S, T + 1), py=_x(B, 1, S + 1, T), token_durations=(0, 1), blank_durations=(1,))
    if func in (REC_TDT + "_band", VIT_BAND):
        names = ("durations", "blank_durations") if func == REC_TDT + "_band" else ("token_durations", "blank_durations")
        return {"px_band": _x(B, 2, T, R), "py_band": _x(B, 1, T, R), "ranges": _i(B, T, R), names[0]: (0, 1), names[1]: (1,), "S": S}
    tdt = func in TDT_FAMILY
    joint = not func.endswith("_pruned")
    args = dict(logits=_x(B, T, S + 1 if joint else R, C + 2 if tdt else C), symbols=_i(B, S), termination_symbol=0)
    if not joint:
        args["ranges"] = _i(B, T, R)
    if func in MB_BUILDERS + TDT_BUILDERS:
        args["boundary"] = None
    args.update(dict(durations=(0, 1)) if tdt else dict(big_blanks=((1, 2),)))
    if func in MIX_LOSSES:
        args["omega"] = 0.3
    return args


def _logits(func, dtype=torch.float32, rank3=False):
    shape = tuple(_base(func)["logits"].shape)
    return dict(logits=_x(*(shape[:3] if rank3 else shape), dtype=dtype))


def _rows(funcs, label, over):
    return [(f, label, over(f) if callable(over) else over) for f in funcs]


# (function, label, what replaces or joins the arguments of _base): each check on its own, then pairs of two bad arguments,
# then, last for each function, the call with nothing wrong
CASES = []
for f in MB_FAMILY:
    loss, pruned = f in MB_LOSSES, f.endswith("_pruned")
    CASES += _rows([f], "logits float64", _logits(f, F64)) + _rows([f], "logits rank 3", _logits(f, rank3=True))
    CASES += [(f, "symbols shape", dict(symbols=_i(B + 1, S))),
              (f, "boundary shape", dict(boundary=_i(B, 3))),
              (f, "sigma -1", dict(sigma=-1.0)),
              (f, "sigma nan", dict(sigma=float("nan"))),
              (f, "big blanks: 8 of them", dict(big_blanks=tuple((i + 1, i + 2) for i in range(8)), logits=_x(B, T, S + 1 if not pruned else R, 12))),
              (f, "big blanks: duration 33", dict(big_blanks=((1, 33),))),
              (f, "big blanks: duration 1", dict(big_blanks=((1, 1),))),
              (f, "big blanks: not increasing", dict(big_blanks=((1, 4), (2, 3)))),
              (f, "big blanks: duplicate id", dict(big_blanks=((1, 2), (1, 3)))),
              (f, "big blanks: id is the blank", dict(big_blanks=((0, 2),))),
              (f, "big blanks: id C", dict(big_blanks=((C, 2),))),
              (f, "big blanks: id -1", dict(big_blanks=((-1, 2),))),
              (f, "termination_symbol C", dict(termination_symbol=C)),
              (f, "termination_symbol -1", dict(termination_symbol=-1)),
              (f, "pair: sigma -1 + big blanks: duration 33", dict(sigma=-1.0, big_blanks=((1, 33),))),
              (f, "pair: big blanks: duration 33 + duplicate id", dict(big_blanks=((1, 33), (1, 34)))),
              (f, "pair: termination_symbol C + big blanks: id C", dict(termination_symbol=C, big_blanks=((C, 2),))),
              (f, "pair: logits float64 + sigma -1", dict(sigma=-1.0, **_logits(f, F64)))]
    if pruned:
        CASES += [(f, "ranges shape", dict(ranges=_i(B, T, R + 1))),
                  (f, "pair: ranges shape + symbols shape", dict(ranges=_i(B, T, R + 1), symbols=_i(B + 1, S)))]
    if loss:
        CASES += [(f, "rnnt_type", dict(rnnt_type="modified")),
                  (f, "reduction", dict(reduction="max")),
                  (f, "pair: rnnt_type + reduction", dict(rnnt_type="modified", reduction="max")),
                  (f, "pair: reduction + sigma -1", dict(reduction="max", sigma=-1.0)),
                  (f, "pair: reduction + logits float64", dict(reduction="max", **_logits(f, F64)))]
    CASES += [(f, "nothing wrong, no big blank", dict(big_blanks=())), (f, "nothing wrong", dict())]

for f in TDT_FAMILY:
    loss, mix, pruned = f in TDT_LOSSES + MIX_LOSSES, f in MIX_LOSSES, f.endswith("_pruned")
    CASES += _rows([f], "logits float64", _logits(f, F64)) + _rows([f], "logits rank 3", _logits(f, rank3=True))
    CASES += [(f, "symbols shape", dict(symbols=_i(B + 1, S))),
              (f, "boundary shape", dict(boundary=_i(B, 3))),
              (f, "sigma -1", dict(sigma=-1.0)),
              (f, "durations: empty", dict(durations=())),
              (f, "durations: 6 of them", dict(durations=(0, 1, 2, 3, 4, 5))),
              (f, "durations: 17", dict(durations=(0, 17))),
              (f, "durations: -1", dict(durations=(-1, 1))),
              (f, "durations: not increasing", dict(durations=(1, 1))),
              (f, "durations: none positive", dict(durations=(0,))),
              (f, "durations: no token column left", dict(durations=(0, 1, 2, 3, 4), logits=_x(B, T, S + 1 if not pruned else R, 5))),
              (f, "termination_symbol C", dict(termination_symbol=C)),
              (f, "termination_symbol -1", dict(termination_symbol=-1)),
              (f, "pair: sigma -1 + durations: 17", dict(sigma=-1.0, durations=(0, 17))),
              (f, "pair: durations: none positive + termination_symbol C", dict(durations=(0,), termination_symbol=C + 1)),
              (f, "pair: durations: 17 + not increasing", dict(durations=(17, 17))),
              (f, "pair: logits float64 + durations: empty", dict(durations=(), **_logits(f, F64)))]
    if pruned:
        CASES += [(f, "ranges shape", dict(ranges=_i(B, T, R + 1))),
                  (f, "pair: ranges shape + durations: empty", dict(ranges=_i(B, T, R + 1), durations=()))]
    if loss:
        CASES += [(f, "reduction", dict(reduction="max")),
                  (f, "pair: reduction + sigma -1", dict(reduction="max", sigma=-1.0)),
                  (f, "pair: reduction + durations: empty", dict(reduction="max", durations=()))]
    if loss and not mix:
        CASES += [(f, "rnnt_type", dict(rnnt_type="constrained")),
                  (f, "pair: rnnt_type + reduction", dict(rnnt_type="constrained", reduction="max"))]
    if mix:
        CASES += [(f, "omega -0.1", dict(omega=-0.1)),
                  (f, "omega 1.5", dict(omega=1.5)),
                  (f, "omega nan", dict(omega=float("nan"))),
                  (f, "omega text", dict(omega="half")),
                  (f, "pair: omega 1.5 + reduction", dict(omega=1.5, reduction="max")),
                  (f, "pair: omega 1.5 + durations: empty", dict(omega=1.5, durations=())),
                  (f, "pair: omega 0 + reduction", dict(omega=0.0, reduction="max")),
                  (f, "nothing wrong, omega 0", dict(omega=0.0)),
                  (f, "nothing wrong, omega 1", dict(omega=1.0))]
    CASES += [(f, "nothing wrong", dict())]

for f in (REC_MB, REC_MB + "_band"):
    band = f.endswith("_band")
    x, y = ("px_band", "py_band") if band else ("px", "py")
    good_x, good_y = _base(f)[x], _base(f)[y]
    CASES += [(f, "px float64", {x: good_x.to(F64)}),
              (f, "py float64", {y: good_y.to(F64)}),
              (f, "durations: empty", dict(durations=())),
              (f, "durations: 9 of them", dict(durations=tuple(range(1, 10)))),
              (f, "durations: 33", dict(durations=(1, 33))),
              (f, "durations: 0", dict(durations=(0, 2))),
              (f, "durations: not increasing", dict(durations=(2, 2))),
              (f, "px rank", {x: good_x[0]}),
              (f, "py rank", {y: good_y[:, 0]}),
              (f, "py shape: D", {y: torch.cat([good_y, good_y], 1)}),
              (f, "py shape: T", {y: torch.cat([good_y, good_y], 3 if not band else 2)}),
              (f, "boundary shape", dict(boundary=_i(B, 3))),
              (f, "pair: px float64 + durations: empty", {x: good_x.to(F64), "durations": ()}),
              (f, "pair: durations: 33 + px rank", {x: good_x[0], "durations": (1, 33)}),
              (f, "pair: py shape: D + boundary shape", {y: torch.cat([good_y, good_y], 1), "boundary": _i(B, 3)})]
    if band:
        CASES += [(f, "ranges shape", dict(ranges=_i(B, T, R + 1))),
                  (f, "S -1", dict(S=-1)),
                  (f, "T 0", dict(px_band=_x(B, 0, R), py_band=_x(B, 2, 0, R), ranges=_i(B, 0, R))),
                  (f, "s_range 16", dict(px_band=_x(B, T, 16), py_band=_x(B, 2, T, 16), ranges=_i(B, T, 16), S=20)),
                  (f, "S from the ranges", dict(S=None)),
                  (f, "pair: ranges shape + boundary shape", dict(ranges=_i(B, T, R + 1), boundary=_i(B, 3))),
                  (f, "pair: boundary shape + S -1", dict(boundary=_i(B, 3), S=-1)),
                  (f, "pair: S -1 + s_range 16", dict(px_band=_x(B, T, 16), py_band=_x(B, 2, T, 16), ranges=_i(B, T, 16), S=-1))]
    else:
        CASES += [(f, "px last axis", dict(px=_x(B, S, T))),
                  (f, "pair: px last axis + py shape: D", dict(px=_x(B, S, T), py=torch.cat([good_y, good_y], 1)))]
    CASES += [(f, "nothing wrong", dict())]

for f in (REC_TDT, REC_TDT + "_band", VIT, VIT_BAND):
    band, vit = f.endswith("_band"), f in (VIT, VIT_BAND)
    x, y = ("px_band", "py_band") if band else ("px", "py")
    tok = "durations" if f == REC_TDT + "_band" else "token_durations"
    good_x, good_y = _base(f)[x], _base(f)[y]
    CASES += [(f, "px float64", {x: good_x.to(F64)}),
              (f, "py float64", {y: good_y.to(F64)}),
              (f, "token durations: empty", {tok: ()}),
              (f, "blank durations: empty", dict(blank_durations=())),
              (f, "token durations: 17", {tok: (0, 17)}),
              (f, "token durations: -1", {tok: (-1, 1)}),
              (f, "token durations: not increasing", {tok: (1, 1)}),
              (f, "blank durations: 0", dict(blank_durations=(0,))),
              (f, "blank durations: 17", dict(blank_durations=(17,))),
              (f, "blank durations: 33", dict(blank_durations=(33,))),
              (f, "6 token durations", {tok: tuple(range(6)), x: torch.cat([good_x] * 3, 1)}),
              (f, "6 blank durations", {"blank_durations": tuple(range(1, 7)), y: torch.cat([good_y] * 6, 1)}),
              (f, "10 moves", {tok: tuple(range(5)), "blank_durations": tuple(range(1, 6))}),
              (f, "11 moves", {tok: tuple(range(6)), "blank_durations": tuple(range(1, 6))}),
              (f, "px rank", {x: good_x[0]}),
              (f, "py rank", {y: good_y[:, 0]}),
              (f, "px shape: Dx", {x: good_x[:, :1]}),
              (f, "py shape: Dy", {y: torch.cat([good_y, good_y], 1)}),
              (f, "boundary shape", dict(boundary=_i(B, 3))),
              (f, "pair: px float64 + token durations: empty", {x: good_x.to(F64), tok: ()}),
              (f, "pair: token durations: 17 + blank durations: 0", {tok: (0, 17), "blank_durations": (0,)}),
              (f, "pair: blank durations: empty + 11 moves", {tok: tuple(range(11)), "blank_durations": ()}),
              (f, "pair: 11 moves + px rank", {tok: tuple(range(6)), "blank_durations": tuple(range(1, 6)), x: good_x[0]}),
              (f, "pair: px shape: Dx + py shape: Dy", {x: good_x[:, :1], y: torch.cat([good_y, good_y], 1)}),
              (f, "pair: py shape: Dy + boundary shape", {y: torch.cat([good_y, good_y], 1), "boundary": _i(B, 3)})]
    if band:
        wide = dict(px_band=_x(B, 2, T, 16), py_band=_x(B, 1, T, 16), ranges=_i(B, T, 16))
        CASES += [(f, "ranges shape", dict(ranges=_i(B, T, R + 1))),
                  (f, "S -1", dict(S=-1)),
                  (f, "T 0", dict(px_band=_x(B, 2, 0, R), py_band=_x(B, 1, 0, R), ranges=_i(B, 0, R))),
                  (f, "s_range 16", dict(S=20, **wide)),
                  (f, "S from the ranges", dict(S=None)),
                  (f, "pair: ranges shape + boundary shape", dict(ranges=_i(B, T, R + 1), boundary=_i(B, 3))),
                  (f, "pair: boundary shape + S -1", dict(boundary=_i(B, 3), S=-1)),
                  (f, "pair: S -1 + s_range 16", dict(S=-1, **wide))]
    else:
        CASES += [(f, "px last axis", dict(px=_x(B, 2, S, T))),
                  (f, "pair: px last axis + px shape: Dx", dict(px=_x(B, 1, S, T)))]
    CASES += [(f, "nothing wrong", dict())]

FUNCS = list(dict.fromkeys(func for func, _, _ in CASES))
WAIVED = " | waived"
IDS = [f"{func}: {label}{w}" for func, label, _ in CASES for w in ("", WAIVED)]


class _DeviceAsked(Exception):
    pass


def _ask(*_a, **_k):
    raise _DeviceAsked()


@contextlib.contextmanager
def _device_question_waived(ft):
    quiet = lambda t, name: None
    mi, rl = (sys.modules[f"{ft.__name__}.{m}"] for m in ("mutual_information", "rnnt_loss"))   # ft.rnnt_loss is the function
    with mock.patch.object(mi, "_require_gpu", quiet), mock.patch.object(rl, "_require_gpu", quiet), \
         mock.patch.object(torch.cuda, "device", _ask), mock.patch.object(torch.cuda, "current_stream", _ask), \
         mock.patch.object(torch.cuda, "is_current_stream_capturing", lambda: False):
        yield


def _reply(ft, func, over, waived):
    """[exception type, text] of the call, ["device", "asked for"] for the marker, or [None, "returned"]"""
    try:
        with _device_question_waived(ft) if waived else contextlib.nullcontext():
            getattr(ft, func)(**{**_base(func), **over})
    except _DeviceAsked:
        return ["device", "asked for"]
    except Exception as exc:   # noqa: BLE001  (whatever it is, it is what gets recorded)
        return [type(exc).__name__, str(exc)]
    return [None, "returned"]


def _replies(ft, funcs=FUNCS):
    return {f"{func}: {label}{WAIVED if w else ''}": _reply(ft, func, over, w)
            for func, label, over in CASES if func in funcs for w in (False, True)}


def test_the_table_is_the_recorded_one():
    golden = json.load(open(GOLDEN))
    assert len(set(IDS)) == len(IDS) and set(golden) == set(IDS)
    assert len(FUNCS) == 18
    for func in FUNCS:      # every function's last row: nothing wrong, and no device
        last = [i for i in IDS if i.startswith(func + ": ") and not i.endswith(WAIVED)][-1]
        assert last == f"{func}: nothing wrong", last
        assert golden[last][0] == "RuntimeError" and "no CPU fallback" in golden[last][1], last
        assert golden[last + WAIVED] == ["device", "asked for"], last
    assert sum("pair: " in i for i in IDS) >= 100
    # the waived rows do reach the checks behind the device question: most of them are answered by the package itself
    waived = [golden[i] for i in IDS if i.endswith(WAIVED) and "nothing wrong" not in i]
    assert sum(r[0] in ("ValueError", "TypeError") for r in waived) > 0.8 * len(waived)


@pytest.mark.parametrize("func", FUNCS)
def test_refusals_are_the_recorded_ones(ft, func):
    golden = json.load(open(GOLDEN))
    got = _replies(ft, (func,))
    assert got == {i: golden[i] for i in got}


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tf-fast-rnnt_amd"))
    import tf_fast_rnnt
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as fh:
        json.dump(_replies(tf_fast_rnnt), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", GOLDEN)
