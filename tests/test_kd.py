"""Knowledge distillation on the pruned band (rnnt_kd_loss_pruned), everything that needs no device: the float64
restatement of the definition (tests/kd_restatement.py) against an independent torch composition with autograd, the three
entries of include/ftr_kd.h (declared, exported, bound, validated in the documented order, their replies recorded in
tests/golden/kd_capi_messages.json), and the argument errors of the Python function.

    python tests/test_kd.py        records tests/golden/kd_capi_messages.json from the library as built"""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kd_capi_messages.json")
HEADER = os.path.join(ROOT, "include", "ftr_kd.h")
ENTRIES = ("ftr_pruned_kd_fwd_dt", "ftr_pruned_kd_bwd_scaled_dt", "ftr_pruned_kd_reduce_f32")
KD_DEFAULTS = dict(teacher_kind=0, mode=0)       # parameters the table of tests/test_capi_messages.py does not know
# on top of that table: the checks these entries add, alone and against a bad size / null pointers (which answers first)
KD_EXTRA = [dict(teacher_kind=7), dict(mode=2), dict(mode=-1), dict(temperature=0.0), dict(temperature=-1.0),
            dict(temperature=float("inf")), dict(temperature=float("nan")), dict(kind=7, teacher_kind=7),
            dict(teacher_kind=7, B=-1), dict(mode=2, B=-1), dict(temperature=0.0, B=-1), dict(mode=2, temperature=0.0),
            dict(teacher_kind=7, mode=2), dict(mode=2, termination_symbol=-1), dict(temperature=0.0, scale_stride=2),
            dict(mode=2, B=0), dict(temperature=0.0, B=0), dict(mode=1), dict(temperature=2.0), dict(teacher_kind=2, kind=1)]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _prototype(name):
    m = re.search(r"\b%s\s*\(([^()]*)\)\s*;" % name, _header())
    assert m, f"{name} is not declared in include/ftr_kd.h"
    out = []
    for p in m.group(1).split(","):
        typ, par = re.match(r"(.*?)(\w+)$", " ".join(p.split())).groups()
        out.append((typ.strip(), par))
    return out


def _call(ft, name, **over):
    """The entry with every pointer NULL and small valid sizes, `over` on top (by parameter name)"""
    import test_capi_messages as tcm
    values = {**tcm.DEFAULTS, **KD_DEFAULTS, **over}
    args = []
    for (typ, par), at in zip(_prototype(name), ft._lib._KD_SIGNATURES[name][1]):
        if "*" in typ:
            args.append(None)            # every device pointer and the stream: NULL
        elif at is ctypes.c_float:
            args.append(float(values.get(par, 1.0)))
        else:
            args.append(int(values[par]))
    L = ft._lib.lib()
    return getattr(L, name)(*args), L.ftr_last_error().decode("utf-8", "replace")


def _replies(ft):
    import test_capi_messages as tcm
    got = {}
    for name in ENTRIES:
        names = {par for _, par in _prototype(name)}
        for over in [dict()] + [c for c in tcm.SINGLES + tcm.ARRAYS + KD_EXTRA if set(c) <= names]:
            label = ",".join(f"{k}={over[k]}" for k in over).replace(" ", "") or "default"
            got.setdefault(name, {})[label] = list(_call(ft, name, **over))
    return got


# ---- the definition

@pytest.mark.parametrize("sym_is_blank", [False, True])
@pytest.mark.parametrize("tau", [1.0, 2.0])
@pytest.mark.parametrize("blank_last", [False, True])
@pytest.mark.parametrize("mode", ["full", "collapsed"])
@pytest.mark.parametrize("C", [8, 37])
def test_restatement_agrees_with_torch_autograd(C, mode, blank_last, tau, sym_is_blank):
    import kd_cases as K
    import kd_restatement as R
    x, y, sym, blank = K.logits_pair(C, blank_last, mode == "collapsed")
    if sym_is_blank:
        sym = sym.copy()
        sym[:, 1] = blank                  # a node whose correct symbol is the blank column has two classes
    rg = K.band_ranges()
    valid = R.valid_nodes(rg, K.BOUNDARY, K.S)
    assert (~valid[1, 9:]).all() and (~valid[1, :9]).any() and valid[0].all()   # invalid by frame AND by s > s_end
    loss, grad = R.kd_loss_and_grad(x, y, sym, rg, blank, K.BOUNDARY, mode, tau)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    lt = K.kd_loss_torch(xt, torch.from_numpy(y).double(), torch.from_numpy(sym), torch.from_numpy(rg), blank,
                         torch.from_numpy(K.BOUNDARY), mode, tau)
    lt.sum().backward()
    assert loss.shape == (K.B,) and (loss > 0).all()
    assert np.abs(loss - lt.detach().numpy()).max() <= 1e-12 * np.abs(loss).max()
    assert np.abs(grad - xt.grad.numpy()).max() <= 1e-12
    assert (grad[~valid] == 0).all() and (grad[valid].any(axis=-1)).all()


def test_restatement_edge_values():
    import kd_cases as K
    import kd_restatement as R
    x, y, sym, blank = K.logits_pair(8, False, False)
    rg = K.band_ranges()
    base = R.kd_loss_and_grad(x, y, sym, rg, blank, K.BOUNDARY)[0]
    for mode in ("full", "collapsed"):
        l0, g0 = R.kd_loss_and_grad(x, x, sym, rg, blank, K.BOUNDARY, mode)          # teacher = student
        assert np.abs(l0).max() <= 1e-12 and np.abs(g0).max() <= 1e-12
        xp, yp = x.copy(), y.copy()                                                   # invalid rows hold NaN: no effect
        bad = ~R.valid_nodes(rg, K.BOUNDARY, K.S)
        xp[bad] = np.nan
        yp[bad] = np.nan
        a, b = R.kd_loss_and_grad(x, y, sym, rg, blank, K.BOUNDARY, mode), R.kd_loss_and_grad(xp, yp, sym, rg, blank, K.BOUNDARY, mode)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    y0 = y.copy()
    y0[0, 0, 0, 5] = -np.inf                                                          # teacher mass 0: the term is 0
    assert np.isfinite(R.kd_loss_and_grad(x, y0, sym, rg, blank, K.BOUNDARY)[0]).all()
    x0 = x.copy()
    x0[0, 0, 0, 5] = -np.inf                                                          # student -inf under teacher mass: +inf
    l = R.kd_loss_and_grad(x0, y, sym, rg, blank, K.BOUNDARY)[0]
    assert l[0] == np.inf and l[1] == base[1]
    x0[0, 0, 0, 5] = np.nan
    l = R.kd_loss_and_grad(x0, y, sym, rg, blank, K.BOUNDARY)[0]
    assert np.isnan(l[0]) and l[1] == base[1]
    assert np.array_equal(R.kd_loss_and_grad(x, y, sym, rg, blank, None)[0] > base, [False, True])   # no boundary: more nodes


# ---- the C ABI

def test_entries_are_declared_exported_and_bound(ft):
    handle = ctypes.CDLL(ft._lib.LIB_PATH)
    declared = set(re.findall(r"\b(ftr_\w+)\s*\(", _header()))
    assert declared == set(ENTRIES) == set(ft._lib.KD_SYMBOLS)
    assert not set(ft._lib.KD_SYMBOLS) & (set(ft._lib.EXPORTED_SYMBOLS) | set(ft._lib.LOWP_SYMBOLS))
    for name in ENTRIES:
        params = _prototype(name)
        assert hasattr(handle, name), f"{name} is not exported by libftr_hip.so"
        assert len(ft._lib._KD_SIGNATURES[name][1]) == len(params), name
        assert params[-1] == ("void*", "stream"), name
    for name in ENTRIES[:2]:
        assert _prototype(name)[:4] == [("const void*", "logits"), ("int", "kind"), ("const void*", "teacher_logits"),
                                        ("int", "teacher_kind")], name
    assert ("void*", "glogits") in _prototype("ftr_pruned_kd_bwd_scaled_dt")
    assert '#include "ftr_lowp.h"' in open(HEADER).read()
    for name, value in (("FTR_KD_FULL", 0), ("FTR_KD_COLLAPSED", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), _header()) and getattr(ft._lib, name) == value
    L = ft._lib.lib()
    assert L.ftr_abi_version() == 133 and L.ftr_package_version() == b"1.2"


def test_header_is_plain_c():
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    subprocess.check_call(["gcc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", HEADER])
    subprocess.check_call(["g++", "-x", "c++", "-Wall", "-Werror", "-fsyntax-only", HEADER])


@pytest.mark.parametrize("name", ENTRIES[:2])
def test_kind_mode_and_temperature_are_refused_first(ft, name):
    for over, words in ((dict(kind=7), ("7", "element type")), (dict(teacher_kind=9), ("9", "element type")),
                        (dict(mode=2), ("2", "mode")), (dict(temperature=0.0), ("temperature",)),
                        (dict(temperature=float("nan")), ("temperature",)), (dict(temperature=float("inf")), ("temperature",))):
        rc, msg = _call(ft, name, **over)
        assert rc == 0 and all(w in msg for w in words), (over, rc, msg)            # FTR_ERR_INVALID_ARG
        # ... before a bad size, a bad termination symbol and the null pointers that every one of these calls has
        assert _call(ft, name, B=-1, termination_symbol=-1, **over) == (rc, msg)
        assert _call(ft, name, B=0, **over) == (rc, msg)
    for kind in (0, 1, 2):
        for teacher_kind in (0, 1, 2):
            for mode in (0, 1):
                rc, msg = _call(ft, name, kind=kind, teacher_kind=teacher_kind, mode=mode)
                assert rc == 0 and msg.endswith("null pointer"), (rc, msg)
                assert _call(ft, name, kind=kind, teacher_kind=teacher_kind, mode=mode, B=0)[0] == 1   # FTR_OK, nothing to do
    assert "bad sizes" in _call(ft, name, B=-1)[1] and "termination_symbol" in _call(ft, name, termination_symbol=10)[1]


def test_validation_replies_are_the_recorded_ones(ft):
    golden = json.load(open(GOLDEN))
    got = _replies(ft)
    assert set(got) == set(golden) == set(ENTRIES)
    for name in ENTRIES:
        assert set(got[name]) == set(golden[name]), name
        for label, reply in golden[name].items():
            assert reply[0] in (0, 1), (name, label)     # no recorded case got past validation
            assert got[name][label] == reply, (name, label, got[name][label], reply)


# ---- the Python function, as far as it goes without a device

def test_python_argument_errors(ft):
    import inspect
    assert list(inspect.signature(ft.rnnt_kd_loss_pruned).parameters) == [
        "logits", "teacher_logits", "symbols", "ranges", "termination_symbol", "boundary", "mode", "temperature", "reduction"]
    d = {k: v.default for k, v in inspect.signature(ft.rnnt_kd_loss_pruned).parameters.items()}
    assert (d["boundary"], d["mode"], d["temperature"], d["reduction"]) == (None, "full", 1.0, "mean")
    assert "temperature ** 2" in ft.rnnt_kd_loss_pruned.__doc__
    x = torch.zeros(2, 4, 2, 8)
    sym, rg = torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 4, 2, dtype=torch.int32)
    f = ft.rnnt_kd_loss_pruned
    for bad in (x.double(), x.to(torch.int32)):
        with pytest.raises(TypeError):
            f(bad, x, sym, rg, 0)
        with pytest.raises(TypeError):
            f(x, bad, sym, rg, 0)
    with pytest.raises(TypeError):
        f(x.to(torch.bfloat16), x.double(), sym, rg, 0)
    for teacher in (x[:, :, :, :4], x[:1], x[0]):
        with pytest.raises(ValueError):
            f(x, teacher, sym, rg, 0)
    with pytest.raises(ValueError):
        f(x[0], x[0], sym, rg, 0)
    with pytest.raises(ValueError, match="mode"):
        f(x, x, sym, rg, 0, mode="partial")
    for tau in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            f(x, x, sym, rg, 0, temperature=tau)
    with pytest.raises(ValueError, match="reduction"):
        f(x, x, sym, rg, 0, reduction="avg")
    with pytest.raises(ValueError, match="termination_symbol"):
        f(x, x, sym, rg, 8)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):      # valid arguments, no device: no quiet fall-back
            f(x, x, sym, rg, 0)


if __name__ == "__main__":
    sys.path[:0] = [os.path.join(ROOT, "tf-fast-rnnt_amd"), os.path.join(ROOT, "tests")]
    import tf_fast_rnnt as ft
    rec = _replies(ft)
    bad = {(n, c): v for n in rec for c, v in rec[n].items() if v[0] not in (0, 1)}
    assert not bad, f"cases that got past validation: {bad}"
    with open(GOLDEN, "w") as fh:   # one entry point per line
        fh.write("{\n" + ",\n".join(f"{json.dumps(n)}:{json.dumps(rec[n], separators=(',', ':'))}" for n in rec) + "\n}\n")
    print(f"{sum(len(v) for v in rec.values())} cases from {ft._lib.LIB_PATH} -> {GOLDEN}")
