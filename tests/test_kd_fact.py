"""Factored knowledge distillation on the pruned band (rnnt_kd_loss_pruned_factored), everything that needs no device: the
float64 restatement of the definition (tests/kd_fact_restatement.py) against an independent torch composition with autograd
and, for the softmax form without weights, against tests/kd_restatement.py; the two entries of include/ftr_kd_fact.h
(declared there only, exported, bound, validated in the documented order, their replies recorded in
tests/golden/kd_fact_capi_messages.json); and the argument errors of the Python function.

    python tests/test_kd_fact.py        records tests/golden/kd_fact_capi_messages.json from the library as built"""
import ctypes
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kd_fact_capi_messages.json")
HEADER = os.path.join(ROOT, "include", "ftr_kd_fact.h")
ENTRIES = ("ftr_pruned_kd_fact_fwd_dt", "ftr_pruned_kd_fact_bwd_scaled_dt")
FACT_DEFAULTS = dict(teacher_kind=0, mode=0, factorization=0, n_dur=0, dur_weight=1.0)
# on top of the table of tests/test_capi_messages.py: the checks these entries add, alone and against what answers later
FACT_EXTRA = [dict(teacher_kind=7), dict(mode=2), dict(temperature=0.0), dict(temperature=float("nan")),
              dict(factorization=3), dict(factorization=-1), dict(factorization=3, mode=2), dict(factorization=3, B=-1),
              dict(factorization=3, B=0), dict(factorization=1), dict(factorization=2), dict(factorization=2, n_dur=0),
              dict(factorization=2, n_dur=6), dict(factorization=2, n_dur=4), dict(factorization=2, n_dur=5, mode=1),
              dict(factorization=0, n_dur=1), dict(factorization=1, n_dur=2), dict(factorization=2, n_dur=10),
              dict(factorization=2, n_dur=4, C=4), dict(factorization=2, n_dur=4, C=5),
              dict(factorization=2, n_dur=4, dur_weight=-1.0), dict(factorization=2, n_dur=4, dur_weight=float("inf")),
              dict(factorization=2, n_dur=4, dur_weight=float("nan")), dict(factorization=2, n_dur=4, dur_weight=0.0),
              dict(factorization=2, n_dur=4, dur_weight=-1.0, B=-1), dict(factorization=2, n_dur=6, B=0),
              dict(factorization=1, dur_weight=-1.0), dict(factorization=2, n_dur=4, termination_symbol=6),
              dict(factorization=2, n_dur=4, termination_symbol=5), dict(factorization=1, C=1), dict(factorization=1, C=1, B=-1),
              dict(factorization=1, C=1, termination_symbol=5), dict(factorization=1, C=2, termination_symbol=1),
              dict(factorization=1, C=1, B=0), dict(factorization=2, n_dur=4, scale_stride=2)]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _prototype(name):
    m = re.search(r"\b%s\s*\(([^()]*)\)\s*;" % name, _header())
    assert m, f"{name} is not declared in include/ftr_kd_fact.h"
    out = []
    for p in m.group(1).split(","):
        typ, par = re.match(r"(.*?)(\w+)$", " ".join(p.split())).groups()
        out.append((typ.strip(), par))
    return out


def _call(ft, name, **over):
    """The entry with every pointer NULL and small valid sizes, `over` on top (by parameter name)"""
    import test_capi_messages as tcm
    values = {**tcm.DEFAULTS, **FACT_DEFAULTS, **over}
    args = []
    for (typ, par), at in zip(_prototype(name), ft._lib._KD_FACT_SIGNATURES[name][1]):
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
        for over in [dict()] + [c for c in tcm.SINGLES + tcm.ARRAYS + FACT_EXTRA if set(c) <= names]:
            label = ",".join(f"{k}={over[k]}" for k in over).replace(" ", "") or "default"
            got.setdefault(name, {})[label] = list(_call(ft, name, **over))
    return got


# ---- the definition

CASES = [("softmax", 9, 0), ("softmax", 37, 0), ("hat", 9, 0), ("hat", 37, 0), ("hat", 2, 0), ("tdt", 12, 4), ("tdt", 41, 5),
         ("tdt", 4, 1)]


def _sym_blank(K, W, N, blank_last, sym_is_blank):
    if W - N < 3:                               # too few token columns for symbols_for: every symbol is column W - N - 1 or 0
        blank = W - N - 1 if blank_last else 0
        sym = np.full((K.B, K.S), (W - N - 1) - blank, np.int32)
    else:
        sym, blank = K.symbols_for(W - N, blank_last, 17 * W + N)
    if sym_is_blank:
        sym = sym.copy()
        sym[:, 1] = blank                       # a node whose correct symbol is the blank column has one class fewer
    return sym, blank


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("sym_is_blank", [False, True])
@pytest.mark.parametrize("tau,dw", [(1.0, 1.0), (2.0, 0.3)])
@pytest.mark.parametrize("blank_last", [False, True])
@pytest.mark.parametrize("mode", ["full", "collapsed"])
@pytest.mark.parametrize("fact,W,N", CASES)
def test_restatement_agrees_with_torch_autograd(fact, W, N, mode, blank_last, tau, dw, sym_is_blank, weighted):
    import kd_fact_cases as K
    import kd_fact_restatement as R
    from kd_restatement import valid_nodes
    rng = np.random.default_rng(100 * W + N)
    x, y = 3.0 * rng.standard_normal((2, K.B, K.T, K.R, W))
    sym, blank = _sym_blank(K, W, N, blank_last, sym_is_blank)
    rg = K.band_ranges()
    w = K.node_weights(zeros=0.2) if weighted else None
    valid = valid_nodes(rg, K.BOUNDARY, K.S)
    assert (~valid[1, 4:]).all() and (~valid[1, :4]).any() and valid[0].all()   # invalid by frame AND by s > s_end
    if weighted:
        assert (w[valid] == 0).any() and (w[valid] != 0).any()
        valid = valid & (w != 0)
    loss, grad = R.kd_fact_loss_and_grad(x, y, sym, rg, blank, K.BOUNDARY, fact, N, mode, tau, dw, w)
    xt = torch.from_numpy(x).requires_grad_(True)
    lt = K.kd_fact_loss_torch(xt, torch.from_numpy(y), torch.from_numpy(sym), torch.from_numpy(rg), blank,
                              torch.from_numpy(K.BOUNDARY), fact, N, mode, tau, dw, None if w is None else torch.from_numpy(w))
    lt.sum().backward()
    assert loss.shape == (K.B,) and (loss > 0).all()
    assert np.abs(loss - lt.detach().numpy()).max() <= 1e-12 * np.abs(loss).max()
    assert np.abs(grad - xt.grad.numpy()).max() <= 1e-12
    assert (grad[~valid] == 0).all()
    assert (grad[valid].any(axis=-1)).all()
    if fact == "tdt":
        assert N == 1 or (grad[valid][:, W - N:] != 0).any(axis=-1).all()    # a head of one column is constant
        np.testing.assert_allclose(grad[valid][:, W - N:].sum(-1), 0, atol=1e-12)    # each head's gradient sums to 0
        np.testing.assert_allclose(grad[valid][:, :W - N].sum(-1), 0, atol=1e-12)


@pytest.mark.parametrize("mode", ["full", "collapsed"])
@pytest.mark.parametrize("C", [8, 37])
def test_softmax_without_weights_is_the_kd_restatement(C, mode):
    import kd_cases as K0
    import kd_fact_restatement as R
    import kd_restatement as R0
    x, y, sym, blank = K0.logits_pair(C, True, mode == "collapsed")
    rg = K0.band_ranges()
    for tau in (1.0, 2.0):
        a = R0.kd_loss_and_grad(x, y, sym, rg, blank, K0.BOUNDARY, mode, tau)
        b = R.kd_fact_loss_and_grad(x, y, sym, rg, blank, K0.BOUNDARY, "softmax", 0, mode, tau)
        assert np.abs(a[0] - b[0]).max() <= 1e-12 * np.abs(a[0]).max() and np.abs(a[1] - b[1]).max() <= 1e-12
        ones = np.ones(rg.shape, np.float32)
        c = R.kd_fact_loss_and_grad(x, y, sym, rg, blank, K0.BOUNDARY, "softmax", 0, mode, tau, node_weights=ones)
        assert np.array_equal(b[0], c[0]) and np.array_equal(b[1], c[1])


def test_tdt_full_is_the_kl_of_the_joint_distribution():
    import kd_fact_cases as K
    import kd_fact_restatement as R
    from kd_restatement import valid_nodes
    x, y, sym, blank = K.logits_pair(12, 4, False, False)
    rg = K.band_ranges()
    loss, _ = R.kd_fact_loss_and_grad(x, y, sym, rg, blank, K.BOUNDARY, "tdt", 4, "full", 2.0, 1.0)
    valid = torch.from_numpy(valid_nodes(rg, K.BOUNDARY, K.S))
    joint = K.joint_tdt_kl_torch(torch.from_numpy(x).double(), torch.from_numpy(y).double(), 4, 2.0, valid).numpy()
    assert np.abs(loss - joint).max() <= 1e-12 * np.abs(loss).max()


def test_restatement_edge_values():
    import kd_fact_cases as K
    import kd_fact_restatement as R
    from kd_restatement import valid_nodes
    rg = K.band_ranges()
    bad = ~valid_nodes(rg, K.BOUNDARY, K.S)
    for fact, W, N in (("softmax", 9, 0), ("hat", 9, 0), ("tdt", 12, 4)):
        for mode in ("full", "collapsed"):
            x, y, sym, blank = K.logits_pair(W, N, False, mode == "collapsed")
            f = lambda x, y, **kw: R.kd_fact_loss_and_grad(x, y, sym, rg, blank, K.BOUNDARY, fact, N, mode, **kw)
            base = f(x, y)
            l0, g0 = f(x, x)                                                   # teacher = student
            assert np.abs(l0).max() <= 1e-12 and np.abs(g0).max() <= 1e-12
            xp, yp = x.copy(), y.copy()                                        # invalid rows hold NaN: no effect
            xp[bad] = np.nan
            yp[bad] = np.nan
            got = f(xp, yp)
            assert np.array_equal(base[0], got[0]) and np.array_equal(base[1], got[1])
            w = K.node_weights(zeros=0.3)                                      # ... and so do rows of weight 0
            xp, yp = x.copy(), y.copy()
            xp[w == 0] = np.nan
            yp[w == 0] = np.nan
            a, b = f(x, y, node_weights=w), f(xp, yp, node_weights=w)
            assert np.isfinite(b[0]).all() and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            assert (b[1][w == 0] == 0).all() and (a[0] != base[0]).all()
            w2 = np.full(rg.shape, 2.0, np.float32)                            # a constant weight scales both
            c = f(x, y, node_weights=w2)
            np.testing.assert_allclose(c[0], 2 * base[0], rtol=1e-14)
            np.testing.assert_allclose(c[1], 2 * base[1], rtol=1e-14)
            wn = np.ones(rg.shape, np.float32)
            wn[0, 0, 0] = np.nan                                               # a NaN weight on a valid node
            ln = f(x, y, node_weights=wn)[0]
            assert np.isnan(ln[0]) and ln[1] == base[0][1]
            x0 = x.copy()
            x0[0, 0, 0, 1 if blank == 0 else 0] = np.nan                       # NaN in a valid row
            ln = f(x0, y)[0]
            assert np.isnan(ln[0]) and ln[1] == base[0][1]
    x, y, sym, blank = K.logits_pair(12, 4, False, False)                      # duration_weight 0: the head is not there
    l, g = R.kd_fact_loss_and_grad(x, y, sym, rg, blank, K.BOUNDARY, "tdt", 4, "full", 1.0, 0.0)
    l8, g8 = R.kd_fact_loss_and_grad(x[..., :8], y[..., :8], sym, rg, blank, K.BOUNDARY, "softmax", 0, "full", 1.0)
    assert np.array_equal(l, l8) and np.array_equal(g[..., :8], g8) and (g[..., 8:] == 0).all()
    xp = x.copy()
    xp[..., 8:] = np.nan
    assert np.array_equal(R.kd_fact_loss_and_grad(xp, y, sym, rg, blank, K.BOUNDARY, "tdt", 4, "full", 1.0, 0.0)[0], l)


# ---- the C ABI

def test_entries_are_declared_exported_and_bound(ft):
    handle = ctypes.CDLL(ft._lib.LIB_PATH)
    declared = set(re.findall(r"\b(ftr_\w+)\s*\(", _header()))
    assert declared == set(ENTRIES) == set(ft._lib.KD_FACT_SYMBOLS)
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):           # declared in the new header only
        if other != "ftr_kd_fact.h":
            text = open(os.path.join(ROOT, "include", other)).read()
            assert not any(name in text for name in ENTRIES), other
    tables = [n for n in dir(ft._lib) if n.endswith("_SYMBOLS") and n != "KD_FACT_SYMBOLS"]
    assert {"EXPORTED_SYMBOLS", "LOWP_SYMBOLS", "KD_SYMBOLS", "TDT_MIX_SYMBOLS"} <= set(tables)
    for table in tables:
        assert not set(ft._lib.KD_FACT_SYMBOLS) & set(getattr(ft._lib, table)), table
    for name, kd in zip(ENTRIES, ("ftr_pruned_kd_fwd_dt", "ftr_pruned_kd_bwd_scaled_dt")):
        params = _prototype(name)
        assert hasattr(handle, name), f"{name} is not exported by libftr_hip.so"
        assert len(ft._lib._KD_FACT_SIGNATURES[name][1]) == len(params), name
        assert params[-1] == ("void*", "stream"), name
        # the argument list of its ftr_kd.h counterpart, the four new arguments, the stream
        import test_kd
        assert params[:-5] == test_kd._prototype(kd)[:-1], name
        assert params[-5:-1] == [("int", "factorization"), ("int", "n_dur"), ("float", "dur_weight"), ("const float*", "node_weights")]
    assert '#include "ftr_kd.h"' in open(HEADER).read()
    for name, value in (("FTR_KD_FACT_SOFTMAX", 0), ("FTR_KD_FACT_HAT", 1), ("FTR_KD_FACT_TDT", 2), ("FTR_KD_FACT_MAX_DUR", 5)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), _header()) and getattr(ft._lib, name) == value
    L = ft._lib.lib()
    assert L.ftr_abi_version() == 133 and L.ftr_package_version() == b"1.2"


def test_header_is_plain_c_and_states_the_saved_planes():
    import shutil
    import subprocess
    text = " ".join(open(HEADER).read().split())
    for fact, mode, planes in (("SOFTMAX", "FULL", 2), ("SOFTMAX", "COLLAPSED", 4), ("HAT", "FULL", 2), ("HAT", "COLLAPSED", 4),
                               ("TDT", "FULL", 4), ("TDT", "COLLAPSED", 6)):
        assert re.search(r"%s %s %d:" % (fact, mode, planes), text), (fact, mode)
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    subprocess.check_call(["gcc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", HEADER])
    subprocess.check_call(["g++", "-x", "c++", "-Wall", "-Werror", "-fsyntax-only", HEADER])


@pytest.mark.parametrize("name", ENTRIES)
def test_head_is_refused_first(ft, name):
    tdt = dict(factorization=2, n_dur=4)
    for over, words in ((dict(kind=7), ("7", "element type")), (dict(teacher_kind=9), ("9", "element type")),
                        (dict(mode=2), ("2", "mode")), (dict(temperature=0.0), ("temperature",)),
                        (dict(temperature=float("nan")), ("temperature",)), (dict(factorization=3), ("3", "factorization")),
                        (dict(factorization=-1), ("-1", "factorization")), (dict(n_dur=1), ("n_dur",)),
                        (dict(factorization=1, n_dur=1), ("n_dur",)), (dict(factorization=2), ("n_dur",)),
                        (dict(factorization=2, n_dur=6), ("n_dur", "6")), (dict(factorization=2, n_dur=4, C=4), ("n_dur", "C = 4")),
                        (dict(dur_weight=-0.5, **tdt), ("dur_weight",)), (dict(dur_weight=float("inf"), **tdt), ("dur_weight",)),
                        (dict(dur_weight=float("nan"), **tdt), ("dur_weight",))):
        rc, msg = _call(ft, name, **over)
        assert rc == 0 and all(w in msg for w in words), (over, rc, msg)            # FTR_ERR_INVALID_ARG
        # ... before a bad size, a bad termination symbol and the null pointers that every one of these calls has
        assert _call(ft, name, **{"B": -1, "termination_symbol": -1, **over}) == (rc, msg)
        assert _call(ft, name, **{"B": 0, **over}) == (rc, msg)
    # kind / mode / temperature answer before the factorization, as they do in ftr_kd.h
    assert "mode" in _call(ft, name, mode=2, factorization=3)[1] and "temperature" in _call(ft, name, temperature=0.0, n_dur=1)[1]
    for fact, n_dur in ((0, 0), (1, 0), (2, 1), (2, 5)):
        for kind in (0, 1, 2):
            for teacher_kind in (0, 1, 2):
                for mode in (0, 1):
                    over = dict(kind=kind, teacher_kind=teacher_kind, mode=mode, factorization=fact, n_dur=n_dur)
                    rc, msg = _call(ft, name, **over)
                    assert rc == 0 and msg.endswith("null pointer"), (rc, msg)
                    assert _call(ft, name, B=0, **over)[0] == 1   # FTR_OK, nothing to do
    # then the order of ftr_kd.h: sizes (HAT's C >= 2 with them), the termination symbol against the token columns
    assert "bad sizes" in _call(ft, name, B=-1)[1] and "termination_symbol" in _call(ft, name, termination_symbol=10)[1]
    assert "HAT" in _call(ft, name, factorization=1, C=1)[1] and "HAT" in _call(ft, name, factorization=1, C=1, termination_symbol=5)[1]
    assert "bad sizes" in _call(ft, name, factorization=1, C=1, B=-1)[1]
    assert _call(ft, name, termination_symbol=5, **tdt)[1].endswith("null pointer")        # C = 10: six token columns
    assert "termination_symbol" in _call(ft, name, termination_symbol=6, **tdt)[1]
    assert _call(ft, name, dur_weight=0.0, **tdt)[1].endswith("null pointer") and _call(ft, name, dur_weight=-1.0)[1].endswith("null pointer")


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

def test_python_signature_and_argument_errors(ft):
    assert "rnnt_kd_loss_pruned_factored" in dir(ft)
    f = ft.rnnt_kd_loss_pruned_factored
    sig = inspect.signature(f).parameters
    assert list(sig) == ["logits", "teacher_logits", "symbols", "ranges", "termination_symbol", "boundary", "factorization",
                         "num_durations", "mode", "temperature", "duration_weight", "node_weights", "reduction"]
    d = {k: v.default for k, v in sig.items()}
    assert [d[k] for k in list(sig)[5:]] == [None, "softmax", 0, "full", 1.0, 1.0, None, "mean"]
    # rnnt_kd_loss_pruned is what it was
    assert list(inspect.signature(ft.rnnt_kd_loss_pruned).parameters) == [
        "logits", "teacher_logits", "symbols", "ranges", "termination_symbol", "boundary", "mode", "temperature", "reduction"]
    for word in ("torch.gather", "py_grad", "px_grad", "node_weights", "temperature ** 2"):
        assert word in f.__doc__, word
    x = torch.zeros(2, 4, 2, 8)
    sym, rg = torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 4, 2, dtype=torch.int32)
    for bad in (x.double(), x.to(torch.int32)):
        with pytest.raises(TypeError):
            f(bad, x, sym, rg, 0)
        with pytest.raises(TypeError):
            f(x, bad, sym, rg, 0)
    for teacher in (x[:, :, :, :4], x[:1], x[0]):
        with pytest.raises(ValueError):
            f(x, teacher, sym, rg, 0)
    with pytest.raises(ValueError):
        f(x[0], x[0], sym, rg, 0)
    with pytest.raises(ValueError, match="'softmax' \\| 'hat' \\| 'tdt'"):
        f(x, x, sym, rg, 0, factorization="multiblank")
    with pytest.raises(ValueError, match="mode"):
        f(x, x, sym, rg, 0, mode="partial")
    with pytest.raises(ValueError, match="factorization"):           # the order of the checks: factorization, then mode
        f(x, x, sym, rg, 0, factorization="x", mode="partial")
    for tau in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            f(x, x, sym, rg, 0, temperature=tau)
    for fact in ("softmax", "hat"):
        with pytest.raises(ValueError, match="num_durations"):
            f(x, x, sym, rg, 0, factorization=fact, num_durations=2)
    for n in (0, 6, -1, 8):
        with pytest.raises(ValueError, match="num_durations"):
            f(x, x, sym, rg, 0, factorization="tdt", num_durations=n)
    for dw in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="duration_weight"):
            f(x, x, sym, rg, 0, factorization="tdt", num_durations=2, duration_weight=dw)
    with pytest.raises(ValueError, match="hat"):
        f(x[..., :1], x[..., :1], sym, rg, 0, factorization="hat")
    with pytest.raises(ValueError, match="reduction"):
        f(x, x, sym, rg, 0, reduction="avg")
    with pytest.raises(ValueError, match="termination_symbol"):
        f(x, x, sym, rg, 8)
    with pytest.raises(ValueError, match=r"termination_symbol 6 not in \[0,6\)"):      # the token columns, not the row
        f(x, x, sym, rg, 6, factorization="tdt", num_durations=2)
    with pytest.raises(TypeError, match="node_weights"):
        f(x, x, sym, rg, 0, node_weights=torch.zeros(2, 4, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match="node_weights"):
        f(x, x, sym, rg, 0, node_weights=torch.zeros(2, 4, 3))
    if not torch.cuda.is_available():
        for kw in (dict(), dict(factorization="hat"), dict(factorization="tdt", num_durations=2), dict(node_weights=torch.ones(2, 4, 2))):
            with pytest.raises(RuntimeError, match="no CPU fallback"):      # valid arguments, no device: no quiet fall-back
                f(x, x, sym, rg, 0, **kw)


if __name__ == "__main__":
    sys.path[:0] = [os.path.join(ROOT, "tf-fast-rnnt_amd"), os.path.join(ROOT, "tests")]
    import tf_fast_rnnt as ft
    rec = _replies(ft)
    bad = {(n, c): v for n in rec for c, v in rec[n].items() if v[0] not in (0, 1)}
    assert not bad, f"cases that got past validation: {bad}"
    with open(GOLDEN, "w") as fh:   # one entry point per line
        fh.write("{\n" + ",\n".join(f"{json.dumps(n)}:{json.dumps(rec[n], separators=(',', ':'))}" for n in rec) + "\n}\n")
    print(f"{sum(len(v) for v in rec.values())} cases from {ft._lib.LIB_PATH} -> {GOLDEN}")
