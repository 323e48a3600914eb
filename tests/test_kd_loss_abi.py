"""The entry points of include/ftr_kd_loss.h (the transducer loss on the pruned band and the distillation loss of ftr_kd.h in
one pass), checked without a device: they are declared, exported and bound with matching prototypes, their symbol table is
disjoint from every other one, the header parses as C99 and as C++ on its own, and their validation -- every device pointer
NULL, so no call gets as far as a launch -- answers in the order the header states.  Also the public signature of
rnnt_loss_pruned_kd and its refusals that need no device."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ftr_kd_loss.h")
FWD, BWD = "ftr_pruned_band_kd_fwd_dt", "ftr_pruned_band_kd_bwd_scaled_dt"
ENTRIES = (FWD, BWD)
DEFAULTS = dict(kind=0, teacher_kind=0, termination_symbol=0, temperature=1.0, mode=0, delay_penalty=0.0, modified=0, B=2, T=4,
                S=3, C=10, r=2, loss_scale_stride=0, loss_scale_mul=1.0, kd_scale_stride=1, kd_scale_mul=0.5)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _prototype(name):
    m = re.search(r"\b%s\s*\(([^()]*)\)\s*;" % name, _header())
    assert m, f"{name} is not declared in include/ftr_kd_loss.h"
    return [tuple(s.strip() for s in re.match(r"(.*?)(\w+)$", " ".join(p.split())).groups()) for p in m.group(1).split(",")]


def _call(ft, name, **over):
    """(return code, error text) of the entry with every pointer NULL and the other arguments from DEFAULTS / `over`"""
    vals = {**DEFAULTS, **over}
    args = [None if "*" in typ else vals[par] for typ, par in _prototype(name)]
    L = ft._lib.lib()
    rc = getattr(L, name)(*args)
    return rc, L.ftr_last_error().decode("utf-8", "replace")


def test_entries_are_declared_exported_and_bound(ft):
    handle = ctypes.CDLL(ft._lib.LIB_PATH)
    declared = set(re.findall(r"\b(ftr_\w+)\s*\(", _header()))
    assert declared == set(ENTRIES) == set(ft._lib.KD_LOSS_SYMBOLS)
    for name in ENTRIES:
        params = _prototype(name)
        restype, argtypes = ft._lib._KD_LOSS_SIGNATURES[name]
        assert hasattr(handle, name), f"{name} is not exported by libftr_hip.so"
        assert restype is ctypes.c_int and len(argtypes) == len(params), name
        for (typ, par), at in zip(params, argtypes):
            want = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double}.get(typ, ctypes.c_void_p)
            assert at is want and (want is not ctypes.c_void_p or "*" in typ), (name, par)
        assert params[-1] == ("void*", "stream"), name
    # the head of the ftr_kd.h entries, and two scale triples in the backward
    import test_kd
    for name, kd in zip(ENTRIES, ("ftr_pruned_kd_fwd_dt", "ftr_pruned_kd_bwd_scaled_dt")):
        assert _prototype(name)[:10] == test_kd._prototype(kd)[:10], name
    names = [par for _, par in _prototype(BWD)]
    assert names[names.index("loss_scale"):names.index("loss_scale") + 3] == ["loss_scale", "loss_scale_stride", "loss_scale_mul"]
    assert names[names.index("kd_scale"):names.index("kd_scale") + 3] == ["kd_scale", "kd_scale_stride", "kd_scale_mul"]
    assert '#include "ftr_kd.h"' in open(HEADER).read()
    L = ft._lib.lib()
    assert L.ftr_abi_version() == 133 and L.ftr_package_version() == b"1.2" and ft.__version__ == "1.2"


def test_symbol_table_is_disjoint_from_every_other_one(ft):
    tables = [n for n in dir(ft._lib) if n.endswith("_SYMBOLS") and n != "KD_LOSS_SYMBOLS"]
    assert {"EXPORTED_SYMBOLS", "LOWP_SYMBOLS", "KD_SYMBOLS", "KD_FACT_SYMBOLS", "TDT_MIX_SYMBOLS"} <= set(tables)
    for table in tables:
        assert not set(ft._lib.KD_LOSS_SYMBOLS) & set(getattr(ft._lib, table)), table
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):           # declared in the new header only
        if other != "ftr_kd_loss.h":
            text = open(os.path.join(ROOT, "include", other)).read()
            assert not any(name in text for name in ENTRIES), other


def test_header_is_plain_c():
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    subprocess.check_call(["gcc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", HEADER])
    subprocess.check_call(["g++", "-x", "c++", "-Wall", "-Werror", "-fsyntax-only", HEADER])


@pytest.mark.parametrize("name", ENTRIES)
def test_validation_order(ft, name):
    bwd = name == BWD
    # an unknown kind / teacher_kind / mode, or a bad temperature: before anything else is looked at
    for over, words in ((dict(kind=7), ("7", "element type")), (dict(teacher_kind=9), ("9", "element type")),
                        (dict(mode=2), ("2", "mode")), (dict(mode=-1), ("-1", "mode")), (dict(temperature=0.0), ("temperature",)),
                        (dict(temperature=-2.0), ("temperature",)), (dict(temperature=float("inf")), ("temperature",)),
                        (dict(temperature=float("nan")), ("temperature",))):
        rc, msg = _call(ft, name, **over)
        assert rc == 0 and all(w in msg for w in words) and msg.startswith(name[4:] + ":"), (over, rc, msg)   # FTR_ERR_INVALID_ARG
        assert _call(ft, name, **{"B": -1, "termination_symbol": -1, **over}) == (rc, msg)
        assert _call(ft, name, **{"B": 0, **over}) == (rc, msg)
        if bwd:
            assert _call(ft, name, **{"loss_scale_mul": float("nan"), "kd_scale_stride": 2, **over}) == (rc, msg)
    assert "element type" in _call(ft, name, kind=7, mode=2)[1] and "mode" in _call(ft, name, mode=2, temperature=0.0)[1]
    if bwd:   # then the two multipliers, which must be finite
        for over in (dict(loss_scale_mul=float("nan")), dict(kd_scale_mul=float("inf")), dict(kd_scale_mul=float("-inf"))):
            rc, msg = _call(ft, name, **over)
            assert rc == 0 and "finite" in msg, (over, rc, msg)
            assert _call(ft, name, **{"B": -1, "loss_scale_stride": 2, **over}) == (rc, msg)
            assert _call(ft, name, **{"B": 0, **over}) == (rc, msg)
    # then sizes, the termination symbol, the scale strides
    for over in (dict(B=-1), dict(T=0), dict(S=-1), dict(C=0), dict(r=0)):
        rc, msg = _call(ft, name, **over)
        assert rc == 0 and "bad sizes" in msg, (over, rc, msg)
        assert _call(ft, name, **{"termination_symbol": 10, **over}) == (rc, msg)
    for blank in (-1, 10):
        rc, msg = _call(ft, name, termination_symbol=blank)
        assert rc == 0 and "termination_symbol" in msg, (blank, rc, msg)
        assert _call(ft, name, termination_symbol=blank, B=0) == (rc, msg)
        if bwd:
            assert _call(ft, name, termination_symbol=blank, loss_scale_stride=2) == (rc, msg)
    if bwd:
        for over in (dict(loss_scale_stride=2), dict(kd_scale_stride=-1)):
            rc, msg = _call(ft, name, **over)
            assert rc == 0 and "scale_stride" in msg, (over, rc, msg)
            assert _call(ft, name, B=0, **over) == (rc, msg)
    # B == 0: nothing to do; otherwise the pointers (all NULL here), before the device
    for kind in (0, 1, 2):
        for teacher_kind in (0, 1, 2):
            for mode in (0, 1):
                over = dict(kind=kind, teacher_kind=teacher_kind, mode=mode)
                assert _call(ft, name, B=0, **over) == (1, "")                      # FTR_OK
                rc, msg = _call(ft, name, **over)
                assert rc == 0 and msg.endswith("null pointer"), (over, rc, msg)
    if bwd:   # an absent part: still the pointers of the other one
        for over in (dict(loss_scale_mul=0.0), dict(kd_scale_mul=0.0), dict(loss_scale_mul=0.0, kd_scale_mul=0.0)):
            assert _call(ft, name, **over)[1].endswith("null pointer") and _call(ft, name, B=0, **over)[0] == 1


def test_public_signature_and_docstring(ft):
    E = inspect.Parameter.empty
    sig = [(n, p.default) for n, p in inspect.signature(ft.rnnt_loss_pruned_kd).parameters.items()]
    assert sig == [("logits", E), ("teacher_logits", E), ("symbols", E), ("ranges", E), ("termination_symbol", E),
                   ("boundary", None), ("mode", "full"), ("temperature", 1.0), ("rnnt_type", "regular"), ("delay_penalty", 0.0),
                   ("reduction", "mean")]
    doc = " ".join(ft.rnnt_loss_pruned_kd.__doc__.split())
    for words in ("rnnt_loss_pruned(", "rnnt_kd_loss_pruned(", "constrained", "s_range >= 16", "stream capture", "never gets a gradient"):
        assert words in doc, words
    # the two functions it composes are what they were
    assert list(inspect.signature(ft.rnnt_kd_loss_pruned).parameters) == [
        "logits", "teacher_logits", "symbols", "ranges", "termination_symbol", "boundary", "mode", "temperature", "reduction"]
    assert list(inspect.signature(ft.rnnt_loss_pruned).parameters) == [
        "logits", "symbols", "ranges", "termination_symbol", "boundary", "rnnt_type", "delay_penalty", "reduction", "calc_gradients"]


def test_refusals_without_a_device(ft):
    x = torch.zeros(2, 4, 2, 8)
    sym = torch.zeros(2, 3, dtype=torch.int32)
    rg = torch.zeros(2, 4, 2, dtype=torch.int32)
    f = ft.rnnt_loss_pruned_kd
    with pytest.raises(ValueError, match="rnnt_type"):
        f(x, x, sym, rg, 0, rnnt_type="other")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(x, x, sym, rg, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(x.double(), x, sym, rg, 0)        # the device is asked for first, as rnnt_loss_pruned does
