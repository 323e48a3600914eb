"""The two entry points of include/ftr_band_constrained.h without a device: declared, exported and bound with matching
prototypes, and refused in the documented order (every pointer NULL, so no call gets as far as a launch)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ftr_band_constrained.h")
ENTRIES = ("ftr_pruned_band_constrained_fwd_dt", "ftr_pruned_band_constrained_bwd_scaled_dt")
OK, INVALID, UNSUPPORTED = 1, 0, -1


def _prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): [re.match(r"(.*?)(\w+)$", " ".join(p.split())).groups() for p in m.group(2).split(",")]
            for m in re.finditer(r"\b(ftr_\w+)\s*\(([^()]*)\)\s*;", text)}


def _call(ft, name, **over):
    values = dict(kind=0, flags=0, B=1, T=4, S=2, C=10, r=2, termination_symbol=0, scale_stride=0)
    values.update(over)
    args = [None if "*" in typ else 0.0 if at in (ctypes.c_float, ctypes.c_double) else int(values[par])
            for (typ, par), at in zip(_prototypes()[name], ft._lib._BAND_CONSTRAINED_SIGNATURES[name][1])]
    L = ft._lib.lib()
    return getattr(L, name)(*args), L.ftr_last_error().decode()


def test_entries_are_declared_exported_and_bound(ft):
    protos = _prototypes()
    assert set(protos) == set(ENTRIES) == set(ft._lib.BAND_CONSTRAINED_SYMBOLS)
    for name, params in protos.items():
        assert hasattr(ctypes.CDLL(ft._lib.LIB_PATH), name), f"{name} is not exported by libftr_hip.so"
        restype, argtypes = ft._lib._BAND_CONSTRAINED_SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params), name
        for (typ, par), at in zip(params, argtypes):
            want = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double}.get(typ.strip(), ctypes.c_void_p)
            assert at is want and (want is not ctypes.c_void_p or "*" in typ), (name, par)
        assert not any(name in getattr(ft._lib, t) for t in ("EXPORTED_SYMBOLS", "LOWP_SYMBOLS", "BAND_VITERBI_SYMBOLS")), name
    assert ft._lib.lib().ftr_abi_version() == 133


@pytest.mark.parametrize("name", ENTRIES)
def test_refusals_come_in_the_documented_order(ft, name):
    rc, msg = _call(ft, name, kind=7, B=-1, r=16, termination_symbol=-1)
    assert rc == INVALID and "element type" in msg and "7" in msg            # kind before everything
    rc, msg = _call(ft, name, T=0, r=16, S=20)
    assert rc == INVALID and "bad sizes" in msg                              # sizes before the domain of r
    rc, msg = _call(ft, name, flags=1, C=1, r=16)
    assert rc == INVALID and "HAT needs" in msg and msg.startswith("hat_")
    for over in (dict(r=16, S=20), dict(r=16, S=20, B=0), dict(r=16, S=20, scale_stride=2)):
        rc, msg = _call(ft, name, **over)
        assert rc == UNSUPPORTED and "r <= 15" in msg, over                  # r = 16 before scale_stride, B == 0 and the pointers
    rc, msg = _call(ft, name, scale_stride=2, B=0)
    assert (rc == INVALID and "scale_stride" in msg) if name.endswith("bwd_scaled_dt") else rc == OK
    assert _call(ft, name, B=0)[0] == OK                                     # nothing to do, before the pointers
    for over in (dict(), dict(r=15, S=20), dict(kind=1), dict(kind=2, flags=1)):
        rc, msg = _call(ft, name, **over)
        assert rc == INVALID and msg.endswith("null pointer"), over

