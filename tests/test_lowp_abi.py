"""The 16-bit-logits entry points of the C ABI (the ftr_*_dt family of include/ftr_lowp.h), checked without a device: they
are declared, exported and bound, and an unknown element type code is answered with FTR_ERR_INVALID_ARG and a message
before anything else -- pointers, sizes, the device -- is looked at.

They live in a header of their own, on top of ftr.h: tests/test_capi_symbols.py and tests/test_capi_messages.py pin ftr.h
symbol for symbol against _lib.EXPORTED_SYMBOLS and against the replies recorded in tests/golden/capi_messages.json, so an
entry added to ftr.h would be one without a recorded reply.  The replies of these four are recorded, over the same table
of argument vectors, in tests/golden/lowp_capi_messages.json (test_validation_replies_are_the_recorded_ones below)."""
import ctypes
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ftr_pruned_logprobs_fwd_dt", "ftr_pruned_logprobs_bwd_scaled_dt", "ftr_pruned_band_fwd_dt",
           "ftr_pruned_band_bwd_scaled_dt")


GOLDEN = os.path.join(ROOT, "tests", "golden", "lowp_capi_messages.json")


def _header():
    return open(os.path.join(ROOT, "include", "ftr_lowp.h")).read()


def _prototype(name):
    """[(type, parameter name)] of one declaration of include/ftr_lowp.h (an _f32 twin: of include/ftr.h)"""
    text = _header() if name in ENTRIES else open(os.path.join(ROOT, "include", "ftr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b%s\s*\(([^()]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared"
    out = []
    for p in m.group(1).split(","):
        typ, par = re.match(r"(.*?)(\w+)$", " ".join(p.split())).groups()
        out.append((typ.strip(), par))
    return out


def _call(L, ft, name, **over):
    """The entry with every pointer NULL and small valid sizes, `over` on top (by parameter name)."""
    values = dict(kind=0, flags=0, B=1, T=4, S=2, C=10, r=2, modified=0, termination_symbol=0, scale_stride=0)
    values.update(over)
    args = []
    signatures = {**ft._lib._SIGNATURES, **ft._lib._LOWP_SIGNATURES}
    for (typ, par), at in zip(_prototype(name), signatures[name][1]):
        if "*" in typ:
            args.append(None)
        elif at in (ctypes.c_float, ctypes.c_double):
            args.append(1.0 if at is ctypes.c_float else 0.0)
        else:
            args.append(int(values[par]))
    return getattr(L, name)(*args), L.ftr_last_error().decode()


def test_entries_are_declared_exported_and_bound(ft):
    handle = ctypes.CDLL(ft._lib.LIB_PATH)
    for name in ENTRIES:
        params = _prototype(name)
        assert params[0] == ("const void*", "logits") and params[1] == ("int", "kind"), name
        assert params[-2:] == [("int", "flags"), ("void*", "stream")], name
        assert hasattr(handle, name), f"{name} is not exported by libftr_hip.so"
        assert name in ft._lib.LOWP_SYMBOLS and name not in ft._lib.EXPORTED_SYMBOLS
        assert len(ft._lib._LOWP_SIGNATURES[name][1]) == len(params), name
    for name in ("ftr_pruned_logprobs_bwd_scaled_dt", "ftr_pruned_band_bwd_scaled_dt"):
        assert ("void*", "glogits") in _prototype(name)
    assert set(ft._lib.LOWP_SYMBOLS) == set(re.findall(r"\b(ftr_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    assert '#include "ftr.h"' in _header()


def test_validation_replies_are_the_recorded_ones(ft):
    """tests/test_capi_messages.py for the four entries: its table of argument vectors (every pointer NULL), its way of
    calling, the replies recorded once in a golden file of their own."""
    import test_capi_messages as tcm
    golden = json.load(open(GOLDEN))
    L = ft._lib.lib()
    got = {}
    for name in ENTRIES:
        params, argtypes = _prototype(name), ft._lib._LOWP_SIGNATURES[name][1]
        names = {par for _, par in params}
        for over in [dict()] + [c for c in tcm.SINGLES + tcm.ARRAYS if set(c) <= names]:
            label = ",".join(f"{k}={over[k]}" for k in over).replace(" ", "") or "default"
            args, _keep = tcm.build_args(params, argtypes, over)
            rc = getattr(L, name)(*args)
            got.setdefault(name, {})[label] = [rc, L.ftr_last_error().decode("utf-8", "replace")]
    assert set(got) == set(golden) == set(ENTRIES)
    for name in ENTRIES:
        assert set(got[name]) == set(golden[name]), name
        for label, reply in golden[name].items():
            assert reply[0] in (0, 1), (name, label)     # no recorded case got past validation
            assert got[name][label] == reply, (name, label, got[name][label], reply)


def test_dtype_codes_are_named_in_the_header(ft):
    text = _header()
    for name, value in (("FTR_DTYPE_F32", 0), ("FTR_DTYPE_BF16", 1), ("FTR_DTYPE_FP16", 2), ("FTR_PRUNED_HAT", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
        assert getattr(ft._lib, name) == value


@pytest.mark.parametrize("name", ENTRIES)
def test_unknown_dtype_is_refused_before_the_device(ft, name):
    L = ft._lib.lib()
    rc, msg = _call(L, ft, name, kind=7)
    assert rc == 0 and msg and "7" in msg and "element type" in msg, (rc, msg)       # FTR_ERR_INVALID_ARG
    # ... before the other checks: a bad size and a bad termination symbol besides still get the dtype reply
    assert _call(L, ft, name, kind=7, B=-1, termination_symbol=-1) == (rc, msg)
    assert _call(L, ft, name, kind=-1)[0] == 0
    # unknown flag bits likewise
    rc, msg = _call(L, ft, name, flags=2)
    assert rc == 0 and "flags" in msg


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("name", ENTRIES)
def test_known_dtypes_validate_as_the_f32_twin(ft, name, kind):
    """With a known code the reply is that of the _f32 / ftr_hat_ twin on the same arguments: the null-pointer check
    (all sizes valid), the early FTR_OK of B == 0, HAT's C >= 2."""
    L = ft._lib.lib()
    rc, msg = _call(L, ft, name, kind=kind)
    assert rc == 0 and msg.endswith("null pointer"), (rc, msg)
    assert _call(L, ft, name, kind=kind, B=0)[0] == 1                               # FTR_OK, nothing to do
    rc, msg = _call(L, ft, name, kind=kind, flags=1, C=1)
    assert rc == 0 and "HAT needs" in msg and msg.startswith("hat_"), (rc, msg)
    twin = name[:-3] + "_f32"
    assert _call(L, ft, twin)[1] == _call(L, ft, name, kind=kind)[1]


def test_header_is_plain_c():
    """include/ftr_lowp.h parses as C99 and as C++ on its own, as include/ftr.h does (tests/test_capi_symbols.py)."""
    import shutil
    import subprocess
    hdr = os.path.join(ROOT, "include", "ftr_lowp.h")
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    subprocess.check_call(["gcc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", hdr])
    subprocess.check_call(["g++", "-x", "c++", "-Wall", "-Werror", "-fsyntax-only", hdr])
