"""The two entry points of include/ftr_prune_sum.h (the prune gather fused with the joiner's first addition, and its
backward), checked without a device: they are declared, exported and bound, they are in no other header's table, an unknown
element type code is answered first, and with a known one the replies are those of ftr_do_pruning_f32 /
ftr_do_pruning_bwd_ws_f32 on the same arguments.  Their replies over the applicable rows of the table of
tests/test_capi_messages.py are recorded once in tests/golden/prune_sum_capi_messages.json:

    python tests/test_prune_sum_abi.py        (writes the file; the library must be built)
"""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ftr_prune_sum.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "prune_sum_capi_messages.json")
ENTRIES = ("ftr_do_pruning_sum_dt", "ftr_do_pruning_sum_bwd_ws_dt")
TWINS = {"ftr_do_pruning_sum_dt": "ftr_do_pruning_f32", "ftr_do_pruning_sum_bwd_ws_dt": "ftr_do_pruning_bwd_ws_f32"}
OTHER_TABLES = ("EXPORTED_SYMBOLS", "LOWP_SYMBOLS", "KD_SYMBOLS", "FUSED_SYMBOLS", "BAND_TDT_SYMBOLS", "BAND_MULTIBLANK_SYMBOLS",
                "BAND_VITERBI_SYMBOLS")


def _prototypes(path=HEADER):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(ftr_\w+)\s*\(([^()]*)\)\s*;", text):
        params = []
        for p in m.group(2).split(","):
            p = " ".join(p.split())
            if p and p != "void":
                typ, name = re.match(r"(.*?)(\w+)$", p).groups()
                params.append((typ.strip(), name))
        out[m.group(1)] = params
    return out


def _call(L, ft, name, **over):
    """The entry (or its _f32 twin, of include/ftr.h) with every pointer NULL and the sizes of tests/test_capi_messages.py,
    `over` on top (by parameter name); (return code, error text)."""
    import test_capi_messages as tcm
    if name in ENTRIES:
        params, argtypes = _prototypes()[name], ft._lib._PRUNE_SUM_SIGNATURES[name][1]
    else:
        params, argtypes = _prototypes(os.path.join(ROOT, "include", "ftr.h"))[name], ft._lib._SIGNATURES[name][1]
    args, _keep = tcm.build_args(params, argtypes, {k: v for k, v in over.items() if k in {p for _, p in params}})
    rc = getattr(L, name)(*args)
    return rc, L.ftr_last_error().decode("utf-8", "replace")


def _replies(ft):
    import test_capi_messages as tcm
    L = ft._lib.lib()
    got = {}
    for name in ENTRIES:
        params, argtypes = _prototypes()[name], ft._lib._PRUNE_SUM_SIGNATURES[name][1]
        names = {par for _, par in params}
        for over in [dict()] + [c for c in tcm.SINGLES if set(c) <= names]:
            label = ",".join(f"{k}={over[k]}" for k in over).replace(" ", "") or "default"
            args, _keep = tcm.build_args(params, argtypes, over)
            rc = getattr(L, name)(*args)
            got.setdefault(name, {})[label] = [rc, L.ftr_last_error().decode("utf-8", "replace")]
    return got


def test_entries_are_declared_exported_and_bound(ft):
    protos = _prototypes()
    handle = ctypes.CDLL(ft._lib.LIB_PATH)
    assert set(protos) == set(ENTRIES) == set(ft._lib.PRUNE_SUM_SYMBOLS)
    for name, params in protos.items():
        restype, argtypes = ft._lib._PRUNE_SUM_SIGNATURES[name]
        assert hasattr(handle, name), f"{name} is not exported by libftr_hip.so"
        assert restype is ctypes.c_int and len(argtypes) == len(params), name
        for (typ, par), at in zip(params, argtypes):
            if typ == "int":
                assert at is ctypes.c_int, (name, par)
            elif typ == "size_t":
                assert at is ctypes.c_size_t, (name, par)
            else:
                assert "*" in typ and at is ctypes.c_void_p, (name, par)
    assert [p for _, p in protos[ENTRIES[0]]] == ["am", "lm", "kind", "ranges", "out", "B", "T", "S1", "C", "r", "stream"]
    assert [p for _, p in protos[ENTRIES[1]]] == ["g_out", "kind", "ranges", "d_am", "d_lm", "B", "T", "S1", "C", "r", "workspace",
                                                  "workspace_bytes", "stream"]
    assert '#include "ftr_lowp.h"' in open(HEADER).read()          # the FTR_DTYPE_* codes
    L = ft._lib.lib()
    assert L.ftr_abi_version() == 133 and L.ftr_package_version() == b"1.2" and ft.__version__ == "1.2"
    assert callable(ft.do_rnnt_pruning_sum)


def test_symbol_table_is_disjoint_from_every_other_one(ft):
    for table in OTHER_TABLES:
        assert not set(ft._lib.PRUNE_SUM_SYMBOLS) & set(getattr(ft._lib, table)), table
    for header in os.listdir(os.path.join(ROOT, "include")):
        if header != "ftr_prune_sum.h":
            assert "do_pruning_sum" not in open(os.path.join(ROOT, "include", header)).read(), header


@pytest.mark.parametrize("name", ENTRIES)
def test_unknown_dtype_is_refused_before_anything_else(ft, name):
    L = ft._lib.lib()
    rc, msg = _call(L, ft, name, kind=7)
    assert rc == 0 and msg and "7" in msg and "element type" in msg, (rc, msg)       # FTR_ERR_INVALID_ARG
    assert _call(L, ft, name, kind=7, B=-1) == (rc, msg)                              # ... a bad size besides: still the dtype reply
    rc, msg = _call(L, ft, name, kind=-1)
    assert rc == 0 and "-1" in msg and "element type" in msg, (rc, msg)
    assert _call(L, ft, name, kind=-1, B=-1) == (rc, msg)


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("name", ENTRIES)
def test_known_dtypes_validate_as_the_f32_twin(ft, name, kind):
    """The null-pointer check (all sizes valid), the early FTR_OK of B == 0, a workspace of no bytes, and a bad size: code
    and text of the _f32 twin on the same arguments."""
    L = ft._lib.lib()
    twin = TWINS[name]
    rc, msg = _call(L, ft, name, kind=kind)
    assert rc == 0 and msg.endswith("null pointer"), (rc, msg)
    assert _call(L, ft, name, kind=kind, B=0)[0] == 1                                # FTR_OK, nothing to do
    for over in (dict(), dict(B=0), dict(workspace_bytes=0), dict(B=0, workspace_bytes=0), dict(B=-1), dict(S1=0), dict(C=0)):
        assert _call(L, ft, name, kind=kind, **over) == _call(L, ft, twin, **over), (name, kind, over)


def test_validation_replies_are_the_recorded_ones(ft):
    golden = json.load(open(GOLDEN))
    got = _replies(ft)
    assert set(got) == set(golden) == set(ENTRIES)
    for name in ENTRIES:
        assert set(got[name]) == set(golden[name]), name
        assert {"default", "B=0", "B=-1", "kind=7", "S1=0", "C=0", "r=0"} <= set(golden[name]), name
        for label, reply in golden[name].items():
            assert reply[0] in (0, 1), (name, label)     # no recorded case got past validation
            assert got[name][label] == reply, (name, label, got[name][label], reply)
    assert "workspace_bytes=0" in golden[ENTRIES[1]]


def test_header_is_plain_c():
    """include/ftr_prune_sum.h parses as C99 and as C++ on its own, as include/ftr.h does (tests/test_capi_symbols.py)."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    subprocess.check_call(["gcc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", HEADER])
    subprocess.check_call(["g++", "-x", "c++", "-Wall", "-Werror", "-fsyntax-only", HEADER])


if __name__ == "__main__":
    for p in (os.path.join(ROOT, "tf-fast-rnnt_amd"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import tf_fast_rnnt
    with open(GOLDEN, "w") as f:
        json.dump(_replies(tf_fast_rnnt), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
