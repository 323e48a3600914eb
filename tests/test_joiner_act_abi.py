"""The two entry points of include/ftr_joiner_act.h (the prune gather fused with the joiner's addition and its activation, and
the backward), checked without a device: they are declared, exported and bound, they are in no other header's table, an
unknown element type code is answered first and an unknown activation code second, and with known ones the replies are those
of ftr_do_pruning_f32 / ftr_do_pruning_bwd_ws_f32 on the same arguments.  Their replies over the applicable rows of the table
of tests/test_capi_messages.py, for both activations, are recorded once in tests/golden/joiner_act_capi_messages.json:

    python tests/test_joiner_act_abi.py        (writes the file; the library must be built)
"""
import ctypes
import json
import os
import shutil
import subprocess
import sys

import pytest

from test_prune_sum_abi import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ftr_joiner_act.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "joiner_act_capi_messages.json")
ENTRIES = ("ftr_pruned_joiner_act_dt", "ftr_pruned_joiner_act_bwd_ws_dt")
TWINS = {"ftr_pruned_joiner_act_dt": "ftr_do_pruning_f32", "ftr_pruned_joiner_act_bwd_ws_dt": "ftr_do_pruning_bwd_ws_f32"}
OTHER_TABLES = ("EXPORTED_SYMBOLS", "LOWP_SYMBOLS", "PRUNE_SUM_SYMBOLS", "KD_SYMBOLS", "FUSED_SYMBOLS", "BAND_TDT_SYMBOLS",
                "BAND_MULTIBLANK_SYMBOLS", "BAND_VITERBI_SYMBOLS")
ACTS = (1, 2)                      # FTR_ACT_TANH, FTR_ACT_RELU


def _call(L, ft, name, **over):
    """The entry (or its _f32 twin, of include/ftr.h) with every pointer NULL and the sizes of tests/test_capi_messages.py,
    `over` on top (by parameter name; act = FTR_ACT_TANH unless given); (return code, error text)."""
    import test_capi_messages as tcm
    if name in ENTRIES:
        params, argtypes = _prototypes(HEADER)[name], ft._lib._JOINER_ACT_SIGNATURES[name][1]
        over = dict({"act": 1}, **over)
    else:
        params, argtypes = _prototypes(os.path.join(ROOT, "include", "ftr.h"))[name], ft._lib._SIGNATURES[name][1]
    # (tcm.build_args, whose table of default sizes has no `act`: every pointer NULL, every integer from `over` or that table)
    args = [None if "*" in typ else int(over[par] if par in over else tcm.DEFAULTS[par]) for typ, par in params]
    assert len(args) == len(argtypes)
    rc = getattr(L, name)(*args)
    return rc, L.ftr_last_error().decode("utf-8", "replace")


def _replies(ft):
    import test_capi_messages as tcm
    L = ft._lib.lib()
    got = {}
    for name in ENTRIES:
        names = {par for _, par in _prototypes(HEADER)[name]}
        table = [dict(act=a, **c) for a in ACTS for c in [dict()] + [c for c in tcm.SINGLES if set(c) <= names]]
        table += [dict(act=0), dict(act=3), dict(act=3, B=-1), dict(act=3, kind=7)]
        for over in table:
            label = ",".join(f"{k}={over[k]}" for k in over).replace(" ", "")
            got.setdefault(name, {})[label] = list(_call(L, ft, name, **over))
    return got


def test_entries_are_declared_exported_and_bound(ft):
    protos = _prototypes(HEADER)
    handle = ctypes.CDLL(ft._lib.LIB_PATH)
    assert set(protos) == set(ENTRIES) == set(ft._lib.JOINER_ACT_SYMBOLS)
    for name, params in protos.items():
        restype, argtypes = ft._lib._JOINER_ACT_SIGNATURES[name]
        assert hasattr(handle, name), f"{name} is not exported by libftr_hip.so"
        assert restype is ctypes.c_int and len(argtypes) == len(params), name
        for (typ, par), at in zip(params, argtypes):
            if typ == "int":
                assert at is ctypes.c_int, (name, par)
            elif typ == "size_t":
                assert at is ctypes.c_size_t, (name, par)
            else:
                assert "*" in typ and at is ctypes.c_void_p, (name, par)
    assert [p for _, p in protos[ENTRIES[0]]] == ["am", "lm", "kind", "act", "ranges", "out", "B", "T", "S1", "C", "r", "stream"]
    assert [p for _, p in protos[ENTRIES[1]]] == ["g_out", "out", "kind", "act", "ranges", "d_am", "d_lm", "B", "T", "S1", "C", "r",
                                                  "workspace", "workspace_bytes", "stream"]
    text = open(HEADER).read()
    assert '#include "ftr_lowp.h"' in text                         # the FTR_DTYPE_* codes
    assert "#define FTR_ACT_TANH 1\n" in text and "#define FTR_ACT_RELU 2\n" in text
    assert (ft._lib.FTR_ACT_TANH, ft._lib.FTR_ACT_RELU) == ACTS
    L = ft._lib.lib()
    assert L.ftr_abi_version() == 133 and L.ftr_package_version() == b"1.2" and ft.__version__ == "1.2"
    assert callable(ft.do_rnnt_pruning_act)


def test_symbol_table_is_disjoint_from_every_other_one(ft):
    for table in OTHER_TABLES:
        assert not set(ft._lib.JOINER_ACT_SYMBOLS) & set(getattr(ft._lib, table)), table
    for header in os.listdir(os.path.join(ROOT, "include")):
        if header != "ftr_joiner_act.h":
            assert "pruned_joiner_act" not in open(os.path.join(ROOT, "include", header)).read(), header


@pytest.mark.parametrize("name", ENTRIES)
def test_unknown_dtype_then_unknown_activation_are_refused_before_a_bad_size(ft, name):
    L = ft._lib.lib()
    for bad in (7, -1):
        rc, msg = _call(L, ft, name, kind=bad)
        assert rc == 0 and msg and str(bad) in msg and "element type" in msg, (rc, msg)       # FTR_ERR_INVALID_ARG
        assert _call(L, ft, name, kind=bad, B=-1) == (rc, msg)                                 # ... a bad size besides: still the dtype reply
        assert _call(L, ft, name, kind=bad, act=9) == (rc, msg)                                # ... a bad activation besides: the dtype first
    for kind in (0, 1, 2):
        for bad in (0, 3, -1):
            rc, msg = _call(L, ft, name, kind=kind, act=bad)
            assert rc == 0 and str(bad) in msg and "activation" in msg, (rc, msg)
            assert _call(L, ft, name, kind=kind, act=bad, B=-1) == (rc, msg)
            assert _call(L, ft, name, kind=kind, act=bad, B=0) == (rc, msg)                    # not the early FTR_OK either


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("name", ENTRIES)
def test_known_codes_validate_as_the_f32_twin(ft, name, kind, act):
    """The null-pointer check (all sizes valid), the early FTR_OK of B == 0, a workspace of no bytes, and a bad size: code
    and text of the _f32 twin on the same arguments."""
    L = ft._lib.lib()
    twin = TWINS[name]
    rc, msg = _call(L, ft, name, kind=kind, act=act)
    assert rc == 0 and msg.endswith("null pointer"), (rc, msg)
    assert _call(L, ft, name, kind=kind, act=act, B=0)[0] == 1                        # FTR_OK, nothing to do
    for over in (dict(), dict(B=0), dict(workspace_bytes=0), dict(B=0, workspace_bytes=0), dict(B=-1), dict(S1=0), dict(C=0)):
        assert _call(L, ft, name, kind=kind, act=act, **over) == _call(L, ft, twin, **over), (name, kind, act, over)


def test_validation_replies_are_the_recorded_ones(ft):
    golden = json.load(open(GOLDEN))
    got = _replies(ft)
    assert set(got) == set(golden) == set(ENTRIES)
    for name in ENTRIES:
        assert set(got[name]) == set(golden[name]), name
        assert {"act=1", "act=2", "act=1,B=0", "act=2,B=-1", "act=1,kind=7", "act=2,S1=0", "act=1,C=0", "act=2,r=0", "act=0", "act=3",
                "act=3,B=-1", "act=3,kind=7"} <= set(golden[name]), name
        for label, reply in golden[name].items():
            assert reply[0] in (0, 1), (name, label)     # no recorded case got past validation
            assert got[name][label] == reply, (name, label, got[name][label], reply)
    assert "act=1,workspace_bytes=0" in golden[ENTRIES[1]]


def test_header_is_plain_c():
    """include/ftr_joiner_act.h parses as C99 and as C++ on its own, as include/ftr.h does (tests/test_capi_symbols.py)."""
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
