"""The band-native multi-blank entry points of the C ABI (include/ftr_band_multiblank.h), checked without a device: they
are declared, exported and bound with matching prototypes, their symbol table is disjoint from the five other tables, the
builders take the argument lists of their lattice twins, the queries answer, and the validation replies -- for the argument
vectors of tests/test_capi_messages.py, every device pointer NULL, so no call gets as far as a launch -- are the ones
recorded in tests/golden/band_multiblank_capi_messages.json:

    python tests/test_band_multiblank_abi.py          (records the file from the library as built)
"""
import ctypes
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ftr_band_multiblank.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "band_multiblank_capi_messages.json")
QUERIES = ("ftr_mutual_information_band_multiblank_workspace_floats", "ftr_mutual_information_band_multiblank_supported")
ENTRIES = ("ftr_mutual_information_band_multiblank_f32", "ftr_multiblank_pruned_band_fwd_f32",
           "ftr_multiblank_pruned_band_bwd_scaled_f32")
LATTICE_TWIN = {"ftr_multiblank_pruned_band_fwd_f32": "ftr_multiblank_pruned_logprobs_fwd_f32",
                "ftr_multiblank_pruned_band_bwd_scaled_f32": "ftr_multiblank_pruned_logprobs_bwd_scaled_f32"}
# on top of the table of tests/test_capi_messages.py (which has durations (1,33), D = 9, D = 0, B = 0, workspace_floats = 0):
# what only these entries check
EXTRA_CASES = [dict(durations=(2, 2)), dict(durations=(1, 32)), dict(r=16, S=20), dict(r=15, S=20), dict(r=16, S=20, B=0),
               dict(T=0, r=16), dict(workspace_floats=0, r=16, S=20), dict(durations=(1, 2, 3, 4, 5, 6, 7, 8), D=8),
               dict(D=9, r=16, S=20), dict(durations=(1, 33), r=16, S=20)]


def _prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(ftr_\w+)\s*\(([^()]*)\)\s*;", text):
        params = []
        for p in m.group(2).split(","):
            typ, name = re.match(r"(.*?)(\w+)$", " ".join(p.split())).groups()
            params.append((typ.strip(), name))
        out[m.group(1)] = params
    return out


def _replies(ft):
    import test_capi_messages as tcm
    L = ft._lib.lib()
    got = {}
    for name in ENTRIES:
        params, argtypes = _prototypes()[name], ft._lib._BAND_MULTIBLANK_SIGNATURES[name][1]
        names = {par for _, par in params}
        for over in [dict()] + [c for c in tcm.SINGLES + tcm.ARRAYS + EXTRA_CASES if set(c) <= names]:
            label = ",".join(f"{k}={over[k]}" for k in over).replace(" ", "") or "default"
            args, _keep = tcm.build_args(params, argtypes, over)
            rc = getattr(L, name)(*args)
            got.setdefault(name, {})[label] = [rc, L.ftr_last_error().decode("utf-8", "replace")]
    return got


def test_entries_are_declared_exported_and_bound(ft):
    protos = _prototypes()
    handle = ctypes.CDLL(ft._lib.LIB_PATH)
    assert len(protos) == 5
    assert set(protos) == set(QUERIES) | set(ENTRIES) == set(ft._lib.BAND_MULTIBLANK_SYMBOLS)
    for name, params in protos.items():
        restype, argtypes = ft._lib._BAND_MULTIBLANK_SIGNATURES[name]
        assert hasattr(handle, name), f"{name} is not exported by libftr_hip.so"
        assert len(argtypes) == len(params), name
        for (typ, par), at in zip(params, argtypes):
            if typ == "int":
                assert at is ctypes.c_int, (name, par)
            elif typ == "size_t":
                assert at is ctypes.c_size_t, (name, par)
            elif typ == "float":
                assert at is ctypes.c_float, (name, par)
            elif typ == "double":
                assert at is ctypes.c_double, (name, par)
            elif par in ("durations", "big_blank_ids"):
                assert typ == "const int32_t*" and at == ctypes.POINTER(ctypes.c_int32), (name, par)   # host arrays
            else:
                assert "*" in typ and at is ctypes.c_void_p, (name, par)
        assert restype is (ctypes.c_size_t if name == QUERIES[0] else ctypes.c_int), name
    assert [p for _, p in protos[QUERIES[0]]] == ["B", "T", "S", "r", "D"]
    assert [p for _, p in protos[QUERIES[1]]] == ["T", "S", "r", "D"]
    assert [p for _, p in protos[ENTRIES[0]]] == ["px_band", "py_band", "ranges", "boundary", "durations", "D", "workspace",
                                                  "workspace_floats", "ans", "gx_band", "gy_band", "B", "T", "S", "r", "stream"]
    assert '#include "ftr.h"' in open(HEADER).read()
    assert ft._lib.lib().ftr_abi_version() == 133


def test_symbol_table_is_disjoint_from_the_other_five(ft):
    others = (set(ft._lib.EXPORTED_SYMBOLS) | set(ft._lib.LOWP_SYMBOLS) | set(ft._lib.KD_SYMBOLS) | set(ft._lib.FUSED_SYMBOLS)
              | set(ft._lib.BAND_TDT_SYMBOLS))
    assert not set(ft._lib.BAND_MULTIBLANK_SYMBOLS) & others
    for header in ("ftr.h", "ftr_lowp.h", "ftr_kd.h", "ftr_fused.h", "ftr_band_tdt.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert "band_multiblank" not in text and "multiblank_pruned_band" not in text, header


def test_band_builders_take_the_arguments_of_their_lattice_twins(ft):
    """Same parameter list up to the names of the lattice-shaped / band-shaped tensors, same ctypes signature."""
    import test_capi_messages as tcm
    ftr_h = tcm.prototypes()
    rename = {"px": "px_band", "py": "py_band", "gpx": "gx_band", "gpy": "gy_band"}
    for band, lattice in LATTICE_TWIN.items():
        want = [(t, rename.get(p, p)) for t, p in ftr_h[lattice]]
        assert _prototypes()[band] == want, band
        assert ft._lib._BAND_MULTIBLANK_SIGNATURES[band] == ft._lib._SIGNATURES[lattice], band


def test_queries_answer_without_a_device(ft):
    L = ft._lib.lib()
    sup, ws = L.ftr_mutual_information_band_multiblank_supported, L.ftr_mutual_information_band_multiblank_workspace_floats
    assert sup(40, 12, 4, 8) == 1 and sup(40, 12, 15, 1) == 1 and sup(1, 0, 1, 1) == 1
    for bad in ((40, 12, 16, 4), (40, 12, 0, 4), (0, 12, 4, 4), (40, -1, 4, 4), (40, 12, 4, 0), (40, 12, 4, 9)):
        assert sup(*bad) == 0 and ws(2, *bad) == 0, bad
    assert sup(2 ** 31 - 1, 2 ** 31 - 1, 4, 8) == 0            # the 32-bit slot-index rule
    # O((S + T) * lanes * (D + 1)) per utterance, nothing of size S * T: linear in B, at most doubling from 8 to 16 lanes
    base = ws(1, 1500, 300, 5, 4)
    assert 0 < base < 1500 * 300
    assert ws(3, 1500, 300, 5, 4) == 3 * base
    assert ws(1, 3000, 600, 5, 4) <= 2 * base + 4096
    assert base < ws(1, 1500, 300, 8, 4) <= 2 * base
    # the TDT entry keeps its own domain: six blank moves are the multi-blank entry's only
    assert L.ftr_mutual_information_band_tdt_supported(40, 12, 4, 1, 6) == 0 and sup(40, 12, 4, 6) == 1


def test_validation_replies_are_the_recorded_ones(ft):
    golden = json.load(open(GOLDEN))
    got = _replies(ft)
    assert set(got) == set(golden) == set(ENTRIES)
    for name in ENTRIES:
        assert set(got[name]) == set(golden[name]), name
        for label, reply in golden[name].items():
            # no recorded case got past validation: FTR_ERR_INVALID_ARG, an early FTR_OK, or FTR_ERR_UNSUPPORTED for the domain
            assert reply[0] in (0, 1, -1) and (reply[0] != -1 or "outside the kernel's domain" in reply[1]), (name, label)
            assert got[name][label] == reply, (name, label, got[name][label], reply)
    # what the header states about the order: D, the duration list, sizes, r, B == 0, the workspace, the pointers
    rec = golden["ftr_mutual_information_band_multiblank_f32"]
    assert rec["durations=(1,33)"][0] == 0 and "outside 1..32" in rec["durations=(1,33)"][1]
    assert rec["durations=(2,2)"][0] == 0 and "strictly increasing" in rec["durations=(2,2)"][1]
    assert rec["durations=(2,3)"][0] == 0 and "null" in rec["durations=(2,3)"][1]          # no 1 needed: as far as the pointers
    assert rec["durations=(1,32)"] == rec["default"] and "null" in rec["default"][1]
    assert rec["durations=(1,2,3,4,5,6,7,8,9),D=9"][0] == -1 and rec["D=0"][0] == -1 and rec["D=9,r=16,S=20"][0] == -1
    assert rec["durations=(1,2,3,4,5,6,7,8),D=8"] == rec["default"]
    assert rec["durations=(1,33),r=16,S=20"][0] == 0                                           # the list before the domain of r
    assert "bad sizes" in rec["T=0,r=16"][1]
    assert rec["r=16,S=20,B=0"][0] == -1 and rec["r=16,S=20"][0] == -1 and rec["r=15,S=20"][0] == 0 and rec["B=0"][0] == 1
    assert "too small" in rec["workspace_floats=0"][1] and rec["workspace_floats=0,r=16,S=20"][0] == -1
    for band, lattice in LATTICE_TWIN.items():       # the builders answer as their lattice twins do, under their own name
        twin = json.load(open(os.path.join(ROOT, "tests", "golden", "capi_messages.json")))[lattice]
        shared = [label for label in twin if label in golden[band]]
        assert len(shared) > 20, band
        for label in shared:
            assert golden[band][label][0] == twin[label][0], (band, label)
            assert golden[band][label][1].split(": ", 1)[-1] == twin[label][1].split(": ", 1)[-1], (band, label)


def test_header_is_plain_c():
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    subprocess.check_call(["gcc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", HEADER])
    subprocess.check_call(["g++", "-x", "c++", "-Wall", "-Werror", "-fsyntax-only", HEADER])


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tf-fast-rnnt_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tf_fast_rnnt as ft
    rec = _replies(ft)
    with open(GOLDEN, "w") as f:   # one entry point per line
        f.write("{\n" + ",\n".join(f"{json.dumps(n)}:{json.dumps(rec[n], separators=(',', ':'))}" for n in rec) + "\n}\n")
    print(f"{sum(len(v) for v in rec.values())} cases from {ft._lib.LIB_PATH} -> {GOLDEN}")
