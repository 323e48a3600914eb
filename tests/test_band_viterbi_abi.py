"""The band-native alignment entry points of the C ABI (include/ftr_band_viterbi.h), checked without a device: they are
declared, exported and bound with matching prototypes, their symbol table is disjoint from every other one, the queries
answer 0 outside the domain, and the validation replies of the entry -- for the argument vectors of
tests/test_capi_messages.py, every device pointer NULL, so no call gets as far as a launch -- are the ones recorded in
tests/golden/band_viterbi_capi_messages.json:

    python tests/test_band_viterbi_abi.py          (records the file from the library as built)
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
HEADER = os.path.join(ROOT, "include", "ftr_band_viterbi.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "band_viterbi_capi_messages.json")
QUERIES = ("ftr_mutual_information_band_viterbi_supported", "ftr_mutual_information_band_viterbi_workspace_bytes")
ENTRIES = ("ftr_mutual_information_band_viterbi_f32",)
OTHER_TABLES = ("EXPORTED_SYMBOLS", "LOWP_SYMBOLS", "KD_SYMBOLS", "FUSED_SYMBOLS", "BAND_TDT_SYMBOLS", "BAND_MULTIBLANK_SYMBOLS")
# on top of the table of tests/test_capi_messages.py: the second move count, and what only this entry checks
EXTRA_DEFAULTS = dict(Ny=1)
NINE = dict(N=4, token_durations=(0, 1, 2, 3), Ny=5, blank_durations=(1, 2, 3, 4, 5))
TEN = dict(N=5, token_durations=(0, 1, 2, 3, 4), Ny=5, blank_durations=(1, 2, 3, 4, 5))
EXTRA_CASES = [dict(Ny=0), dict(Ny=9), dict(N=9), NINE, TEN, dict(TEN, B=0), dict(TEN, T=0), dict(r=16, S=20), dict(r=15, S=20),
               dict(r=16, S=20, B=0), dict(token_durations=(0, 17)), dict(blank_durations=(32,)), dict(blank_durations=(2,)),
               dict(T=0, r=16), dict(workspace_bytes=0, r=16, S=20), dict(N=0, T=0), dict(S=0), dict(S=0, workspace_bytes=0)]


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
    saved = dict(tcm.DEFAULTS)
    tcm.DEFAULTS.update(EXTRA_DEFAULTS)
    try:
        L = ft._lib.lib()
        got = {}
        for name in ENTRIES:
            params, argtypes = _prototypes()[name], ft._lib._BAND_VITERBI_SIGNATURES[name][1]
            names = {par for _, par in params}
            # `durations` is an output device pointer here, not the host list it names in the inherited table: those cases are left out
            for over in [dict()] + [c for c in tcm.SINGLES + tcm.ARRAYS + EXTRA_CASES if set(c) <= names - {"durations"}]:
                label = ",".join(f"{k}={over[k]}" for k in over).replace(" ", "") or "default"
                args, _keep = tcm.build_args(params, argtypes, over)
                rc = getattr(L, name)(*args)
                got.setdefault(name, {})[label] = [rc, L.ftr_last_error().decode("utf-8", "replace")]
        return got
    finally:
        tcm.DEFAULTS.clear()
        tcm.DEFAULTS.update(saved)


def test_entries_are_declared_exported_and_bound(ft):
    protos = _prototypes()
    handle = ctypes.CDLL(ft._lib.LIB_PATH)
    assert set(protos) == set(QUERIES) | set(ENTRIES) == set(ft._lib.BAND_VITERBI_SYMBOLS)
    for name, params in protos.items():
        restype, argtypes = ft._lib._BAND_VITERBI_SIGNATURES[name]
        assert hasattr(handle, name), f"{name} is not exported by libftr_hip.so"
        assert len(argtypes) == len(params), name
        for (typ, par), at in zip(params, argtypes):
            if typ == "int":
                assert at is ctypes.c_int, (name, par)
            elif typ == "size_t":
                assert at is ctypes.c_size_t, (name, par)
            elif par in ("token_durations", "blank_durations"):
                assert typ == "const int32_t*" and at == ctypes.POINTER(ctypes.c_int32), (name, par)   # host arrays
            else:
                assert "*" in typ and at is ctypes.c_void_p, (name, par)
    assert ft._lib._BAND_VITERBI_SIGNATURES[QUERIES[0]][0] is ctypes.c_int
    assert ft._lib._BAND_VITERBI_SIGNATURES[QUERIES[1]][0] is ctypes.c_size_t
    assert [p for _, p in protos[QUERIES[0]]] == ["T", "S", "r", "N", "Ny"]
    assert [p for _, p in protos[QUERIES[1]]] == ["B", "T", "S", "r", "N", "Ny"]
    assert [p for _, p in protos[ENTRIES[0]]] == ["px_band", "py_band", "ranges", "boundary", "token_durations", "N", "blank_durations",
                                                  "Ny", "workspace", "workspace_bytes", "score", "frames", "durations", "blank_steps",
                                                  "B", "T", "S", "r", "stream"]
    assert '#include "ftr.h"' in open(HEADER).read()
    assert ft._lib.lib().ftr_abi_version() == 133


def test_symbol_table_is_disjoint_from_every_other_one(ft):
    for table in OTHER_TABLES:
        assert not set(ft._lib.BAND_VITERBI_SYMBOLS) & set(getattr(ft._lib, table)), table
    for header in os.listdir(os.path.join(ROOT, "include")):
        if header != "ftr_band_viterbi.h":
            assert "band_viterbi" not in open(os.path.join(ROOT, "include", header)).read(), header


def test_queries_answer_without_a_device(ft):
    L = ft._lib.lib()
    sup, ws = L.ftr_mutual_information_band_viterbi_supported, L.ftr_mutual_information_band_viterbi_workspace_bytes
    assert sup(40, 12, 4, 2, 1) == 1 and sup(40, 12, 15, 5, 4) == 1 and sup(40, 12, 15, 1, 8) == 1 and sup(40, 0, 1, 8, 1) == 1
    for bad in ((40, 12, 16, 2, 1), (40, 12, 4, 5, 5), (40, 12, 4, 0, 1), (40, 12, 0, 2, 1), (0, 12, 4, 2, 1), (40, -1, 4, 2, 1),
                (40, 12, 4, 2, 0), (40, 12, 4, 9, 1), (40, 12, 4, 1, 9)):
        assert sup(*bad) == 0 and ws(2, *bad) == 0, bad
    assert ws(-1, 40, 12, 4, 2, 1) == 0
    # the header's formula; nothing of size S * T: linear in B, S + T and the move count
    for B, T, S, r, N, Ny in ((1, 1500, 300, 5, 5, 4), (3, 40, 12, 8, 1, 8), (2, 9, 0, 1, 1, 1)):
        steps, lanes = (S + T + 1 + 3) // 4 * 4, 8 if r <= 7 else 16
        assert ws(B, T, S, r, N, Ny) == B * ((steps + 4) * lanes * (N + Ny + 1) * 4 + steps * lanes // 2)
    base = ws(1, 1500, 300, 5, 5, 4)
    assert 0 < base < 300 * 1501 * 4                 # below ONE px plane of the lattice route
    assert ws(1, 3000, 600, 5, 5, 4) <= 2 * base + 4096
    assert ws(1, 1500, 300, 8, 5, 4) <= 2 * base + 4096          # 16 lanes instead of 8


def test_validation_replies_are_the_recorded_ones(ft):
    golden = json.load(open(GOLDEN))
    got = _replies(ft)
    assert set(got) == set(golden) == set(ENTRIES)
    rec = golden[ENTRIES[0]]
    assert set(got[ENTRIES[0]]) == set(rec)
    for label, reply in rec.items():
        # no recorded case got past validation: FTR_ERR_INVALID_ARG, an early FTR_OK, or FTR_ERR_UNSUPPORTED for the domain
        assert reply[0] in (0, 1, -1) and (reply[0] != -1 or "outside the kernel's domain" in reply[1]), label
        assert got[ENTRIES[0]][label] == reply, (label, got[ENTRIES[0]][label], reply)
        assert "durations=" not in label.replace("token_durations=", "").replace("blank_durations=", ""), label
    # what the header states about the order: duration lists, sizes, the domain, B == 0, the workspace, the pointers
    nine = "N=4,token_durations=(0,1,2,3),Ny=5,blank_durations=(1,2,3,4,5)"
    ten = "N=5,token_durations=(0,1,2,3,4),Ny=5,blank_durations=(1,2,3,4,5)"
    assert "token_durations" in rec["N=0"][1] and rec["N=0"][0] == 0 and "token_durations" in rec["N=0,T=0"][1]
    assert "blank_durations" in rec["Ny=0"][1] and rec["Ny=0"][0] == 0 and rec["Ny=9"][0] == 0 and rec["N=9"][0] == 0
    assert rec["token_durations=(0,17)"][0] == 0 and rec["blank_durations=(33,)"][0] == 0
    assert "null" in rec["blank_durations=(32,)"][1] and "null" in rec["blank_durations=(2,)"][1]    # the lists pass
    assert "bad sizes" in rec["T=0,r=16"][1] and "bad sizes" in rec[ten + ",T=0"][1]
    assert rec[ten][0] == -1 and rec[ten + ",B=0"][0] == -1 and "null" in rec[nine][1]
    assert rec["r=16,S=20,B=0"][0] == -1 and rec["r=16,S=20"][0] == -1 and rec["r=15,S=20"][0] == 0 and rec["B=0"][0] == 1
    assert rec["workspace_bytes=0,r=16,S=20"][0] == -1 and "too small" in rec["workspace_bytes=0"][1]
    assert rec["B=0,workspace_bytes=0"][0] == 1 and "too small" in rec["S=0,workspace_bytes=0"][1]
    assert "null" in rec["default"][1] and "null" in rec["S=0"][1]


def test_header_is_plain_c():
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
