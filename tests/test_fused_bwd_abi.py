"""The W-operand entry points of the fused d am kernel (include/ftr_fused.h), checked without a device: declared, exported,
bound, and validated like their product-operand twins of include/ftr.h.

They live in a header of their own, on top of ftr.h, for the reason tests/test_lowp_abi.py gives: ftr.h is pinned symbol for
symbol against _lib.EXPORTED_SYMBOLS and tests/golden/capi_messages.json.  The replies of the two pointer-taking entries
are recorded, over the table of argument vectors of tests/test_capi_messages.py, in tests/golden/fused_capi_messages.json:

    python tests/test_fused_bwd_abi.py
"""
import ctypes
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ftr_fused.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "fused_capi_messages.json")
ENTRIES = ("ftr_simple_logprobs_fused_bwd_am_w_f32", "ftr_smoothed_logprobs_fused_bwd_am_w_f32")
QUERY = "ftr_simple_logprobs_fused_bwd_am_w_columns"


def _text(path=HEADER):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _prototype(name, path=HEADER):
    m = re.search(r"\b%s\s*\(([^()]*)\)\s*;" % name, _text(path))
    assert m, f"{name} is not declared in {os.path.basename(path)}"
    out = []
    for p in m.group(1).split(","):
        typ, par = re.match(r"(.*?)(\w+)$", " ".join(p.split())).groups()
        out.append((typ.strip(), par))
    return out


def _replies(ft):
    import test_capi_messages as tcm
    L = ft._lib.lib()
    got = {}
    for name in ENTRIES:
        params, argtypes = _prototype(name), ft._lib._FUSED_SIGNATURES[name][1]
        names = {par for _, par in params}
        for over in [dict()] + [c for c in tcm.SINGLES + tcm.ARRAYS if set(c) <= names]:
            label = ",".join(f"{k}={over[k]}" for k in over).replace(" ", "") or "default"
            args, _keep = tcm.build_args(params, argtypes, over)
            rc = getattr(L, name)(*args)
            got.setdefault(name, {})[label] = [rc, L.ftr_last_error().decode("utf-8", "replace")]
    return got


def test_entries_are_declared_exported_and_bound(ft):
    handle = ctypes.CDLL(ft._lib.LIB_PATH)
    declared = set(re.findall(r"\b(ftr_\w+)\s*\(", _text()))
    assert declared == set(ENTRIES) | {QUERY} == set(ft._lib.FUSED_SYMBOLS)
    assert not set(ft._lib.FUSED_SYMBOLS) & (set(ft._lib.EXPORTED_SYMBOLS) | set(ft._lib.LOWP_SYMBOLS) | set(ft._lib.KD_SYMBOLS))
    for name in declared:
        assert hasattr(handle, name), f"{name} is not exported by libftr_hip.so"
        assert len(ft._lib._FUSED_SIGNATURES[name][1]) == len(_prototype(name)), name
    assert '#include "ftr.h"' in open(HEADER).read()
    assert ft._lib.lib().ftr_abi_version() == 133      # a header of its own: the version of ftr.h does not move


def test_arguments_are_the_product_operand_twins_with_w_for_prod():
    """Same order as ftr_*_logprobs_fused_bwd_am_f32 of ftr.h, `W` where `prod` was, and no combined scale (W carries it)."""
    ftr_h = os.path.join(ROOT, "include", "ftr.h")
    for name in ENTRIES:
        twin = [(t, "W" if n == "prod" else n) for t, n in _prototype(name.replace("_w_f32", "_f32"), ftr_h) if n != "combined_scale"]
        assert _prototype(name) == twin, name


def test_validation_replies_are_the_recorded_ones(ft):
    golden = json.load(open(GOLDEN))
    got = _replies(ft)
    assert set(got) == set(golden) == set(ENTRIES)
    for name in ENTRIES:
        assert set(got[name]) == set(golden[name]), name
        for label, reply in golden[name].items():
            assert reply[0] in (0, 1), (name, label)     # no recorded case got past validation
            assert got[name][label] == reply, (name, label, got[name][label], reply)
            # the same checks in the same order as the twin: its reply with the entry's own name in front
            assert reply[1] == "" or reply[1].startswith(name[len("ftr_"):-len("_f32")] + ":"), (name, label, reply)


def test_tiling_query_needs_no_device(ft, monkeypatch):
    """128 or 256 columns for any shape; FTR_FUSED_BWD_CT forces one, any other value is ignored."""
    L = ft._lib.lib()
    monkeypatch.delenv("FTR_FUSED_BWD_CT", raising=False)
    for shape in ((32, 1000, 500), (32, 2000, 1024), (1, 4, 4), (8, 8000, 512)):
        assert L.ftr_simple_logprobs_fused_bwd_am_w_columns(*shape) in (128, 256)
    for forced in (128, 256):
        monkeypatch.setenv("FTR_FUSED_BWD_CT", str(forced))
        assert L.ftr_simple_logprobs_fused_bwd_am_w_columns(32, 1000, 500) == forced
    monkeypatch.setenv("FTR_FUSED_BWD_CT", "192")
    assert L.ftr_simple_logprobs_fused_bwd_am_w_columns(32, 1000, 500) in (128, 256)


def test_header_is_plain_c():
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    subprocess.check_call(["gcc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", HEADER])
    subprocess.check_call(["g++", "-x", "c++", "-Wall", "-Werror", "-fsyntax-only", HEADER])


if __name__ == "__main__":
    for p in (os.path.join(ROOT, "tf-fast-rnnt_amd"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import tf_fast_rnnt as ft
    rec = _replies(ft)
    bad = {(n, c): v for n in rec for c, v in rec[n].items() if v[0] not in (0, 1)}
    assert not bad, f"cases that got past validation: {bad}"
    with open(GOLDEN, "w") as f:   # one entry point per line
        f.write("{\n" + ",\n".join(f"{json.dumps(n)}:{json.dumps(rec[n], separators=(',', ':'))}" for n in rec) + "\n}\n")
    print(f"{sum(len(v) for v in rec.values())} cases from {ft._lib.LIB_PATH} -> {GOLDEN}")
