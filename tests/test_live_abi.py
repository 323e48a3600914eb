"""The entry points of include/ftr_live.h (the W kernel with its table of live frame intervals, the fused d am kernel that
reads it), checked without a device: declared, exported, bound, disjoint from every other header's table, and argument for
argument their twins of ftr.h / ftr_fused.h with `live` added behind rsy (W entries) or behind W (d am entries)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ftr_live.h")
TWINS = {   # entry -> (header of the twin, twin, the argument `live` follows)
    "ftr_simple_logprobs_bwd_w_live_f32": ("ftr.h", "ftr_simple_logprobs_bwd_w_scaled_f32", "rsy"),
    "ftr_smoothed_logprobs_bwd_w_live_f32": ("ftr.h", "ftr_smoothed_logprobs_bwd_w_scaled_f32", "rsy"),
    "ftr_simple_logprobs_fused_bwd_am_live_f32": ("ftr_fused.h", "ftr_simple_logprobs_fused_bwd_am_w_f32", "W"),
    "ftr_smoothed_logprobs_fused_bwd_am_live_f32": ("ftr_fused.h", "ftr_smoothed_logprobs_fused_bwd_am_w_f32", "W"),
}
OTHER_TABLES = ("EXPORTED_SYMBOLS", "LOWP_SYMBOLS", "PRUNE_SUM_SYMBOLS", "JOINER_ACT_SYMBOLS", "KD_SYMBOLS", "FUSED_SYMBOLS",
                "BAND_TDT_SYMBOLS", "BAND_MULTIBLANK_SYMBOLS", "BAND_VITERBI_SYMBOLS")


def _text(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _prototype(name, path):
    m = re.search(r"\b%s\s*\(([^()]*)\)\s*;" % name, _text(path))
    assert m, f"{name} is not declared in {os.path.basename(path)}"
    return [re.match(r"(.*?)(\w+)$", " ".join(p.split())).groups() for p in m.group(1).split(",")]


def test_entries_are_declared_exported_and_bound(ft):
    handle = ctypes.CDLL(ft._lib.LIB_PATH)
    declared = set(re.findall(r"\b(ftr_\w+)\s*\(", _text(HEADER)))
    assert declared == set(TWINS) == set(ft._lib.LIVE_SYMBOLS)
    for table in OTHER_TABLES:
        assert not declared & set(getattr(ft._lib, table)), table
    for name in declared:
        assert hasattr(handle, name), f"{name} is not exported by libftr_hip.so"
        assert len(ft._lib._LIVE_SIGNATURES[name][1]) == len(_prototype(name, HEADER)), name
    assert '#include "ftr_fused.h"' in open(HEADER).read()
    assert ft._lib.lib().ftr_abi_version() == 133      # a header of its own: the version of ftr.h does not move


@pytest.mark.parametrize("name", sorted(TWINS))
def test_arguments_are_the_twins_with_live_added(name):
    header, twin, after = TWINS[name]
    want = []
    for typ, par in _prototype(twin, os.path.join(ROOT, "include", header)):
        want.append((typ.strip(), par))
        if par == after:
            want.append(("int32_t*" if after == "rsy" else "const int32_t*", "live"))
    assert [(t.strip(), p) for t, p in _prototype(name, HEADER)] == want


@pytest.mark.parametrize("name", sorted(TWINS))
def test_sizes_are_checked_before_pointers_and_device(ft, name):
    """A negative size is refused with the entry's own name in the reply, whatever the pointers: no device needed."""
    L = ft._lib.lib()
    args = []
    for (typ, par), ctype in zip(_prototype(name, HEADER), ft._lib._LIVE_SIGNATURES[name][1]):
        if ctype is ctypes.c_void_p:
            args.append(None)
        elif ctype is ctypes.c_float:
            args.append(1.0)
        else:
            args.append({"B": -1, "T": 8, "S": 3, "C": 8, "termination_symbol": 7}.get(par, 0))
    rc = getattr(L, name)(*args)
    msg = L.ftr_last_error().decode()
    assert rc == 0 and msg.startswith(name[len("ftr_"):-len("_f32")] + ":"), (rc, msg)     # FTR_ERR_INVALID_ARG


def test_header_is_plain_c():
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    subprocess.check_call(["gcc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", HEADER])
    subprocess.check_call(["g++", "-x", "c++", "-Wall", "-Werror", "-fsyntax-only", HEADER])
