"""The entry points of include/ftr_tdt_mix.h (the TDT loss mixed with the ordinary loss on the token head, omega), checked
without a device: they are declared, exported and bound with matching prototypes, their symbol table is disjoint from every
other table, the header parses as C99 and as C++, and their validation replies -- for the argument vectors of
tests/test_capi_messages.py, every device pointer NULL, so no call gets as far as a launch -- are the ones recorded in
tests/golden/tdt_mix_capi_messages.json:

    python tests/test_tdt_mix_abi.py          (records the file from the library as built)

Also here, because they need no device either: the public signatures of rnnt_loss_tdt_mixed[_pruned] and the refusal of an
omega outside [0, 1] before anything else is looked at."""
import ctypes
import inspect
import json
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ftr_tdt_mix.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "tdt_mix_capi_messages.json")
ENTRIES = ("ftr_tdt_mix_pruned_band_fwd_f32", "ftr_tdt_mix_pruned_logprobs_fwd_f32",
           "ftr_tdt_mix_pruned_band_bwd_scaled_f32", "ftr_tdt_mix_pruned_logprobs_bwd_scaled_f32")
# (the entry without the mix, the file its replies are recorded in)
TWIN = {"ftr_tdt_mix_pruned_band_fwd_f32": ("ftr_tdt_pruned_band_fwd_f32", "band_tdt_capi_messages.json"),
        "ftr_tdt_mix_pruned_logprobs_fwd_f32": ("ftr_tdt_pruned_logprobs_fwd_f32", "capi_messages.json"),
        "ftr_tdt_mix_pruned_band_bwd_scaled_f32": ("ftr_tdt_pruned_band_bwd_scaled_f32", "band_tdt_capi_messages.json"),
        "ftr_tdt_mix_pruned_logprobs_bwd_scaled_f32": ("ftr_tdt_pruned_logprobs_bwd_scaled_f32", "capi_messages.json")}
# on top of the table of tests/test_capi_messages.py: both parts by default, and what only these entries check.  With every
# pointer NULL a call whose `parts` / multipliers are accepted answers with the pointer check (or FTR_OK at B = 0).
EXTRA_DEFAULTS = dict(parts=3)
EXTRA_CASES = [dict(parts=0), dict(parts=4), dict(parts=-1), dict(parts=1), dict(parts=2), dict(parts=2, B=0), dict(parts=0, B=0),
               dict(parts=0, sigma=-1.0), dict(parts=0, T=0), dict(parts=4, r=4), dict(mul_tdt=0.0), dict(mul_rnnt=0.0),
               dict(mul_tdt=0.0, B=0), dict(mul_tdt=float("nan")), dict(mul_rnnt=float("inf")), dict(mul_tdt=float("nan"), B=-1),
               dict(mul_rnnt=float("nan"), sigma=-1.0), dict(mul_tdt=float("nan"), scale_stride=2)]


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
            params, argtypes = _prototypes()[name], ft._lib._TDT_MIX_SIGNATURES[name][1]
            names = {par for _, par in params}
            for over in [dict()] + [c for c in tcm.SINGLES + tcm.ARRAYS + EXTRA_CASES if set(c) <= names]:
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
    assert set(protos) == set(ENTRIES) == set(ft._lib.TDT_MIX_SYMBOLS)
    for name, params in protos.items():
        restype, argtypes = ft._lib._TDT_MIX_SIGNATURES[name]
        assert restype is ctypes.c_int
        assert hasattr(handle, name), f"{name} is not exported by libftr_hip.so"
        assert len(argtypes) == len(params), name
        for (typ, par), at in zip(params, argtypes):
            if typ == "int":
                assert at is ctypes.c_int, (name, par)
            elif typ == "float":
                assert at is ctypes.c_float, (name, par)
            elif typ == "double":
                assert at is ctypes.c_double, (name, par)
            elif par == "durations":
                assert typ == "const int32_t*" and at == ctypes.POINTER(ctypes.c_int32), (name, par)   # a host array
            else:
                assert "*" in typ and at is ctypes.c_void_p, (name, par)
    assert '#include "ftr_band_tdt.h"' in open(HEADER).read()
    assert ft._lib.lib().ftr_abi_version() == 133
    assert (ft._lib.FTR_TDT_MIX_TDT, ft._lib.FTR_TDT_MIX_RNNT) == (1, 2)
    assert re.search(r"#define FTR_TDT_MIX_TDT 1\b", open(HEADER).read()) and re.search(r"#define FTR_TDT_MIX_RNNT 2\b", open(HEADER).read())


def test_entries_extend_the_parameter_lists_of_their_twins(ft):
    """The twin's list with `parts` after sigma and the ordinary planes after the TDT planes (forward), or the ordinary
    occupancies after the TDT ones and the two multipliers in place of scale_mul (backward)."""
    import test_capi_messages as tcm
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_band_tdt_abi as band
    twins = {**tcm.prototypes(), **band._prototypes()}
    f, cf = "float*", "const float*"
    for name in ENTRIES:
        want = list(twins[TWIN[name][0]])
        pn = [p for _, p in want]
        if "fwd" in name:
            want.insert(pn.index("sigma") + 1, ("int", "parts"))
            at = [p for _, p in want].index("py_band" if "band" in name else "py") + 1
            want[at:at] = [(f, "px0_band"), (f, "py0_band")] if "band" in name else [(f, "px0"), (f, "py0")]
        else:
            at = pn.index("gy_band" if "band" in name else "gpy") + 1
            want[at:at] = [(cf, "gx0_band"), (cf, "gy0_band")] if "band" in name else [(cf, "gpx0"), (cf, "gpy0")]
            at = [p for _, p in want].index("scale_mul")
            want[at:at + 1] = [("float", "mul_tdt"), ("float", "mul_rnnt")]
        assert _prototypes()[name] == want, name


def test_symbol_table_is_disjoint_from_every_other_one(ft):
    tables = [getattr(ft._lib, n) for n in dir(ft._lib) if n.endswith("_SYMBOLS") and n != "TDT_MIX_SYMBOLS"]
    assert len(tables) >= 10
    for table in tables:
        assert not set(ft._lib.TDT_MIX_SYMBOLS) & set(table)
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if header != "ftr_tdt_mix.h":
            assert "tdt_mix" not in open(os.path.join(ROOT, "include", header)).read(), header


def test_validation_replies_are_the_recorded_ones(ft):
    golden = json.load(open(GOLDEN))
    got = _replies(ft)
    assert set(got) == set(golden) == set(ENTRIES)
    for name in ENTRIES:
        assert set(got[name]) == set(golden[name]), name
        for label, reply in golden[name].items():
            assert reply[0] in (0, 1), (name, label)     # no recorded case got past validation: INVALID_ARG or an early FTR_OK
            assert got[name][label] == reply, (name, label, got[name][label], reply)
    for name in ENTRIES:
        rec = golden[name]
        if "fwd" in name:
            for bad in ("parts=0", "parts=4", "parts=-1"):
                assert rec[bad][0] == 0 and "parts" in rec[bad][1], (name, bad)
            # an accepted `parts` gets as far as the pointer check; the planes of an absent part were NULL like all the others
            for ok in ("parts=1", "parts=2", "default"):
                assert rec[ok] == [0, rec["default"][1]] and "null pointer" in rec[ok][1], (name, ok)
            assert rec["parts=2,B=0"][0] == 1 and rec["parts=0,B=0"][0] == 0
            assert "sigma" in rec["parts=0,sigma=-1.0"][1] and "parts" in rec["parts=0,T=0"][1] and "parts" in rec["parts=4,r=4"][1]
        else:
            for bad in ("mul_tdt=nan", "mul_rnnt=inf", "mul_tdt=nan,B=-1", "mul_tdt=nan,scale_stride=2"):
                assert rec[bad][0] == 0 and "finite" in rec[bad][1], (name, bad)
            assert "sigma" in rec["mul_rnnt=nan,sigma=-1.0"][1]
            assert "null pointer" in rec["mul_tdt=0.0"][1] and "null pointer" in rec["mul_rnnt=0.0"][1] and rec["mul_tdt=0.0,B=0"][0] == 1
        twin_name, twin_file = TWIN[name]      # the shared cases answer as the twin does, under the entry's own name
        twin = json.load(open(os.path.join(ROOT, "tests", "golden", twin_file)))[twin_name]
        shared = [label for label in twin if label in rec]
        assert len(shared) >= 20, name
        for label in shared:
            assert rec[label][0] == twin[label][0], (name, label)
            assert rec[label][1].split(": ", 1)[-1] == twin[label][1].split(": ", 1)[-1], (name, label)


def test_header_is_plain_c():
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    subprocess.check_call(["gcc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", HEADER])
    subprocess.check_call(["g++", "-x", "c++", "-Wall", "-Werror", "-fsyntax-only", HEADER])


def test_public_signatures(ft):
    def sig(f):
        return [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert sig(ft.rnnt_loss_tdt_mixed_pruned) == [("logits", E), ("symbols", E), ("ranges", E), ("termination_symbol", E),
                                                  ("durations", E), ("omega", E), ("boundary", None), ("sigma", 0.0),
                                                  ("delay_penalty", 0.0), ("reduction", "mean")]
    assert sig(ft.rnnt_loss_tdt_mixed) == [("logits", E), ("symbols", E), ("termination_symbol", E), ("durations", E),
                                           ("omega", E), ("boundary", None), ("sigma", 0.0), ("delay_penalty", 0.0),
                                           ("reduction", "mean")]
    assert "rnnt_loss_tdt_mixed_pruned" in ft.rnnt_loss_tdt_pruned.__doc__
    assert "not claimed to be bit-compatible with NeMo" in " ".join(ft.rnnt_loss_tdt_mixed_pruned.__doc__.split())


@pytest.mark.parametrize("omega", [-0.1, 1.5, float("nan")])
def test_omega_outside_the_unit_interval_is_refused_first(ft, omega):
    """ValueError before any device check: the same call with a valid omega fails on its CPU tensors instead."""
    x = torch.zeros(1, 4, 2, 7)
    sym = torch.zeros(1, 3, dtype=torch.int32)
    rg = torch.zeros(1, 4, 2, dtype=torch.int32)
    with pytest.raises(ValueError, match="omega"):
        ft.rnnt_loss_tdt_mixed_pruned(x, sym, rg, 0, (0, 1), omega)
    with pytest.raises(ValueError, match="omega"):
        ft.rnnt_loss_tdt_mixed(torch.zeros(1, 4, 4, 7), sym, 0, (0, 1), omega)
    for ok in (0.0, 0.5, 1.0):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ft.rnnt_loss_tdt_mixed_pruned(x, sym, rg, 0, (0, 1), ok)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tf-fast-rnnt_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tf_fast_rnnt as ft
    rec = _replies(ft)
    with open(GOLDEN, "w") as f:   # one entry point per line
        f.write("{\n" + ",\n".join(f"{json.dumps(n)}:{json.dumps(rec[n], separators=(',', ':'))}" for n in rec) + "\n}\n")
    print(f"{sum(len(v) for v in rec.values())} cases from {ft._lib.LIB_PATH} -> {GOLDEN}")
