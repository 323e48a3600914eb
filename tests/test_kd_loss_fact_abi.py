"""The entry points of include/ftr_kd_loss_fact.h (the transducer loss on the pruned band and the factored distillation loss in
one pass: HAT rows, node weights, occupancy weights), checked without a device: they are declared, exported and bound with
matching prototypes, their symbol table is disjoint from every other one, the header parses as C99 and as C++ on its own, and
their validation -- every device pointer NULL, so no call gets as far as a launch -- answers in the order the header states;
the replies are recorded in tests/golden/kd_loss_fact_capi_messages.json.  Also the public signatures of
rnnt_loss_pruned_kd_factored and rnnt_node_occupancy_pruned and their refusals that need no device.

    python tests/test_kd_loss_fact_abi.py        records tests/golden/kd_loss_fact_capi_messages.json from the library as built"""
import ctypes
import inspect
import json
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ftr_kd_loss_fact.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "kd_loss_fact_capi_messages.json")
FWD, BWD = "ftr_pruned_band_kd_fact_fwd_dt", "ftr_pruned_band_kd_fact_bwd_scaled_dt"
OCC, USUM = "ftr_band_node_occupancy_f32", "ftr_pruned_kd_weighted_utt_sum_f32"
ENTRIES = (FWD, BWD, OCC, USUM)
DEFAULTS = dict(kind=0, teacher_kind=0, termination_symbol=0, temperature=1.0, mode=0, delay_penalty=0.0, modified=0, B=2, T=4,
                S=3, C=10, r=2, loss_scale_stride=0, loss_scale_mul=1.0, kd_scale_stride=1, kd_scale_mul=0.5, factorization=0)
# the recorded cases: every check of the row entries alone, and against what answers later
RECORDED = [dict(), dict(kind=7), dict(teacher_kind=9), dict(mode=2), dict(temperature=0.0), dict(temperature=float("nan")),
            dict(factorization=1), dict(factorization=2), dict(factorization=3), dict(factorization=-1), dict(factorization=2, B=-1),
            dict(factorization=2, B=0), dict(factorization=3, mode=2), dict(factorization=2, temperature=0.0),
            dict(factorization=1, C=1), dict(factorization=1, C=1, B=-1), dict(factorization=1, C=1, termination_symbol=5),
            dict(factorization=0, C=1), dict(loss_scale_mul=float("nan")), dict(kd_scale_mul=float("inf"), factorization=2),
            dict(kd_scale_mul=float("inf"), B=-1), dict(B=-1), dict(T=0), dict(S=-1), dict(C=0), dict(r=0),
            dict(termination_symbol=10), dict(termination_symbol=-1, B=0), dict(loss_scale_stride=2), dict(kd_scale_stride=-1, B=0),
            dict(B=0), dict(B=0, factorization=1), dict(loss_scale_mul=0.0), dict(kd_scale_mul=0.0), dict(kind=1, teacher_kind=2, mode=1)]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _prototype(name):
    m = re.search(r"\b%s\s*\(([^()]*)\)\s*;" % name, _header())
    assert m, f"{name} is not declared in include/ftr_kd_loss_fact.h"
    return [tuple(s.strip() for s in re.match(r"(.*?)(\w+)$", " ".join(p.split())).groups()) for p in m.group(1).split(",")]


def _call(ft, name, **over):
    """(return code, error text) of the entry with every pointer NULL and the other arguments from DEFAULTS / `over`"""
    vals = {**DEFAULTS, **over}
    args = [None if "*" in typ else vals[par] for typ, par in _prototype(name)]
    L = ft._lib.lib()
    rc = getattr(L, name)(*args)
    return rc, L.ftr_last_error().decode("utf-8", "replace")


def _label(over):
    return ",".join(f"{k}={v}" for k, v in over.items()) or "defaults"


def _replies(ft):
    out = {}
    for name in ENTRIES:
        known = {par for _, par in _prototype(name)}
        out[name] = {_label(over): list(_call(ft, name, **over)) for over in RECORDED if set(over) <= known}
    return out


def test_entries_are_declared_exported_and_bound(ft):
    handle = ctypes.CDLL(ft._lib.LIB_PATH)
    declared = set(re.findall(r"\b(ftr_\w+)\s*\(", _header()))
    assert declared == set(ENTRIES) == set(ft._lib.KD_LOSS_FACT_SYMBOLS)
    for name in ENTRIES:
        params = _prototype(name)
        restype, argtypes = ft._lib._KD_LOSS_FACT_SIGNATURES[name]
        assert hasattr(handle, name), f"{name} is not exported by libftr_hip.so"
        assert restype is ctypes.c_int and len(argtypes) == len(params), name
        for (typ, par), at in zip(params, argtypes):
            want = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double}.get(typ, ctypes.c_void_p)
            assert at is want and (want is not ctypes.c_void_p or "*" in typ), (name, par)
        assert params[-1] == ("void*", "stream"), name
    # the argument lists of the ftr_kd_loss.h entries plus (factorization, node_weights) in front of the stream
    import test_kd_loss_abi as A
    for name, kd in zip((FWD, BWD), A.ENTRIES):
        assert _prototype(name)[:-3] == A._prototype(kd)[:-1], name
        assert _prototype(name)[-3:] == [("int", "factorization"), ("const float*", "node_weights"), ("void*", "stream")], name
    assert '#include "ftr_kd_fact.h"' in open(HEADER).read()
    L = ft._lib.lib()
    assert L.ftr_abi_version() == 133 and L.ftr_package_version() == b"1.2" and ft.__version__ == "1.2"


def test_symbol_table_is_disjoint_from_every_other_one(ft):
    tables = [n for n in dir(ft._lib) if n.endswith("_SYMBOLS") and n != "KD_LOSS_FACT_SYMBOLS"]
    assert {"EXPORTED_SYMBOLS", "LOWP_SYMBOLS", "KD_SYMBOLS", "KD_FACT_SYMBOLS", "KD_LOSS_SYMBOLS", "KD_TOPK_SYMBOLS"} <= set(tables)
    for table in tables:
        assert not set(ft._lib.KD_LOSS_FACT_SYMBOLS) & set(getattr(ft._lib, table)), table
        for other in getattr(ft._lib, table):          # and no name of one table inside a name of the other
            assert not any(other in name or name in other for name in ENTRIES), (table, other)
    text = open(HEADER).read()
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != "ftr_kd_loss_fact.h":
            assert not any(name in open(os.path.join(ROOT, "include", other)).read() for name in ENTRIES), other   # declared here only
    for table in tables:                                # the header speaks of the other headers' entries by header, never by name
        if table != "EXPORTED_SYMBOLS":                 # (ftr.h's ftr_last_error() and ftr_abi_version() are named in every header)
            assert not any(other in text for other in getattr(ft._lib, table)), table


def test_header_is_plain_c():
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    subprocess.check_call(["gcc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", HEADER])
    subprocess.check_call(["g++", "-x", "c++", "-Wall", "-Werror", "-fsyntax-only", HEADER])


@pytest.mark.parametrize("name", (FWD, BWD))
def test_validation_order(ft, name):
    bwd = name == BWD
    # an unknown kind / teacher_kind / mode, a bad temperature, an unknown factorization or TDT: before anything else
    for over, words in ((dict(kind=7), ("7", "element type")), (dict(teacher_kind=9), ("9", "element type")),
                        (dict(mode=2), ("2", "mode")), (dict(mode=-1), ("-1", "mode")), (dict(temperature=0.0), ("temperature",)),
                        (dict(temperature=float("inf")), ("temperature",)), (dict(temperature=float("nan")), ("temperature",)),
                        (dict(factorization=3), ("3", "factorization")), (dict(factorization=-1), ("-1", "factorization")),
                        (dict(factorization=2), ("FTR_KD_FACT_TDT", "out of scope"))):
        rc, msg = _call(ft, name, **over)
        assert rc == 0 and all(w in msg for w in words) and msg.startswith(name[4:] + ":"), (over, rc, msg)   # FTR_ERR_INVALID_ARG
        assert _call(ft, name, **{"B": -1, "termination_symbol": -1, **over}) == (rc, msg)
        assert _call(ft, name, **{"B": 0, **over}) == (rc, msg)
        if bwd:
            assert _call(ft, name, **{"loss_scale_mul": float("nan"), "kd_scale_stride": 2, **over}) == (rc, msg)
    assert "element type" in _call(ft, name, kind=7, mode=2)[1] and "mode" in _call(ft, name, mode=2, factorization=2)[1]
    assert "temperature" in _call(ft, name, temperature=0.0, factorization=3)[1]
    if bwd:   # then the two multipliers, which must be finite
        for over in (dict(loss_scale_mul=float("nan")), dict(kd_scale_mul=float("inf")), dict(kd_scale_mul=float("-inf"))):
            rc, msg = _call(ft, name, **over)
            assert rc == 0 and "finite" in msg, (over, rc, msg)
            assert _call(ft, name, **{"B": -1, "loss_scale_stride": 2, **over}) == (rc, msg)
            assert _call(ft, name, **{"B": 0, **over}) == (rc, msg)
    # then sizes (HAT's C >= 2 with them), the termination symbol, the scale strides
    for over in (dict(B=-1), dict(T=0), dict(S=-1), dict(C=0), dict(r=0)):
        rc, msg = _call(ft, name, **over)
        assert rc == 0 and "bad sizes" in msg, (over, rc, msg)
        assert _call(ft, name, **{"termination_symbol": 10, **over}) == (rc, msg)
    assert "HAT" in _call(ft, name, factorization=1, C=1)[1] and "HAT" in _call(ft, name, factorization=1, C=1, termination_symbol=5)[1]
    assert "bad sizes" in _call(ft, name, factorization=1, C=1, B=-1)[1]
    assert _call(ft, name, factorization=0, C=1)[1].endswith("null pointer")
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
                for fact in (0, 1):
                    over = dict(kind=kind, teacher_kind=teacher_kind, mode=mode, factorization=fact)
                    assert _call(ft, name, B=0, **over) == (1, "")                      # FTR_OK
                    rc, msg = _call(ft, name, **over)
                    assert rc == 0 and msg.endswith("null pointer"), (over, rc, msg)
    if bwd:   # an absent part: still the pointers of the other one
        for over in (dict(loss_scale_mul=0.0), dict(kd_scale_mul=0.0), dict(loss_scale_mul=0.0, kd_scale_mul=0.0)):
            assert _call(ft, name, **over)[1].endswith("null pointer") and _call(ft, name, B=0, **over)[0] == 1


@pytest.mark.parametrize("name", (OCC, USUM))
def test_validation_order_of_the_small_entries(ft, name):
    for over in (dict(B=-1), dict(T=0), dict(r=0)) + ((dict(S=-1),) if name == OCC else ()):
        rc, msg = _call(ft, name, **over)
        assert rc == 0 and "bad sizes" in msg and msg.startswith(name[4:-4] + ":"), (over, rc, msg)
    assert _call(ft, name, B=0) == (1, "")
    rc, msg = _call(ft, name)
    assert rc == 0 and msg.endswith("null pointer")


def test_validation_replies_are_the_recorded_ones(ft):
    golden = json.load(open(GOLDEN))
    got = _replies(ft)
    assert set(got) == set(golden) == set(ENTRIES)
    for name in ENTRIES:
        assert set(got[name]) == set(golden[name]), name
        for label, reply in golden[name].items():
            assert reply[0] in (0, 1), (name, label)     # no recorded case got past validation
            assert got[name][label] == reply, (name, label, got[name][label], reply)


def test_public_signatures_and_docstrings(ft):
    E = inspect.Parameter.empty
    sig = [(n, p.default) for n, p in inspect.signature(ft.rnnt_loss_pruned_kd_factored).parameters.items()]
    assert sig == [("logits", E), ("teacher_logits", E), ("symbols", E), ("ranges", E), ("termination_symbol", E),
                   ("boundary", None), ("factorization", "softmax"), ("mode", "full"), ("temperature", 1.0), ("node_weights", None),
                   ("rnnt_type", "regular"), ("delay_penalty", 0.0), ("reduction", "mean")]
    sig = [(n, p.default) for n, p in inspect.signature(ft.rnnt_node_occupancy_pruned).parameters.items()]
    assert sig == [("logits", E), ("symbols", E), ("ranges", E), ("termination_symbol", E), ("boundary", None),
                   ("factorization", "softmax"), ("rnnt_type", "regular"), ("delay_penalty", 0.0)]
    doc = " ".join(ft.rnnt_loss_pruned_kd_factored.__doc__.split())
    for words in ("hat_loss_pruned", "rnnt_kd_loss_pruned_factored(", '"occupancy"', "out of scope", "s_range <= 15", "weight is 0",
                  "rnnt_node_occupancy_pruned("):
        assert words in doc, words
    doc = " ".join(ft.rnnt_node_occupancy_pruned.__doc__.split())
    for words in ("[B,T,s_range]", "exact zeros", "detached", "No gradient"):
        assert words in doc, words
    # the functions composed are what they were
    assert list(inspect.signature(ft.rnnt_kd_loss_pruned_factored).parameters) == [
        "logits", "teacher_logits", "symbols", "ranges", "termination_symbol", "boundary", "factorization", "num_durations", "mode",
        "temperature", "duration_weight", "node_weights", "reduction"]
    assert list(inspect.signature(ft.hat_loss_pruned).parameters) == [
        "logits", "symbols", "ranges", "termination_symbol", "boundary", "rnnt_type", "delay_penalty", "reduction"]


def test_refusals_without_a_device(ft):
    x = torch.zeros(2, 4, 2, 8)
    sym = torch.zeros(2, 3, dtype=torch.int32)
    rg = torch.zeros(2, 4, 2, dtype=torch.int32)
    f, occ = ft.rnnt_loss_pruned_kd_factored, ft.rnnt_node_occupancy_pruned
    with pytest.raises(ValueError, match="rnnt_type"):
        f(x, x, sym, rg, 0, rnnt_type="other")
    with pytest.raises(ValueError, match="out of scope"):
        f(x, x, sym, rg, 0, factorization="tdt")
    with pytest.raises(ValueError, match="out of scope"):
        occ(x, sym, rg, 0, factorization="tdt")
    with pytest.raises(ValueError, match="factorization"):
        occ(x, sym, rg, 0, factorization="other")
    with pytest.raises(ValueError, match="node_weights"):
        f(x, x, sym, rg, 0, node_weights="all")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(x[..., :1], x[..., :1], sym, rg, 0, factorization="hat")      # C < 2: the device is still asked for first
    for kw in (dict(), dict(factorization="hat"), dict(node_weights="occupancy"), dict(node_weights=torch.ones(2, 4, 2))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(x, x, sym, rg, 0, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(x.double(), x, sym, rg, 0, factorization="hat")        # the device is asked for first, as hat_loss_pruned does
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        occ(x, sym, rg, 0)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tf-fast-rnnt_amd"))
    import tf_fast_rnnt
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as fh:
        json.dump(_replies(tf_fast_rnnt), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", GOLDEN)
