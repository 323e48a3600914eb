"""include/ftr_path.h without a device: declared, exported, bound; an unknown dtype code or flag bit is refused first (all pointers NULL)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ftr_path.h")
ENTRIES = ("ftr_pruned_path_logprob_fwd_dt", "ftr_pruned_path_logprob_bwd_dt")


def _call(ft, name, kind=0, flags=0, B=1, T=4, S=2, C=10, r=2, blank=0):
    n_out = 3 if name.endswith("fwd_dt") else 4       # arc_lp, arc_lse, logprob | arc_lse, logprob, logprob_grad, glogits
    L = ft._lib.lib()
    rc = getattr(L, name)(None, kind, None, None, None, None, blank, *([None] * n_out), B, T, S, C, r, flags, None)
    return rc, L.ftr_last_error().decode()


def test_entries_are_declared_exported_and_bound(ft):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = dict(re.findall(r"\b(ftr_\w+)\s*\(([^()]*)\)\s*;", text))
    assert set(protos) == set(ENTRIES) == set(ft._lib.PATH_SYMBOLS)
    handle = ctypes.CDLL(ft._lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(handle, name), f"{name} is not exported by libftr_hip.so"
        assert len(protos[name].split(",")) == len(ft._lib._PATH_SIGNATURES[name][1])
        assert not any(name in getattr(ft._lib, t) for t in dir(ft._lib) if t.endswith("_SYMBOLS") and t != "PATH_SYMBOLS")
    assert ft._lib.FTR_PATH_MODIFIED == int(re.search(r"#define FTR_PATH_MODIFIED (\d+)", text).group(1)) == 2
    assert ft._lib.lib().ftr_abi_version() == 133 and callable(ft.rnnt_path_logprob_pruned)


@pytest.mark.parametrize("name", ENTRIES)
def test_unknown_dtype_or_flag_is_refused_first(ft, name):
    rc, msg = _call(ft, name, kind=7, flags=4, B=-1, blank=-1)
    assert rc == 0 and "element type" in msg and "7" in msg
    rc, msg = _call(ft, name, flags=4, B=-1, blank=-1)
    assert rc == 0 and "flags 4" in msg
    rc, msg = _call(ft, name, flags=3, T=0)
    assert rc == 0 and "bad sizes" in msg and msg.startswith("hat_")      # both known bits pass; then the sizes
    assert _call(ft, name, flags=1, C=1)[1].count("HAT needs") == 1 and "termination_symbol" in _call(ft, name, blank=10)[1]
    assert _call(ft, name, B=0) == (1, "")                                  # nothing to do, before the pointers
    for kind, flags in ((0, 0), (1, 2), (2, 3)):
        rc, msg = _call(ft, name, kind=kind, flags=flags)
        assert rc == 0 and msg.endswith("null pointer"), (kind, flags)
