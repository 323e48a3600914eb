"""The entry point of include/ftr_kd_topk_teacher.h, without a device: declared, exported and bound; the header is plain C; the
validation (every pointer NULL, so no call reaches a launch) answers in the order the header states; and the refusals of
rnnt_kd_topk_cache, all of which come before the device is looked at."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ftr_kd_topk_teacher.h")
ENTRY = "ftr_kd_teacher_topk_dt"
DEFAULTS = dict(kind=0, temperature=1.0, B=2, T=3, r=2, rows=12, C=10, K=4)


def _call(ft, **over):
    a = {**DEFAULTS, **over}
    L = ft._lib.lib()
    rc = getattr(L, ENTRY)(None, a["kind"], None, None, None, None, a["temperature"], a["B"], a["T"], a["r"], a["rows"], a["C"],
                           a["K"], None)
    return rc, L.ftr_last_error().decode("utf-8", "replace")


def test_entry_is_declared_exported_bound_and_plain_c(ft):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert set(re.findall(r"\b(ftr_\w+)\s*\(", text)) == {ENTRY} == set(ft._lib.KD_TOPK_TEACHER_SYMBOLS)
    assert hasattr(ctypes.CDLL(ft._lib.LIB_PATH), ENTRY) and callable(ft.rnnt_kd_topk_cache)
    assert len(re.search(r"\b%s\s*\(([^()]*)\)\s*;" % ENTRY, text).group(1).split(",")) == len(ft._lib._KD_TOPK_TEACHER_SIGNATURES[ENTRY][1]) == 14
    assert '#include "ftr_lowp.h"' in text and ft._lib.lib().ftr_abi_version() == 133
    subprocess.check_call(["gcc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", HEADER])
    subprocess.check_call(["g++", "-x", "c++", "-Wall", "-Werror", "-fsyntax-only", HEADER])


def test_validation_order(ft):
    steps = [(dict(kind=7), "element type"), (dict(C=0), "C = 0"), (dict(K=0), "K = 0"), (dict(K=11), "K = 11"),
             (dict(K=65, C=500), "K = 65"), (dict(temperature=0.0), "temperature"), (dict(temperature=float("nan")), "temperature"),
             (dict(rows=-1), "bad sizes")]
    for i, (over, word) in enumerate(steps):
        rc, msg = _call(ft, **over)
        assert rc == 0 and word in msg and msg.startswith(ENTRY[4:] + ":"), (over, rc, msg)     # FTR_ERR_INVALID_ARG
        for later, _ in steps[i + 1:]:                       # an earlier failing check is the reply, whatever comes later
            if not set(later) & set(over):
                assert _call(ft, **{**later, **over}) == (rc, msg), (over, later)
        assert "rows" in over or _call(ft, rows=0, **over) == (rc, msg)
    assert _call(ft, rows=0) == (1, "")                      # FTR_OK, nothing to do: before the pointers
    for kind in (0, 1, 2):                                   # the outputs are NULL: the pointers, before the device
        rc, msg = _call(ft, kind=kind)
        assert rc == 0 and msg.endswith("null pointer"), (kind, rc, msg)


def test_refusals_of_the_python_function(ft):
    y = torch.zeros(2, 3, 500)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ft.rnnt_kd_topk_cache(y, 8)
    with pytest.raises(TypeError, match="float64"):
        ft.rnnt_kd_topk_cache(y.double(), 8)
    for bad, match in ((dict(k=0), "k = 0"), (dict(k=65), "k = 65"), (dict(k=8, temperature=0.0), "temperature"),
                       (dict(k=8, temperature=-1.0), "temperature"), (dict(k=8, boundary=torch.zeros(2, 4, dtype=torch.int32)), "boundary")):
        with pytest.raises(ValueError, match=match):
            ft.rnnt_kd_topk_cache(y, **bad)
