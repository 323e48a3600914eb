"""The entry points of include/ftr_kd_topk.h (distillation on the pruned band from a stored top-K teacher), checked without a
device: they are declared, exported and bound with matching prototypes, their symbol table is disjoint from every other one,
the header parses as C99 and as C++ on its own, and their validation -- every device pointer NULL, so no call gets as far
as a launch -- answers in the order the header states.  Also the public signatures of rnnt_kd_loss_pruned_topk and
rnnt_kd_topk_teacher, their refusals that need no device, and the cache builder against the numpy top-K."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ftr_kd_topk.h")
FWD, BWD = "ftr_pruned_kd_topk_fwd_dt", "ftr_pruned_kd_topk_bwd_scaled_dt"
ENTRIES = (FWD, BWD)
DEFAULTS = dict(kind=0, teacher_kind=0, temperature=1.0, B=2, T=4, S=3, C=10, r=2, r_t=2, K=4, scale_stride=1, scale_mul=0.5)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _prototype(name):
    m = re.search(r"\b%s\s*\(([^()]*)\)\s*;" % name, _header())
    assert m, f"{name} is not declared in include/ftr_kd_topk.h"
    return [tuple(s.strip() for s in re.match(r"(.*?)(\w+)$", " ".join(p.split())).groups()) for p in m.group(1).split(",")]


def _call(ft, name, **over):
    """(return code, error text) of the entry with every pointer NULL and the other arguments from DEFAULTS / `over`"""
    vals = {**DEFAULTS, **over}
    args = [None if "*" in typ else vals[par] for typ, par in _prototype(name)]
    L = ft._lib.lib()
    rc = getattr(L, name)(*args)
    return rc, L.ftr_last_error().decode("utf-8", "replace")


def test_entries_are_declared_exported_and_bound(ft):
    handle = ctypes.CDLL(ft._lib.LIB_PATH)
    declared = set(re.findall(r"\b(ftr_\w+)\s*\(", _header()))
    assert declared == set(ENTRIES) == set(ft._lib.KD_TOPK_SYMBOLS)
    for name in ENTRIES:
        params = _prototype(name)
        restype, argtypes = ft._lib._KD_TOPK_SIGNATURES[name]
        assert hasattr(handle, name), f"{name} is not exported by libftr_hip.so"
        assert restype is ctypes.c_int and len(argtypes) == len(params), name
        for (typ, par), at in zip(params, argtypes):
            want = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double}.get(typ, ctypes.c_void_p)
            assert at is want and (want is not ctypes.c_void_p or "*" in typ), (name, par)
        assert params[-1] == ("void*", "stream"), name
        assert [par for _, par in params[-8:-1]] == ["B", "T", "S", "C", "r", "r_t", "K"], name
    assert _prototype(FWD)[:11] == _prototype(BWD)[:11]
    names = [par for _, par in _prototype(BWD)]
    assert names[names.index("scale"):names.index("scale") + 3] == ["scale", "scale_stride", "scale_mul"]
    text = open(HEADER).read()
    assert '#include "ftr_lowp.h"' in text and "#define FTR_KD_TOPK_MAX_K 64\n" in text and ft._lib.FTR_KD_TOPK_MAX_K == 64
    L = ft._lib.lib()
    assert L.ftr_abi_version() == 133 and L.ftr_package_version() == b"1.2" and ft.__version__ == "1.2"


def test_symbol_table_is_disjoint_from_every_other_one(ft):
    tables = [n for n in dir(ft._lib) if n.endswith("_SYMBOLS") and n != "KD_TOPK_SYMBOLS"]
    assert {"EXPORTED_SYMBOLS", "LOWP_SYMBOLS", "KD_SYMBOLS", "KD_FACT_SYMBOLS", "KD_LOSS_SYMBOLS", "TDT_MIX_SYMBOLS"} <= set(tables)
    for table in tables:
        assert not set(ft._lib.KD_TOPK_SYMBOLS) & set(getattr(ft._lib, table)), table
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):           # declared in the new header only
        if other != "ftr_kd_topk.h":
            text = open(os.path.join(ROOT, "include", other)).read()
            assert "kd_topk" not in text and not any(name in text for name in ENTRIES), other


def test_header_is_plain_c():
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    subprocess.check_call(["gcc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", HEADER])
    subprocess.check_call(["g++", "-x", "c++", "-Wall", "-Werror", "-fsyntax-only", HEADER])


@pytest.mark.parametrize("name", ENTRIES)
def test_validation_order(ft, name):
    bwd = name == BWD
    # (1) an unknown kind / teacher_kind, or a bad temperature: before anything else is looked at
    for over, words in ((dict(kind=7), ("7", "element type")), (dict(teacher_kind=9), ("9", "element type")),
                        (dict(temperature=0.0), ("temperature",)), (dict(temperature=-2.0), ("temperature",)),
                        (dict(temperature=float("inf")), ("temperature",)), (dict(temperature=float("nan")), ("temperature",))):
        rc, msg = _call(ft, name, **over)
        assert rc == 0 and all(w in msg for w in words) and msg.startswith(name[4:] + ":"), (over, rc, msg)   # FTR_ERR_INVALID_ARG
        assert _call(ft, name, **{"B": -1, "K": 0, **over}) == (rc, msg)
        assert _call(ft, name, **{"B": 0, **over}) == (rc, msg)
        if bwd:
            assert _call(ft, name, **{"scale_stride": 2, **over}) == (rc, msg)
    assert "element type" in _call(ft, name, kind=7, temperature=0.0)[1]
    # (2) sizes, r_t >= 1 and 1 <= K <= 64 among them; without teacher_ranges (NULL here) r_t must be r
    for over in (dict(B=-1), dict(T=0), dict(S=-1), dict(C=0), dict(r=0), dict(r_t=0)):
        rc, msg = _call(ft, name, **over)
        assert rc == 0 and "bad sizes" in msg, (over, rc, msg)
        assert _call(ft, name, **{"K": 65, **over}) == (rc, msg)
    for k in (0, -1, 65):
        rc, msg = _call(ft, name, K=k)
        assert rc == 0 and "K = %d" % k in msg and "[1,64]" in msg, (k, rc, msg)
        assert _call(ft, name, K=k, B=0) == (rc, msg)
        assert _call(ft, name, K=k, r_t=3) == (rc, msg)
        if bwd:
            assert _call(ft, name, K=k, scale_stride=2) == (rc, msg)
    for k in (1, 64):
        assert _call(ft, name, K=k)[1].endswith("null pointer")
    rc, msg = _call(ft, name, r_t=3)
    assert rc == 0 and "r_t = 3" in msg and "teacher_ranges" in msg, (rc, msg)
    assert _call(ft, name, r_t=3, B=0) == (rc, msg)
    # (3) the scale stride
    if bwd:
        for over in (dict(scale_stride=2), dict(scale_stride=-1)):
            rc, msg = _call(ft, name, **over)
            assert rc == 0 and "scale_stride" in msg, (over, rc, msg)
            assert _call(ft, name, B=0, **over) == (rc, msg)
    # B == 0: nothing to do; otherwise (4) the pointers (all NULL here), before (5) the device
    for kind in (0, 1, 2):
        for teacher_kind in (0, 1, 2):
            over = dict(kind=kind, teacher_kind=teacher_kind)
            assert _call(ft, name, B=0, **over) == (1, "")                      # FTR_OK
            rc, msg = _call(ft, name, **over)
            assert rc == 0 and msg.endswith("null pointer"), (over, rc, msg)


def test_public_signatures_and_docstrings(ft):
    E = inspect.Parameter.empty
    sig = [(n, p.default) for n, p in inspect.signature(ft.rnnt_kd_loss_pruned_topk).parameters.items()]
    assert sig == [("logits", E), ("teacher_values", E), ("teacher_indices", E), ("ranges", E), ("boundary", None),
                   ("teacher_ranges", None), ("teacher_rest", None), ("temperature", 1.0), ("node_weights", None),
                   ("reduction", "mean")]
    sig = [(n, p.default) for n, p in inspect.signature(ft.rnnt_kd_topk_teacher).parameters.items()]
    assert sig == [("teacher_logits", E), ("k", E), ("temperature", 1.0), ("with_rest", True)]
    doc = " ".join(ft.rnnt_kd_loss_pruned_topk.__doc__.split())
    for words in ("teacher_ranges[b,t,0]", "distilled", ".sum((1, 2))", "temperature ** 2", "rnnt_kd_topk_teacher", "clamped"):
        assert words in doc, words
    # the three existing distillation functions are what they were
    assert list(inspect.signature(ft.rnnt_kd_loss_pruned).parameters) == [
        "logits", "teacher_logits", "symbols", "ranges", "termination_symbol", "boundary", "mode", "temperature", "reduction"]
    assert list(inspect.signature(ft.rnnt_kd_loss_pruned_factored).parameters) == [
        "logits", "teacher_logits", "symbols", "ranges", "termination_symbol", "boundary", "factorization", "num_durations", "mode",
        "temperature", "duration_weight", "node_weights", "reduction"]
    assert list(inspect.signature(ft.rnnt_loss_pruned_kd).parameters) == [
        "logits", "teacher_logits", "symbols", "ranges", "termination_symbol", "boundary", "mode", "temperature", "rnnt_type",
        "delay_penalty", "reduction"]


def test_refusals_without_a_device(ft):
    f = ft.rnnt_kd_loss_pruned_topk
    x = torch.zeros(2, 4, 3, 8)
    v = torch.zeros(2, 4, 3, 5)
    i = torch.zeros(2, 4, 3, 5, dtype=torch.int32)
    rg = torch.zeros(2, 4, 3, dtype=torch.int32)
    w = torch.ones(2, 4, 3)
    for bad in (lambda: f(x.double(), v, i, rg), lambda: f(x, v.double(), i, rg), lambda: f(x, v, i.long(), rg),
                lambda: f(x, v, i, rg, teacher_rest=w.double()), lambda: f(x, v, i, rg, node_weights=w.half())):
        with pytest.raises(TypeError):
            bad()
    v2, i2 = torch.zeros(2, 4, 2, 5), torch.zeros(2, 4, 2, 5, dtype=torch.int32)
    for bad, match in ((lambda: f(x[0], v, i, rg), "logits"), (lambda: f(x, v[:, :3], i[:, :3], rg), "teacher_values"),
                       (lambda: f(x, v, i[..., :4], rg), "teacher_indices"),
                       (lambda: f(x, torch.zeros(2, 4, 3, 65), torch.zeros(2, 4, 3, 65, dtype=torch.int32), rg), "K = 65"),
                       (lambda: f(x, v[..., :0], i[..., :0], rg), "K = 0"),
                       (lambda: f(x, v2, i2, rg), "r_t = 2"),                          # no teacher_ranges: r_t must be s_range
                       (lambda: f(x, v2, i2, rg, teacher_ranges=rg), "teacher_ranges"),
                       (lambda: f(x, v, i, rg, teacher_rest=torch.zeros(2, 4, 2)), "teacher_rest"),
                       (lambda: f(x, v, i, rg, node_weights=torch.zeros(2, 4, 2)), "node_weights"),
                       (lambda: f(x, v, i, rg, temperature=0.0), "temperature"),
                       (lambda: f(x, v, i, rg, temperature=float("nan")), "temperature"),
                       (lambda: f(x, v, i, rg, reduction="other"), "reduction")):
        with pytest.raises(ValueError, match=match):
            bad()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(x, v, i, rg)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(x, v2, i2, rg, teacher_ranges=rg[:, :, :2], teacher_rest=torch.zeros(2, 4, 2), node_weights=w)
    with pytest.raises(ValueError, match="k = 9"):
        ft.rnnt_kd_topk_teacher(x, 9)
    with pytest.raises(ValueError, match="k = 0"):
        ft.rnnt_kd_topk_teacher(x, 0)
    with pytest.raises(ValueError, match="temperature"):
        ft.rnnt_kd_topk_teacher(x, 2, temperature=-1.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,k,tau", [(37, 5, 1.0), (500, 8, 2.0), (8, 8, 1.0)])
def test_cache_builder_against_numpy(ft, C, k, tau, dtype):
    """rnnt_kd_topk_teacher is plain torch and runs anywhere: values in the dtype of the logits, int32 columns, the rest at the
    given temperature (float32 logsumexp: a few ulp of float32 next to the float64 one); -inf when every column is stored."""
    import kd_topk_cases as TC
    y = torch.from_numpy(TC.dense_teacher(C, 4)).to(dtype)
    vals, idx, rest = ft.rnnt_kd_topk_teacher(y, k, temperature=tau)
    nv, ni, nr = TC.topk_cache(y.float().numpy(), k, tau, k < C)
    assert vals.dtype == dtype and idx.dtype == torch.int32 and rest.dtype == torch.float32
    assert vals.shape == y.shape[:-1] + (k,) == idx.shape and rest.shape == y.shape[:-1]
    assert np.array_equal(vals.float().numpy(), nv)           # ties (16-bit values) may pick another column of the same value
    assert np.array_equal(np.take_along_axis(y.float().numpy(), idx.numpy().astype(np.int64), -1), nv)
    assert all(len(set(row)) == k for row in idx.numpy().reshape(-1, k))
    if k < C:
        assert np.abs(rest.numpy() - nr).max() <= 8 * 2.0 ** -24 * max(1.0, np.abs(nr).max())
    else:
        assert torch.isinf(rest).all() and (rest < 0).all()
    assert ft.rnnt_kd_topk_teacher(y, k, with_rest=False)[2] is None
