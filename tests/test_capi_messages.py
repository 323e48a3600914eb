"""Every validation reply of the C ABI, pinned without a GPU: the return code and the ftr_last_error() text of each entry
point of include/ftr.h that takes a pointer, for a table of argument vectors whose device pointers are all NULL (so no
call can get as far as a launch: the answer is FTR_ERR_INVALID_ARG = 0 or an early FTR_OK = 1, never FTR_ERR_NO_DEVICE).
tests/golden/capi_messages.json was recorded once, from the library as it stood before the argument checks of capi.hip
were folded onto shared helpers:

    FTR_LIB_PATH=<that build's libftr_hip.so> python tests/test_capi_messages.py

The table: per entry point the all-NULL call with every size valid (= its null-pointer check), B == 0 (the early FTR_OK),
every scalar check on its own, and pairs of bad arguments (which check answers first).  The 8-byte alignment checks of
the five duration-lattice workspaces sit behind a null check and cannot be reached with NULL pointers."""
import ctypes
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "capi_messages.json")
HUGE = 1 << 40   # a workspace size that passes every size check

# the values every call starts from (B=1 T=4 S=2 C=10 r=2, as tests/test_multiblank.py::_call), by parameter name
DEFAULTS = dict(B=1, T=4, S=2, C=10, r=2, S1=3, T1=4, s_range=2, rows=4, rows1=2, rows2=2, cols=4, kind=0, modified=0,
                termination_symbol=0, scale_stride=0, reduction=0, flags=0, overwrite_ans_grad=0, solution=0,
                D=2, Dx=2, Dy=1, N=2, p_floats=HUGE, workspace_floats=HUGE, workspace_bytes=HUGE)
HOST_PTR = ctypes.POINTER(ctypes.c_int32)   # the host arrays' argtype in tf_fast_rnnt/_lib.py (device pointers are void*)
HOST_ARRAYS = dict(durations=(1, 2), big_blank_ids=(1,), token_durations=(0, 1), blank_durations=(1,))

# single overrides, tried on every entry point that has the parameter(s)
SINGLES = [dict(B=0), dict(B=-1), dict(T=-1), dict(T=0), dict(S=-1), dict(S=0), dict(S=0, T=0), dict(C=0), dict(C=1), dict(r=0),
           dict(r=4), dict(S1=0), dict(T1=6), dict(s_range=0), dict(s_range=9), dict(rows=-1), dict(rows=0), dict(rows1=-1),
           dict(rows1=0, rows2=0), dict(cols=-1), dict(cols=0), dict(C=-1), dict(termination_symbol=-1),
           dict(termination_symbol=10), dict(scale_stride=2), dict(flags=2), dict(reduction=3), dict(modified=2),
           dict(modified=1, S=0), dict(modified=1, T=0), dict(workspace_floats=0), dict(workspace_bytes=0), dict(sigma=-1.0),
           dict(kind=7), dict(B=0, C=0), dict(B=1, reduction=3),
           # two bad arguments at once: which check answers first
           dict(B=-1, termination_symbol=-1), dict(termination_symbol=-1, scale_stride=2), dict(B=-1, scale_stride=2),
           dict(C=1, termination_symbol=5), dict(termination_symbol=-1, r=4), dict(B=0, termination_symbol=-1),
           dict(B=0, scale_stride=2), dict(B=0, r=4), dict(B=-1, flags=2), dict(flags=2, reduction=3), dict(B=0, flags=2),
           dict(B=0, reduction=3), dict(B=0, modified=2), dict(B=-1, modified=2), dict(B=0, workspace_floats=0),
           dict(B=0, workspace_bytes=0), dict(T=0, T1=9), dict(T1=9, s_range=0), dict(B=0, s_range=0), dict(B=0, sigma=-1.0),
           dict(r=4, sigma=-1.0), dict(B=-1, workspace_floats=0), dict(B=-1, workspace_bytes=0)]
# host-array cases (each entry point that has the named array)
ARRAYS = [dict(durations=None), dict(durations=(1, 2, 3, 4, 5, 6, 7, 8, 9), D=9), dict(D=0), dict(durations=(1, 2, 2), D=3),
          dict(durations=(0, 2)), dict(durations=(1, 33)), dict(durations=(2, 3)), dict(durations=(1,), D=1),
          dict(durations=(0,), N=1), dict(durations=(0, 1, 2, 3, 4, 5), N=6), dict(durations=(0, 17), N=2), dict(N=0),
          dict(big_blank_ids=None), dict(big_blank_ids=(10,)), dict(big_blank_ids=(0,)), dict(big_blank_ids=(3,), termination_symbol=3),
          dict(durations=(1, 2, 4), D=3, big_blank_ids=(5, 5)), dict(durations=(2, 3), B=-1), dict(D=0, B=-1),
          dict(big_blank_ids=(10,), B=-1), dict(termination_symbol=10, durations=(2, 3)),
          dict(token_durations=None), dict(blank_durations=None), dict(Dx=0), dict(Dy=0), dict(Dx=9), dict(token_durations=(1, 0)),
          dict(token_durations=(-1, 1)), dict(blank_durations=(0,)), dict(blank_durations=(17,)), dict(blank_durations=(33,)),
          dict(token_durations=(0, 1, 2, 3, 4), Dx=5, blank_durations=(1, 2, 3, 4, 5), Dy=5), dict(Dx=0, B=-1),
          dict(blank_durations=(0,), workspace_floats=0), dict(N=0, sigma=-1.0), dict(sigma=-1.0, termination_symbol=-1),
          dict(durations=(0, 1), termination_symbol=10, B=-1)]


def prototypes():
    """{name: [(type, parameter name), ...]} of include/ftr.h"""
    text = open(os.path.join(ROOT, "include", "ftr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(ftr_\w+)\s*\(([^()]*)\)\s*;", text):
        params = []
        for p in m.group(2).split(","):
            p = " ".join(p.split())
            if p and p != "void":
                typ, name = re.match(r"(.*?)(\w+)$", p).groups()
                params.append((typ.strip(), name))
        out[m.group(1)] = params
    return out


def build_args(params, argtypes, over):
    args, keep = [], []
    for (typ, name), at in zip(params, argtypes):
        if name in HOST_ARRAYS and at == HOST_PTR:
            vals = over.get(name, HOST_ARRAYS[name])
            arr = None if vals is None else (ctypes.c_int32 * max(len(vals), 1))(*vals)
            keep.append(arr)
            args.append(arr)
        elif name == "r_eff_out":
            keep.append(ctypes.c_int(0))
            args.append(ctypes.byref(keep[-1]))
        elif "*" in typ:
            args.append(None)            # every device pointer and the stream: NULL
        elif at in (ctypes.c_float, ctypes.c_double):
            args.append(float(over.get(name, 1.0 if at is ctypes.c_float else 0.0)))
        else:
            args.append(int(over.get(name, DEFAULTS[name])))
    return args, keep


def cases(L_signatures):
    """[(label, function name, overrides)] in a fixed order (ftr_normalizer_gemm_* do not clear the error text: order matters)"""
    out = []
    protos = prototypes()
    for name, (restype, argtypes) in L_signatures.items():
        params = protos[name]
        if not any("*" in t for t, _ in params):
            continue
        names = {n for (_, n), at in zip(params, argtypes) if n not in HOST_ARRAYS or at == HOST_PTR}
        table = [dict()] + [c for c in SINGLES + ARRAYS if set(c) <= names]
        for over in table:
            label = ",".join(f"{k}={over[k]}" for k in over).replace(" ", "") or "default"
            out.append((label, name, over))
    return out


def run(L, signatures):
    got = {}
    protos = prototypes()
    for label, name, over in cases(signatures):
        args, _keep = build_args(protos[name], signatures[name][1], over)
        rc = getattr(L, name)(*args)
        got.setdefault(name, {})[label] = [rc, L.ftr_last_error().decode("utf-8", "replace")]
    return got


def test_every_pointer_taking_entry_point_is_in_the_table(ft):
    protos = prototypes()
    assert set(protos) == set(ft._lib.EXPORTED_SYMBOLS)
    tabled = {name for _, name, _ in cases(ft._lib._SIGNATURES)}
    assert tabled == {n for n, ps in protos.items() if any("*" in t for t, _ in ps)}


def test_validation_replies_are_the_recorded_ones(ft):
    golden = json.load(open(GOLDEN))
    got = run(ft._lib.lib(), ft._lib._SIGNATURES)
    assert {(n, c) for n in got for c in got[n]} == {(n, c) for n in golden for c in golden[n]}
    for name in golden:
        for label, reply in golden[name].items():
            assert reply[0] in (0, 1), (name, label)     # no recorded case got past validation
            assert got[name][label] == reply, (name, label, got[name][label], reply)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tf-fast-rnnt_amd"))
    import tf_fast_rnnt as ft
    rec = run(ft._lib.lib(), ft._lib._SIGNATURES)
    bad = {(n, c): v for n in rec for c, v in rec[n].items() if v[0] not in (0, 1)}
    assert not bad, f"cases that got past validation: {bad}"
    with open(GOLDEN, "w") as f:   # one entry point per line
        f.write("{\n" + ",\n".join(f"{json.dumps(n)}:{json.dumps(rec[n], separators=(',', ':'))}" for n in rec) + "\n}\n")
    print(f"{sum(len(v) for v in rec.values())} cases from {ft._lib.LIB_PATH} -> {GOLDEN}")
