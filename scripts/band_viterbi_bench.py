"""Best-path alignment of the pruned joiner output on the band route against the lattice route: device-event timings after
warm-up, the candidates interleaved in one process in blocks of 10, the median over all calls and the lowest and highest
block median (the spread the route gate of DESIGN.md section 4m is judged by).  One JSON line per config and wrapper,
appended to --out.

    python scripts/band_viterbi_bench.py --config c3 --config c5 [--reps 50] [--out profiles/band_viterbi_bench_c3_c5.jsonl]

Wrappers and move lists:
  regular      rnnt_alignment_pruned, moves (0,) / (1,)
  tdt          rnnt_alignment_tdt_pruned, durations (0,1,2,3,4)
  multiblank   rnnt_alignment_multiblank_pruned, big blanks of 2, 4 and 8 frames (ids C-3, C-2, C-1; blank 0, symbols in 1..C-4)
Candidates, per wrapper:
  band         the wrapper on its default route here (band builder + csrc/mi_band_viterbi.hip)
  lattice      the same call with FTR_PRUNED_ROUTE=lattice: the lattice builder and csrc/mi_viterbi*.hip, the only route before
  chain_f32    mutual_information_viterbi_tdt_band alone on the band builder's operands (one launch)
  chain_f64    mutual_information_recursion_tdt_band, forward only, on the same operands and moves: the float64 log-add chain
               that the float32 select chain mirrors (a second yardstick, no gate)
Inputs are the seeded BASELINE inputs of bench.py; the prune ranges come from get_rnnt_prune_ranges on the occupancies of
rnnt_loss_simple; the logits are a seeded random tensor.  Each call asserts the route it was meant to take, and the two
routes are compared bit for bit once before timing."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tf-fast-rnnt_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import tf_fast_rnnt as ft  # noqa: E402
from bench import CONFIGS, make_inputs  # noqa: E402

rl = importlib.import_module("tf_fast_rnnt.rnnt_loss")   # the module: the package attribute of that name is the loss function

WRAPPERS = ("regular", "tdt", "multiblank")
TDT_DURATIONS = (0, 1, 2, 3, 4)
BIG_BLANK_DURATIONS = (2, 4, 8)
BLOCK = 10
ENTRY = "ftr_mutual_information_band_viterbi_f32"


def _time(fn, reps):
    ev = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1000.0 for a, b in ev]


def _setup(which, B, T, S, C, r, sym, ranges, bd, blank, dev):
    """(the wrapper call, (px_band, py_band, token durations, blank durations) of its band builder).  The operands of the
    two chain candidates have to be what the wrappers feed their kernel, and the package has no public band builder: they
    are made with the private helpers the wrappers themselves call (rnnt_loss._pruned_inputs, with a dummy logits tensor
    for its shape checks, _tdt_args / _tdt_band_builder_fwd, _big_blank_args / _mb_band_builder_fwd, _pruned_call).  A
    refactor of rnnt_loss.py that renames them has to follow here."""
    g = torch.Generator(device="cpu").manual_seed(2000)
    with torch.no_grad():
        sym, ranges, bd = rl._pruned_inputs(torch.empty((B, T, r, 1), device=dev), sym, ranges, bd)   # int32, contiguous
        if which == "tdt":
            logits = torch.randn((B, T, r, C + len(TDT_DURATIONS)), generator=g, dtype=torch.float32).to(dev)
            arr, durs, blk, Cc = rl._tdt_args(TDT_DURATIONS, blank, logits.shape[3])
            _, _, pxb, pyb = rl._tdt_band_builder_fwd(logits, sym, ranges, bd, blank, arr, durs, blk, Cc, 0.0, 0.0)
            return (lambda: ft.rnnt_alignment_tdt_pruned(logits, sym, ranges, blank, TDT_DURATIONS, bd)), (pxb, pyb, durs, blk)
        logits = torch.randn((B, T, r, C), generator=g, dtype=torch.float32).to(dev)
        if which == "multiblank":
            big = tuple(zip((C - 3, C - 2, C - 1), BIG_BLANK_DURATIONS))             # no symbol is one of them (run)
            ids_arr, durs_arr, dt = rl._big_blank_args(big, blank, C)
            _, pxb, pyb = rl._mb_band_builder_fwd(logits, sym, ranges, bd, blank, ids_arr, durs_arr, len(dt), 0.0, 0.0)
            return (lambda: ft.rnnt_alignment_multiblank_pruned(logits, sym, ranges, blank, big, bd)), (pxb.unsqueeze(1), pyb, (0,), dt)
        lse = torch.empty((B, T, r), dtype=torch.float32, device=dev)
        pxb, pyb = torch.empty_like(lse), torch.empty_like(lse)
        with torch.cuda.device(dev):
            rl._pruned_call("pruned_band_fwd", False, logits, (rl._ptr(sym), rl._ptr(ranges), rl._ptr(bd), int(blank), 0.0, rl._ptr(lse),
                            rl._ptr(pxb), rl._ptr(pyb), B, T, S, C, r, 0), (rl._stream_ptr(logits),))
        return (lambda: ft.rnnt_alignment_pruned(logits, sym, ranges, blank, bd)), (pxb.unsqueeze(1), pyb.unsqueeze(1), (0,), (1,))


def run(config, which, reps, warmup):
    B, T, S, C, r = CONFIGS[config]
    dev = torch.device("cuda:0")
    inp = make_inputs(B, T, S, C, seed=1000, device=dev)
    sym, bd, blank = inp["symbols"], inp["boundary"], inp["blank"]
    if which == "multiblank":   # as scripts/band_multiblank_bench.py: the blank in column 0, the last three columns free for the big blanks
        sym, blank = (1 + sym % (C - 4)).to(torch.int32), 0
    _, (gx, gy) = ft.rnnt_loss_simple(inp["lm"], inp["am"], sym, blank, bd, reduction="sum", calc_gradients=True)
    ranges = ft.get_rnnt_prune_ranges(gx, gy, bd, r)
    del inp, gx, gy
    call, (pxb, pyb, tok, blk) = _setup(which, B, T, S, C, r, sym, ranges, bd, blank, dev)
    names, real = [], ft._lib.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)
    ft._lib.call = spy
    outs = {}

    def routed(name, route, band_calls):
        def step():
            if route is None:
                os.environ.pop("FTR_PRUNED_ROUTE", None)
            else:
                os.environ["FTR_PRUNED_ROUTE"] = route
            del names[:]
            outs[name] = call()
            assert names.count(ENTRY) == band_calls, (name, names)
        return step

    cands = {
        "band": routed("band", None, 1),
        "lattice": routed("lattice", "lattice", 0),
        "chain_f32": lambda: ft.mutual_information_viterbi_tdt_band(pxb, pyb, ranges, tok, blk, bd, S=S),
        "chain_f64": lambda: ft.mutual_information_recursion_tdt_band(pxb, pyb, ranges, tok, blk, bd, S=S),
    }
    try:
        for _ in range(warmup):
            for step in cands.values():
                step()
        torch.cuda.synchronize()
        same = all(torch.equal(a.view(torch.int32) if a.is_floating_point() else a, b.view(torch.int32) if b.is_floating_point() else b)
                   for a, b in zip(outs["band"], outs["lattice"]))
        blocks = {k: [] for k in cands}
        for _ in range((reps + BLOCK - 1) // BLOCK):
            for k, step in cands.items():
                blocks[k].append(_time(step, BLOCK))
    finally:
        ft._lib.call = real
        os.environ.pop("FTR_PRUNED_ROUTE", None)
    score = outs["band"][0]
    out = {"config": config, "B": B, "T": T, "S": S, "C": C, "s_range": r, "reps": reps, "wrapper": which,
           "token_durations": tok, "blank_durations": blk, "routes_bit_identical": bool(same),
           "finite_scores": int(torch.isfinite(score).sum()), "score_sum": float(score[torch.isfinite(score)].sum())}
    for k, bl in blocks.items():
        meds = [statistics.median(b) for b in bl]
        out[k + "_us_median"] = round(statistics.median([v for b in bl for v in b]), 1)
        out[k + "_us_block_median_min"] = round(min(meds), 1)
        out[k + "_us_block_median_max"] = round(max(meds), 1)
    out["lattice_over_band"] = round(out["lattice_us_median"] / out["band_us_median"], 3)
    out["chain_f32_over_chain_f64"] = round(out["chain_f32_us_median"] / out["chain_f64_us_median"], 3)
    # the gate: the band route's slowest block against the lattice route's fastest
    out["band_beats_lattice_by_more_than_the_spread"] = out["band_us_block_median_max"] < out["lattice_us_block_median_min"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", choices=sorted(CONFIGS))
    ap.add_argument("--wrapper", action="append", choices=WRAPPERS)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    for c in a.config or ["c3", "c5"]:
        for which in a.wrapper or WRAPPERS:
            line = json.dumps(run(c, which, a.reps, a.warmup))
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
