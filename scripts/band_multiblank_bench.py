"""Multi-blank loss on the band route against the lattice route, and against the ordinary pruned loss on its band route,
forward + backward: device-event timings after warm-up, the three candidates interleaved in one process in blocks of 10, the
median over all steps and the lowest and highest block median (the spread the route gate of DESIGN.md section 4l is judged
by).  One JSON line per config and big-blank set, appended to --out.

    python scripts/band_multiblank_bench.py --config c3 --config c5 [--reps 50] [--out profiles/band_multiblank_bench_c3_c5.jsonl]

Candidates:
  mb_band       rnnt_loss_multiblank_pruned, its default route here (the multi-blank domain of csrc/mi_band_tdt.hip and the
                band-shaped mb_* builders)
  mb_lattice    the same call with FTR_PRUNED_ROUTE=lattice: the full-size lattices of csrc/mi_multiblank.hip, the only route
                before
  pruned_band   rnnt_loss_pruned on the same logits, its band route (csrc/mi_band.hip)
Big-blank sets: () and the ids C-3, C-2, C-1 with durations 2, 4, 8.  Inputs are the seeded BASELINE inputs of bench.py with
the blank moved to column 0 and the symbols folded into 1..C-4, so that the last three columns are free for the big blanks
(a symbol that is a big blank has px = -inf); the prune ranges come from get_rnnt_prune_ranges on the occupancies of
rnnt_loss_simple on those inputs; the logits [B,T,r,C] are a seeded random tensor.  Each step asserts the route it was meant
to take (_lib.band_multiblank_recursions), and the two multi-blank routes must print the same loss to float32 rounding."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tf-fast-rnnt_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import tf_fast_rnnt as ft  # noqa: E402
from bench import CONFIGS, make_inputs  # noqa: E402

BLOCK = 10


def _time(fn, reps):
    ev = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1000.0 for a, b in ev]


def run(config, with_big, reps, warmup):
    B, T, S, C, r = CONFIGS[config]
    dev = torch.device("cuda:0")
    inp = make_inputs(B, T, S, C, seed=1000, device=dev)
    bd, blank = inp["boundary"], 0
    sym = (1 + inp["symbols"] % (C - 4)).to(torch.int32)
    _, (gx, gy) = ft.rnnt_loss_simple(inp["lm"], inp["am"], sym, blank, bd, reduction="sum", calc_gradients=True)
    ranges = ft.get_rnnt_prune_ranges(gx, gy, bd, r)
    del inp, gx, gy
    g = torch.Generator(device="cpu").manual_seed(2000)
    logits = torch.randn((B, T, r, C), generator=g, dtype=torch.float32).to(dev).requires_grad_(True)
    big = ((C - 3, 2), (C - 2, 4), (C - 1, 8)) if with_big else ()
    losses = {}

    def make(name, fn, route, band_calls):
        def step():
            if route is None:
                os.environ.pop("FTR_PRUNED_ROUTE", None)
            else:
                os.environ["FTR_PRUNED_ROUTE"] = route
            before = ft._lib.band_multiblank_recursions
            loss = fn()
            torch.autograd.grad(loss, logits)
            assert ft._lib.band_multiblank_recursions - before == band_calls, name
            losses[name] = loss
        return step

    mb = lambda: ft.rnnt_loss_multiblank_pruned(logits, sym, ranges, blank, big, bd)
    cands = {
        "mb_band": make("mb_band", mb, None, 1),
        "mb_lattice": make("mb_lattice", mb, "lattice", 0),
        "pruned_band": make("pruned_band", lambda: ft.rnnt_loss_pruned(logits, sym, ranges, blank, bd), None, 0),
    }
    for _ in range(warmup):
        for step in cands.values():
            step()
    torch.cuda.synchronize()
    blocks = {k: [] for k in cands}
    for _ in range((reps + BLOCK - 1) // BLOCK):
        for k, step in cands.items():
            blocks[k].append(_time(step, BLOCK))
    os.environ.pop("FTR_PRUNED_ROUTE", None)
    out = {"config": config, "B": B, "T": T, "S": S, "C": C, "s_range": r, "reps": reps, "big_blanks": big}
    for k, bl in blocks.items():
        meds = [statistics.median(b) for b in bl]
        out[k + "_us_median"] = round(statistics.median([v for b in bl for v in b]), 1)
        out[k + "_us_block_median_min"] = round(min(meds), 1)
        out[k + "_us_block_median_max"] = round(max(meds), 1)
        out[k + "_loss"] = float(losses[k].detach())
    out["lattice_over_band"] = round(out["mb_lattice_us_median"] / out["mb_band_us_median"], 3)
    out["band_over_pruned_band"] = round(out["mb_band_us_median"] / out["pruned_band_us_median"], 3)
    # the gate: the band route's slowest block against the lattice route's fastest
    out["band_beats_lattice_by_more_than_the_spread"] = out["mb_band_us_block_median_max"] < out["mb_lattice_us_block_median_min"]
    a, b = np.float32(out["mb_band_loss"]), np.float32(out["mb_lattice_loss"])
    out["routes_agree_to_float32_rounding"] = bool(np.isfinite(a) and abs(a - b) <= 2 * np.spacing(abs(a)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    agree = True
    for c in a.config or ["c3", "c5"]:
        for with_big in (False, True):
            res = run(c, with_big, a.reps, a.warmup)
            line = json.dumps(res)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            agree = agree and res["routes_agree_to_float32_rounding"]
    assert agree, "the band route and the lattice route print different losses"


if __name__ == "__main__":
    main()
