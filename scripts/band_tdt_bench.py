"""TDT loss on the band route against the lattice route, and against the ordinary pruned loss on its band route, forward +
backward: device-event timings after warm-up, the three candidates interleaved in one process in blocks of 10, the median
over all steps and the lowest and highest block median (the spread the route gate of DESIGN.md section 4k is judged by).  One JSON
line per config and duration list, appended to --out.

    python scripts/band_tdt_bench.py --config c3 --config c5 [--reps 50] [--out profiles/band_tdt_bench_c3_c5.jsonl]

Candidates:
  tdt_band      rnnt_loss_tdt_pruned, its default route here (csrc/mi_band_tdt.hip and the band-shaped builders)
  tdt_lattice   the same call with FTR_PRUNED_ROUTE=lattice: the full-size lattices of csrc/mi_tdt.hip, the only route before
  pruned_band   rnnt_loss_pruned on the first C columns of the same logits, its band route (csrc/mi_band.hip)
Inputs are the seeded BASELINE inputs of bench.py; the prune ranges come from get_rnnt_prune_ranges on the occupancies of
rnnt_loss_simple; the TDT logits [B,T,r,C+N] are a seeded random tensor.  Each step asserts the route it was meant to
take (_lib.band_tdt_recursions)."""
import argparse
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

DURATION_LISTS = ((0, 1), (0, 1, 2, 3, 4))
BLOCK = 10


def _time(fn, reps):
    ev = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1000.0 for a, b in ev]


def run(config, durations, reps, warmup):
    B, T, S, C, r = CONFIGS[config]
    dev = torch.device("cuda:0")
    inp = make_inputs(B, T, S, C, seed=1000, device=dev)
    sym, bd, blank = inp["symbols"], inp["boundary"], inp["blank"]
    _, (gx, gy) = ft.rnnt_loss_simple(inp["lm"], inp["am"], sym, blank, bd, reduction="sum", calc_gradients=True)
    ranges = ft.get_rnnt_prune_ranges(gx, gy, bd, r)
    del inp, gx, gy
    g = torch.Generator(device="cpu").manual_seed(2000)
    wide = torch.randn((B, T, r, C + len(durations)), generator=g, dtype=torch.float32).to(dev)
    logits_tdt = wide.clone().requires_grad_(True)
    logits_plain = wide[..., :C].contiguous().requires_grad_(True)
    del wide
    losses = {}

    def make(name, fn, leaf, route, band_calls):
        def step():
            if route is None:
                os.environ.pop("FTR_PRUNED_ROUTE", None)
            else:
                os.environ["FTR_PRUNED_ROUTE"] = route
            before = ft._lib.band_tdt_recursions
            loss = fn()
            torch.autograd.grad(loss, leaf)
            assert ft._lib.band_tdt_recursions - before == band_calls, name
            losses[name] = loss
        return step

    tdt = lambda: ft.rnnt_loss_tdt_pruned(logits_tdt, sym, ranges, blank, durations, bd)
    cands = {
        "tdt_band": make("tdt_band", tdt, logits_tdt, None, 1),
        "tdt_lattice": make("tdt_lattice", tdt, logits_tdt, "lattice", 0),
        "pruned_band": make("pruned_band", lambda: ft.rnnt_loss_pruned(logits_plain, sym, ranges, blank, bd), logits_plain, None, 0),
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
    out = {"config": config, "B": B, "T": T, "S": S, "C": C, "s_range": r, "reps": reps, "durations": durations}
    for k, bl in blocks.items():
        meds = [statistics.median(b) for b in bl]
        out[k + "_us_median"] = round(statistics.median([v for b in bl for v in b]), 1)
        out[k + "_us_block_median_min"] = round(min(meds), 1)
        out[k + "_us_block_median_max"] = round(max(meds), 1)
        out[k + "_loss"] = float(losses[k].detach())
    out["lattice_over_band"] = round(out["tdt_lattice_us_median"] / out["tdt_band_us_median"], 3)
    out["band_over_pruned_band"] = round(out["tdt_band_us_median"] / out["pruned_band_us_median"], 3)
    # the gate: the band route's slowest block against the lattice route's fastest
    out["band_beats_lattice_by_more_than_the_spread"] = out["tdt_band_us_block_median_max"] < out["tdt_lattice_us_block_median_min"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    for c in a.config or ["c3", "c5"]:
        for durations in DURATION_LISTS:
            line = json.dumps(run(c, durations, a.reps, a.warmup))
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
