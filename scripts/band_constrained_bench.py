"""rnnt_loss_pruned(rnnt_type="constrained") on the band route against the lattice route, and against the modified type on
its band route, forward + backward: device-event timings after warm-up, the three candidates interleaved in one process in
blocks of 10, the median over all steps and the lowest and highest block median (the spread the route gate of DESIGN.md
section 4v is judged by), and the peak of allocated memory of one step above the inputs.  One JSON line per config and
dtype, appended to --out.

    python scripts/band_constrained_bench.py --config c3 --config c5 [--reps 50] [--out profiles/band_constrained_bench_c3_c5.jsonl]

Candidates:
  constrained_band     the call on its default route here: the frame-group builder of csrc/pruned_constrained.hip, the band
                       recursion of csrc/mi_band.hip (modified = 1), one gradient launch
  constrained_lattice  the same call with FTR_PRUNED_ROUTE=lattice: the full-size lattices, torch's px + py[:, 1:] and penalty,
                       the generic recursion and autograd's replay -- the only route before
  modified_band        rnnt_type="modified" on the same inputs, its band route (lse_rows + band_gather, the same recursion)
Inputs are the seeded BASELINE inputs of bench.py; the prune ranges come from get_rnnt_prune_ranges on the occupancies of
rnnt_loss_simple(rnnt_type="constrained"); the logits [B,T,r,C] are a seeded random tensor in the dtype."""
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

DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16}
BLOCK = 10


def _time(fn, reps):
    ev = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1000.0 for a, b in ev]


def run(config, dtype, reps, warmup):
    B, T, S, C, r = CONFIGS[config]
    dev = torch.device("cuda:0")
    inp = make_inputs(B, T, S, C, seed=1000, device=dev)
    sym, bd, blank = inp["symbols"], inp["boundary"], inp["blank"]
    _, (gx, gy) = ft.rnnt_loss_simple(inp["lm"], inp["am"], sym, blank, bd, rnnt_type="constrained", reduction="sum",
                                      calc_gradients=True)      # the first pass of a constrained recipe: a band this type can walk
    ranges = ft.get_rnnt_prune_ranges(gx, gy, bd, r)
    del inp, gx, gy
    g = torch.Generator(device="cpu").manual_seed(2000)
    logits = torch.randn((B, T, r, C), generator=g, dtype=torch.float32).to(dev).to(DTYPES[dtype]).requires_grad_(True)
    losses = {}

    def make(name, rnnt_type, route):
        def step():
            if route is None:
                os.environ.pop("FTR_PRUNED_ROUTE", None)
            else:
                os.environ["FTR_PRUNED_ROUTE"] = route
            loss = ft.rnnt_loss_pruned(logits, sym, ranges, blank, bd, rnnt_type=rnnt_type, delay_penalty=0.01)
            torch.autograd.grad(loss, logits)
            losses[name] = loss
        return step

    cands = {
        "constrained_band": make("constrained_band", "constrained", None),
        "constrained_lattice": make("constrained_lattice", "constrained", "lattice"),
        "modified_band": make("modified_band", "modified", None),
    }
    for _ in range(warmup):
        for step in cands.values():
            step()
    torch.cuda.synchronize()
    blocks = {k: [] for k in cands}
    for _ in range((reps + BLOCK - 1) // BLOCK):
        for k, step in cands.items():
            blocks[k].append(_time(step, BLOCK))
    out = {"config": config, "B": B, "T": T, "S": S, "C": C, "s_range": r, "reps": reps, "dtype": dtype}
    loss_values = {k: float(v.detach()) for k, v in losses.items()}
    losses.clear()
    for k, bl in blocks.items():
        meds = [statistics.median(b) for b in bl]
        out[k + "_us_median"] = round(statistics.median([v for b in bl for v in b]), 1)
        out[k + "_us_block_median_min"] = round(min(meds), 1)
        out[k + "_us_block_median_max"] = round(max(meds), 1)
        out[k + "_loss"] = loss_values[k]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        cands[k]()
        losses.clear()
        torch.cuda.synchronize()
        out[k + "_peak_bytes_above_inputs"] = int(torch.cuda.max_memory_allocated(dev) - base)
    os.environ.pop("FTR_PRUNED_ROUTE", None)
    out["lattice_over_band"] = round(out["constrained_lattice_us_median"] / out["constrained_band_us_median"], 3)
    out["constrained_over_modified"] = round(out["constrained_band_us_median"] / out["modified_band_us_median"], 3)
    # the gate: the band route's slowest block against the lattice route's fastest
    out["band_beats_lattice_by_more_than_the_spread"] = out["constrained_band_us_block_median_max"] < out["constrained_lattice_us_block_median_min"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", choices=sorted(CONFIGS))
    ap.add_argument("--dtype", action="append", choices=sorted(DTYPES))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    for c in a.config or ["c3", "c5"]:
        for dtype in a.dtype or ["float32", "bfloat16"]:
            line = json.dumps(run(c, dtype, a.reps, a.warmup))
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
