"""The mixed TDT / ordinary loss (rnnt_loss_tdt_mixed_pruned, omega = 0.1) against what a caller had to write before it, and
against the TDT loss alone, forward + backward: device-event timings after warm-up, the candidates interleaved in one process
in blocks of 10, the median over all steps and the lowest and highest block median; the peak of torch's allocator above the
inputs during one step of each candidate.  One JSON line per config and duration list, appended to --out.

    python scripts/tdt_mix_bench.py --config c3 --config c5 [--reps 50] [--out profiles/tdt_mix_bench_c3_c5.jsonl]

Candidates:
  mixed         rnnt_loss_tdt_mixed_pruned(x, ..., omega)
  composition   (1 - omega) * rnnt_loss_tdt_pruned(x) + omega * rnnt_loss_pruned(x[..., :C].contiguous()), the slice taken
                inside the step: what the docstring of rnnt_loss_tdt_pruned told users to do
  tdt_only      rnnt_loss_tdt_pruned(x)
Inputs and ranges are those of scripts/band_tdt_bench.py: the seeded BASELINE inputs of bench.py, prune ranges from
get_rnnt_prune_ranges on the occupancies of rnnt_loss_simple, a seeded random TDT logits tensor [B,T,r,C+N].  Every step
asserts that it took the band route (_lib.band_tdt_recursions).

What the lines are judged by: `mixed`'s highest block median below `composition`'s lowest; the
memory saved at least 2 * 4 * B*T*r*C bytes (the copy of the token columns and its gradient).  `mixed - tdt_only` is
recorded without a gate."""
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
OMEGA = 0.1


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
    os.environ.pop("FTR_PRUNED_ROUTE", None)
    inp = make_inputs(B, T, S, C, seed=1000, device=dev)
    sym, bd, blank = inp["symbols"], inp["boundary"], inp["blank"]
    _, (gx, gy) = ft.rnnt_loss_simple(inp["lm"], inp["am"], sym, blank, bd, reduction="sum", calc_gradients=True)
    ranges = ft.get_rnnt_prune_ranges(gx, gy, bd, r)
    del inp, gx, gy
    g = torch.Generator(device="cpu").manual_seed(2000)
    x = torch.randn((B, T, r, C + len(durations)), generator=g, dtype=torch.float32).to(dev).requires_grad_(True)
    losses = {}

    def make(name, fn):
        def step():
            before = ft._lib.band_tdt_recursions
            loss = fn()
            grad, = torch.autograd.grad(loss, x)
            assert ft._lib.band_tdt_recursions - before == 1, name
            losses[name] = loss
            return grad
        return step

    tdt = lambda: ft.rnnt_loss_tdt_pruned(x, sym, ranges, blank, durations, bd)
    cands = {
        "mixed": make("mixed", lambda: ft.rnnt_loss_tdt_mixed_pruned(x, sym, ranges, blank, durations, OMEGA, bd)),
        "composition": make("composition", lambda: (1.0 - OMEGA) * tdt() + OMEGA * ft.rnnt_loss_pruned(x[..., :C].contiguous(), sym, ranges, blank, bd)),
        "tdt_only": make("tdt_only", tdt),
    }
    for _ in range(warmup):
        for step in cands.values():
            step()
    torch.cuda.synchronize()
    # the two ways to the same gradient agree (not a test: tests/test_gpu_tdt_mix.py holds both to float64)
    ga, gb = cands["mixed"](), cands["composition"]()
    agree = float((ga - gb).abs().max() / gb.abs().max())
    del ga, gb
    peak = {}
    for k, step in cands.items():       # the allocator's peak above what is held between steps (inputs, ranges, logits)
        losses.clear()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        step()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated(dev) - base
    blocks = {k: [] for k in cands}
    for _ in range((reps + BLOCK - 1) // BLOCK):
        for k, step in cands.items():
            blocks[k].append(_time(step, BLOCK))
    out = {"config": config, "B": B, "T": T, "S": S, "C": C, "s_range": r, "reps": reps, "durations": durations, "omega": OMEGA}
    for k, bl in blocks.items():
        meds = [statistics.median(b) for b in bl]
        out[k + "_us_median"] = round(statistics.median([v for b in bl for v in b]), 1)
        out[k + "_us_block_median_min"] = round(min(meds), 1)
        out[k + "_us_block_median_max"] = round(max(meds), 1)
        out[k + "_loss"] = float(losses[k].detach())
        out[k + "_peak_bytes_above_inputs"] = int(peak[k])
    out["mixed_vs_composition_grad_max_rel"] = agree
    out["composition_over_mixed"] = round(out["composition_us_median"] / out["mixed_us_median"], 3)
    out["mixed_minus_tdt_only_us"] = round(out["mixed_us_median"] - out["tdt_only_us_median"], 1)
    # the time rule: the new function's slowest block against the composition's fastest
    out["mixed_beats_composition_by_more_than_the_spread"] = out["mixed_us_block_median_max"] < out["composition_us_block_median_min"]
    out["memory_saved_bytes"] = int(peak["composition"] - peak["mixed"])
    out["memory_saved_bound_bytes"] = 2 * 4 * B * T * r * C       # the copy of the token columns and its gradient
    out["memory_saved_meets_bound"] = out["memory_saved_bytes"] >= out["memory_saved_bound_bytes"]
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
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
