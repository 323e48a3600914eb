"""The pruned loss (rnnt_loss_pruned, forward + backward) on float32, bfloat16 and float16 joiner logits holding the same
values: device-event timings after warm-up, the three dtypes interleaved in one process.  One JSON line per config.

    python scripts/lowp_bench.py --config c3 [--config c4 --config c5] [--reps 60] [--out profiles/lowp_bench_c3_c4_c5.jsonl]
    python scripts/lowp_bench.py --config c3 --only bf16 --reps 20     (one dtype: the form to run under rocprofv3
                                                                          --kernel-trace --stats, one run per dtype)

Inputs are the seeded BASELINE inputs of bench.py; the prune ranges come from get_rnnt_prune_ranges on the occupancies of
rnnt_loss_simple (the band route), the logits [B,T,r,C] are a seeded random tensor rounded to bfloat16 and then to float16
precision, so the three runs see the same numbers.  The float32 step of the same run is the yardstick; timings on
another box or in another session differ by more than the differences of interest.  The stream kernels to compare under
the profiler are the <float | bf16_t | fp16_t, ...> instantiations of lse_rows_reg_kernel, band_gather_kernel and
band_grad_banded_kernel.  peak_mb: torch.cuda.max_memory_allocated over one forward + backward, logits included."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tf-fast-rnnt_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import tf_fast_rnnt as ft  # noqa: E402
from bench import CONFIGS, make_inputs  # noqa: E402

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def _time(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1000.0 for a, b in ev]


def run(config, reps, warmup, rnnt_type, only):
    B, T, S, C, r = CONFIGS[config]
    dev = torch.device("cuda:0")
    inp = make_inputs(B, T, S, C, seed=1000, device=dev)
    sym, bd, blank = inp["symbols"], inp["boundary"], inp["blank"]
    _, (gx, gy) = ft.rnnt_loss_simple(inp["lm"], inp["am"], sym, blank, bd, rnnt_type, reduction="sum", calc_gradients=True)
    ranges = ft.get_rnnt_prune_ranges(gx, gy, bd, r)
    del inp, gx, gy
    g = torch.Generator(device="cpu").manual_seed(2000)
    base = torch.randn((B, T, r, C), generator=g, dtype=torch.float32).to(dev)
    base = base.to(torch.bfloat16).to(torch.float16).float()       # representable in all three types
    names = [only] if only else list(DTYPES)
    out = {"config": config, "B": B, "T": T, "S": S, "C": C, "s_range": r, "rnnt_type": rnnt_type}
    times = {n: [] for n in names}
    steps = {}
    for n in names:
        x = base.to(DTYPES[n]).requires_grad_(True)

        def step(x=x, n=n):
            loss = ft.rnnt_loss_pruned(x, sym, ranges, blank, bd, rnnt_type, 0.0, "mean")
            torch.autograd.grad(loss, x)
            return loss
        steps[n] = step
    del base
    for n in names:                                                 # peak memory of one step, before any timing
        torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        out[f"{n}_loss"] = float(steps[n]())
        torch.cuda.synchronize()
        out[f"{n}_peak_mb"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    for _ in range(warmup):
        for n in names:
            steps[n]()
    torch.cuda.synchronize()
    for _ in range(reps // 10 + (reps % 10 > 0)):                   # interleaved in blocks of 10
        for n in names:
            times[n] += _time(steps[n], 10)
    med = lambda v: sorted(v)[len(v) // 2]
    out["reps"] = len(times[names[0]])
    for n in names:
        out[f"{n}_fwd_bwd_us_median"] = round(med(times[n]), 2)
        out[f"{n}_fwd_bwd_us_min"] = round(min(times[n]), 2)
        # spread of the block medians: what one run of 10 steps moves by inside this process
        blocks = [med(times[n][i:i + 10]) for i in range(0, len(times[n]), 10)]
        out[f"{n}_block_median_us_min_max"] = [round(min(blocks), 2), round(max(blocks), 2)]
        if n != "f32" and "f32" in times:
            out[f"{n}_over_f32_median"] = round(med(times[n]) / med(times["f32"]), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rnnt-type", default="regular", choices=["regular", "modified"])
    ap.add_argument("--only", choices=sorted(DTYPES), help="time one dtype only (profiler runs)")
    ap.add_argument("--out", help="append the JSON lines to this file as well")
    args = ap.parse_args()
    for c in args.config or ["c3"]:
        line = json.dumps(run(c, max(args.reps, 10), args.warmup, args.rnnt_type, args.only))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
