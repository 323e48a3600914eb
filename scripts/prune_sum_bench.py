"""do_rnnt_pruning_sum against the unfused pair: forward + backward of
    a      sum(do_rnnt_pruning(am, lm, ranges))          float32 (the gather, then the joiner's addition)
    f32    do_rnnt_pruning_sum(am, lm, ranges)            float32
    bf16   do_rnnt_pruning_sum(am, lm, ranges)            bfloat16
    fp16   do_rnnt_pruning_sum(am, lm, ranges)            float16
on the same values: device-event timings after warm-up, the four arms interleaved in blocks of ten steps in one process.
One JSON line per config.

    python scripts/prune_sum_bench.py --config c3 [--config c4 --config c5] [--reps 60] [--out profiles/prune_sum_bench_c3_c4_c5.jsonl]
    python scripts/prune_sum_bench.py --config c3 --only bf16 --reps 20     (one arm: the form to run under rocprofv3
                                                                               --kernel-trace --stats, one run per arm)

am and lm are the seeded BASELINE inputs of bench.py rounded to bfloat16 and then to float16 precision (representable in all
three types); the prune ranges come from get_rnnt_prune_ranges on the occupancies of rnnt_loss_simple on the unrounded inputs,
as in bench.py (bands).  A step is the forward and torch.autograd.grad of the result towards am and lm with a fixed upstream
gradient of the result's dtype.  Timings on another box or in another session differ by more than the differences of
interest: arm `a` of the same run is the yardstick.  peak_mb: torch.cuda.max_memory_allocated over one step, inputs and the
upstream gradient included.  The gates (each by the rule that the slowest block median of the one lies below the fastest
block median of the other): f32 faster than a; bf16 and fp16 no slower than f32, that is, f32 is not faster than they are
by that rule."""
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

ARMS = {"a": torch.float32, "f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def _time(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1000.0 for a, b in ev]


def run(config, reps, warmup, only):
    B, T, S, C, r = CONFIGS[config]
    dev = torch.device("cuda:0")
    inp = make_inputs(B, T, S, C, seed=1000, device=dev)
    _, (gx, gy) = ft.rnnt_loss_simple(inp["lm"], inp["am"], inp["symbols"], inp["blank"], inp["boundary"], "regular", reduction="sum",
                                      calc_gradients=True)
    ranges = ft.get_rnnt_prune_ranges(gx, gy, inp["boundary"], r)
    round3 = lambda t: t.to(torch.bfloat16).to(torch.float16).float()
    am32, lm32 = round3(inp["am"]), round3(inp["lm"])
    del inp, gx, gy
    g = torch.Generator(device="cpu").manual_seed(2000)
    w32 = round3(torch.randn((B, T, r, C), generator=g, dtype=torch.float32).to(dev))
    names = [only] if only else list(ARMS)
    out = {"config": config, "B": B, "T": T, "S": S, "C": C, "s_range": r, "elements": B * T * r * C}
    steps = {}
    for n in names:
        dt = ARMS[n]
        am = am32.to(dt).requires_grad_(True); lm = lm32.to(dt).requires_grad_(True)
        w = w32 if dt == torch.float32 else w32.to(dt)

        def step(n=n, am=am, lm=lm, w=w):
            z = sum(ft.do_rnnt_pruning(am, lm, ranges)) if n == "a" else ft.do_rnnt_pruning_sum(am, lm, ranges)
            return torch.autograd.grad(z, (am, lm), w)
        steps[n] = step
    for n in names:                                                 # peak memory of one step, before any timing
        torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        steps[n]()
        torch.cuda.synchronize()
        out[f"{n}_peak_mb"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
        out[f"{n}_peak_above_resident_mb"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
    for _ in range(warmup):
        for n in names:
            steps[n]()
    torch.cuda.synchronize()
    times = {n: [] for n in names}
    for _ in range(reps // 10 + (reps % 10 > 0)):                   # interleaved in blocks of 10
        for n in names:
            times[n] += _time(steps[n], 10)
    med = lambda v: sorted(v)[len(v) // 2]
    out["reps"] = len(times[names[0]])
    blocks = {}
    for n in names:
        out[f"{n}_fwd_bwd_us_median"] = round(med(times[n]), 2)
        blocks[n] = [med(times[n][i:i + 10]) for i in range(0, len(times[n]), 10)]
        out[f"{n}_block_median_us_min_max"] = [round(min(blocks[n]), 2), round(max(blocks[n]), 2)]
    if not only:
        out["gate_f32_faster_than_a"] = max(blocks["f32"]) < min(blocks["a"])
        for n in ("bf16", "fp16"):
            out[f"gate_{n}_no_slower_than_f32"] = not (max(blocks["f32"]) < min(blocks[n]))
            out[f"{n}_faster_than_f32"] = max(blocks[n]) < min(blocks["f32"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=sorted(ARMS), help="time one arm only (profiler runs)")
    ap.add_argument("--out", help="append the JSON lines to this file as well")
    args = ap.parse_args()
    for c in args.config or ["c3"]:
        line = json.dumps(run(c, max(args.reps, 10), args.warmup, args.only))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
