"""do_rnnt_pruning_act against the activation applied by torch: forward + backward, per dtype (f32, bf16, fp16) and
activation (tanh, relu), of
    a      torch.<act>(do_rnnt_pruning_sum(am, lm, ranges))        the fused sum, then torch's activation
    b      do_rnnt_pruning_act(am, lm, ranges, activation=<act>)    one operation each way
    a0     torch.<act>(sum(do_rnnt_pruning(am, lm, ranges)))        float32 only: nothing fused
on the same values: device-event timings after warm-up, all arms interleaved in blocks of ten steps in one process.
One JSON line per config.

    python scripts/joiner_act_bench.py --config c3 [--config c4 --config c5] [--reps 60] [--out profiles/joiner_act_bench_c3_c4_c5.jsonl]
    python scripts/joiner_act_bench.py --config c3 --only b_bf16_tanh --reps 20     (one arm: the form to run under rocprofv3
                                                                                      --kernel-trace --stats, one run per arm)

Inputs, ranges, the upstream gradient and the meaning of a step, of peak_mb and of a gate are those of
scripts/prune_sum_bench.py.  The gate, per dtype and activation: b's slowest block median lies below a's fastest.  The
forward alone is timed as well (20 calls per arm, after the steps), to tell the activation's arithmetic from the backward."""
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
ACTS = {"tanh": torch.tanh, "relu": torch.relu}
ARMS = [f"{k}_{d}_{a}" for d in DTYPES for a in ACTS for k in ("a", "b")] + [f"a0_f32_{a}" for a in ACTS]


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
    leaves = {d: (am32.to(dt).requires_grad_(True), lm32.to(dt).requires_grad_(True), w32.to(dt)) for d, dt in DTYPES.items()
              if any(n.split("_")[1] == d for n in names)}
    fwds, steps = {}, {}
    for n in names:
        kind, d, act = n.split("_")
        am, lm, w = leaves[d]

        def fwd(kind=kind, act=act, am=am, lm=lm):
            if kind == "b":
                return ft.do_rnnt_pruning_act(am, lm, ranges, activation=act)
            return ACTS[act](ft.do_rnnt_pruning_sum(am, lm, ranges) if kind == "a" else sum(ft.do_rnnt_pruning(am, lm, ranges)))
        fwds[n] = fwd
        steps[n] = lambda fwd=fwd, am=am, lm=lm, w=w: torch.autograd.grad(fwd(), (am, lm), w)
    for n in names:                                                 # peak memory of one step, before any timing
        torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        steps[n]()
        torch.cuda.synchronize()
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
    with torch.no_grad():
        for n in names:
            out[f"{n}_fwd_only_us_median"] = round(med(_time(fwds[n], 20)), 2)
    if not only:
        for d in DTYPES:
            for act in ACTS:
                out[f"gate_{d}_{act}_b_faster_than_a"] = max(blocks[f"b_{d}_{act}"]) < min(blocks[f"a_{d}_{act}"])
                out[f"ratio_{d}_{act}_b_over_a"] = round(med(times[f"b_{d}_{act}"]) / med(times[f"a_{d}_{act}"]), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=ARMS, help="time one arm only (profiler runs)")
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
