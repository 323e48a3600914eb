"""TDT loss (rnnt_loss_tdt_pruned, durations 0..4: 5 token moves + 4 blank moves) against the multi-blank loss with durations
1..8 (1 token move + 8 blank moves): the same 9 moves per cell through the two row-per-lane recursions, forward + backward:
device-event timings after warm-up, the candidates alternated in one process, median of --reps.  One JSON line per config,
appended to --out.

    python scripts/tdt_bench.py --config c3 --config c5 [--reps 50] [--out profiles/tdt_bench_c3_c5.jsonl]

Inputs are the seeded BASELINE inputs of bench.py; the prune ranges come from get_rnnt_prune_ranges on the occupancies of
rnnt_loss_simple; the TDT logits [B,T,r,C+5] are a seeded random tensor and the multi-blank loss gets their first C
columns.  Under rocprofv3 --kernel-trace --stats the kernels to compare are mi_tdt_kernel<9, false|true> against
mi_multiblank_kernel<8, false|true>, tdt_lse_kernel + tdt_to_lattice_kernel against lse_rows* + mb_to_lattice_kernel, and
tdt_grad_kernel against mb_grad_kernel."""
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

DURATIONS = (0, 1, 2, 3, 4)
BIG_DURATIONS = (2, 3, 4, 5, 6, 7, 8)


def _time(fn, reps):
    ev = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1000.0 for a, b in ev]


def run(config, reps, warmup):
    B, T, S, C, r = CONFIGS[config]
    dev = torch.device("cuda:0")
    inp = make_inputs(B, T, S, C, seed=1000, device=dev)
    sym, bd, blank = inp["symbols"], inp["boundary"], inp["blank"]
    _, (gx, gy) = ft.rnnt_loss_simple(inp["lm"], inp["am"], sym, blank, bd, reduction="sum", calc_gradients=True)
    ranges = ft.get_rnnt_prune_ranges(gx, gy, bd, r)
    del inp, gx, gy
    big = tuple((1 + i, d) for i, d in enumerate(BIG_DURATIONS))
    sym = torch.where((sym >= 1) & (sym <= len(big)), sym + len(big), sym)   # no symbol is a big blank (its px would be -inf)
    g = torch.Generator(device="cpu").manual_seed(2000)
    wide = torch.randn((B, T, r, C + len(DURATIONS)), generator=g, dtype=torch.float32).to(dev)
    logits_tdt = wide.clone().requires_grad_(True)
    logits_mb = wide[..., :C].contiguous().requires_grad_(True)
    del wide
    losses = {}

    def make(name, fn, leaf):
        def step():
            loss = fn()
            torch.autograd.grad(loss, leaf)
            losses[name] = loss
        return step

    cands = {
        "multiblank_1_to_8": make("multiblank_1_to_8", lambda: ft.rnnt_loss_multiblank_pruned(logits_mb, sym, ranges, blank, big, bd), logits_mb),
        "tdt_0_to_4": make("tdt_0_to_4", lambda: ft.rnnt_loss_tdt_pruned(logits_tdt, sym, ranges, blank, DURATIONS, bd), logits_tdt),
    }
    for _ in range(warmup):
        for step in cands.values():
            step()
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for _ in range(reps // 10 + (reps % 10 > 0)):            # alternate in blocks of 10
        for k, step in cands.items():
            times[k] += _time(step, 10)
    out = {"config": config, "B": B, "T": T, "S": S, "C": C, "s_range": r, "reps": reps, "durations": DURATIONS,
           "big_blanks": big}
    for k, v in times.items():
        v = sorted(v[:reps])
        out[k + "_us_median"] = round(statistics.median(v), 1)
        out[k + "_us_min"] = round(v[0], 1)
        out[k + "_loss"] = float(losses[k].detach())
    out["tdt_over_multiblank"] = round(out["tdt_0_to_4_us_median"] / out["multiblank_1_to_8_us_median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    for c in a.config or ["c3", "c5"]:
        line = json.dumps(run(c, a.reps, a.warmup))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
