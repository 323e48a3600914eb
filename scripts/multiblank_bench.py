"""Multi-blank transducer loss (rnnt_loss_multiblank_pruned) against the ordinary pruned loss forced to the lattice route
(the route the multi-blank loss takes), forward + backward: device-event timings after warm-up, the candidates alternated
in one process, median of --reps.  One JSON line per config, appended to --out.

    python scripts/multiblank_bench.py --config c3 --config c5 [--reps 50] [--out profiles/multiblank_bench_c3_c5.jsonl]

Candidates: rnnt_loss_pruned with FTR_PRUNED_ROUTE=lattice; rnnt_loss_multiblank_pruned with big_blanks=(); the same
with durations 2, 4, 8 on columns 1, 2, 3.  Inputs are the seeded BASELINE inputs of bench.py; the prune ranges come from
get_rnnt_prune_ranges on the occupancies of rnnt_loss_simple, the logits [B,T,r,C] are a seeded random tensor.  Under
rocprofv3 --kernel-trace --stats the kernels to compare are mb_to_lattice_kernel / mb_grad_kernel against
band_to_lattice_kernel / band_grad_kernel, and mi_multiblank_kernel<D, false|true> against mi_bidir_fwd_kernel / bwd."""
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
    sym = torch.where((sym >= 1) & (sym <= 3), sym + 3, sym)   # no symbol is a big blank (its px would be -inf)
    g = torch.Generator(device="cpu").manual_seed(2000)
    logits = torch.randn((B, T, r, C), generator=g, dtype=torch.float32).to(dev).requires_grad_(True)
    big = tuple((c, d) for c, d in ((1, 2), (2, 4), (3, 8)) if c != blank)
    os.environ["FTR_PRUNED_ROUTE"] = "lattice"
    losses = {}

    def make(name, fn):
        def step():
            loss = fn()
            torch.autograd.grad(loss, logits)
            losses[name] = loss
        return step

    cands = {
        "pruned_lattice": make("pruned_lattice", lambda: ft.rnnt_loss_pruned(logits, sym, ranges, blank, bd)),
        "multiblank_none": make("multiblank_none", lambda: ft.rnnt_loss_multiblank_pruned(logits, sym, ranges, blank, (), bd)),
        "multiblank_2_4_8": make("multiblank_2_4_8", lambda: ft.rnnt_loss_multiblank_pruned(logits, sym, ranges, blank, big, bd)),
    }
    for _ in range(warmup):
        for step in cands.values():
            step()
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for _ in range(reps // 10 + (reps % 10 > 0)):            # alternate in blocks of 10
        for k, step in cands.items():
            times[k] += _time(step, 10)
    out = {"config": config, "B": B, "T": T, "S": S, "C": C, "s_range": r, "reps": reps, "big_blanks": big}
    for k, v in times.items():
        v = sorted(v[:reps])
        out[k + "_us_median"] = round(statistics.median(v), 1)
        out[k + "_us_min"] = round(v[0], 1)
        out[k + "_loss"] = float(losses[k].detach())
    base = out["pruned_lattice_us_median"]
    out["multiblank_none_over_pruned_lattice"] = round(out["multiblank_none_us_median"] / base, 3)
    out["multiblank_2_4_8_over_pruned_lattice"] = round(out["multiblank_2_4_8_us_median"] / base, 3)
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
