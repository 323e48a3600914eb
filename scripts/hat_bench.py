"""HAT loss (hat_loss_pruned, the ftr_hat_* kernels) against the ordinary pruned loss (rnnt_loss_pruned) on the same
logits, forward + backward: device-event timings after warm-up, the two alternated in one process.  One JSON line per
config.

    python scripts/hat_bench.py --config c3 [--config c5 ...] [--reps 50] [--rnnt-type regular|modified]

Inputs are the seeded BASELINE inputs of bench.py; the prune ranges come from get_rnnt_prune_ranges on the occupancies of
rnnt_loss_simple (so both losses take the band route), the logits [B,T,r,C] are a seeded random tensor.  Under rocprofv3
--kernel-trace --stats the per-kernel times of the <..., true> (HAT) and <..., false> instantiations of lse_rows*,
band_gather_kernel and band_grad_banded_kernel are the ones to compare."""
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


def _time(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    out = []
    for a, b in ev:
        a.record(); fn(); b.record()
        out.append((a, b))
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) * 1000.0 for a, b in out)


def run(config, reps, warmup, rnnt_type):
    B, T, S, C, r = CONFIGS[config]
    dev = torch.device("cuda:0")
    inp = make_inputs(B, T, S, C, seed=1000, device=dev)
    sym, bd, blank = inp["symbols"], inp["boundary"], inp["blank"]
    _, (gx, gy) = ft.rnnt_loss_simple(inp["lm"], inp["am"], sym, blank, bd, rnnt_type, reduction="sum", calc_gradients=True)
    ranges = ft.get_rnnt_prune_ranges(gx, gy, bd, r)
    del inp, gx, gy
    g = torch.Generator(device="cpu").manual_seed(2000)
    logits = torch.randn((B, T, r, C), generator=g, dtype=torch.float32).to(dev).requires_grad_(True)
    losses = {}

    def step(fn, name):
        loss = fn(logits, sym, ranges, blank, bd, rnnt_type, 0.0, "mean")
        torch.autograd.grad(loss, logits)
        losses[name] = loss

    ordinary = lambda: step(ft.rnnt_loss_pruned, "pruned")
    hat = lambda: step(ft.hat_loss_pruned, "hat")
    for _ in range(warmup):
        ordinary(); hat()
    torch.cuda.synchronize()
    tp, th = [], []
    for _ in range(reps // 10 + (reps % 10 > 0)):            # alternate in blocks of 10
        tp += _time(ordinary, 10)
        th += _time(hat, 10)
    tp.sort(); th.sort()
    med = lambda x: x[len(x) // 2]
    return {
        "config": config, "B": B, "T": T, "S": S, "C": C, "s_range": r, "rnnt_type": rnnt_type, "reps": len(tp),
        "pruned_fwd_bwd_us_median": round(med(tp), 2), "pruned_fwd_bwd_us_min": round(tp[0], 2),
        "hat_fwd_bwd_us_median": round(med(th), 2), "hat_fwd_bwd_us_min": round(th[0], 2),
        "hat_over_pruned_median": round(med(th) / med(tp), 4),
        "pruned_loss": float(losses["pruned"]), "hat_loss": float(losses["hat"]),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rnnt-type", default="regular", choices=["regular", "modified"])
    args = ap.parse_args()
    for c in args.config or ["c3"]:
        print(json.dumps(run(c, max(args.reps, 10), args.warmup, args.rnnt_type)), flush=True)


if __name__ == "__main__":
    main()
