"""rnnt_loss_pruned_kd against what a distillation step had to call before it, forward + backward of loss + 0.5 * kd on the
same tensors: device-event timings after warm-up, the two candidates interleaved in one process in blocks of 10, the median
over all steps and the lowest and highest block median; the peak of torch's allocator above the inputs during one step of
each.  One JSON line per config, dtype, mode and temperature, appended to --out.

    python scripts/kd_loss_bench.py --config c3 --config c4 --config c5 [--reps 50] [--out profiles/kd_loss_bench_c3_c4_c5.jsonl]

Candidates:
  fused         loss, kd = rnnt_loss_pruned_kd(x, y, ...); loss + 0.5 * kd
  composition   rnnt_loss_pruned(x, ...) + 0.5 * rnnt_kd_loss_pruned(x, y, ...)
Inputs and ranges are those of scripts/tdt_mix_bench.py: the seeded BASELINE inputs of bench.py, prune ranges from
get_rnnt_prune_ranges on the occupancies of rnnt_loss_simple, seeded random student and teacher logits [B,T,r,C] in one
dtype.  Every fused step is checked to have taken the fused route (the entry of include/ftr_kd_loss.h was called).

What the lines are judged by: `fused`'s highest block median below `composition`'s lowest.  The
memory difference is recorded next to what was expected of it, one tensor of the size of `logits`, without a gate."""
import argparse
import contextlib
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

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
MODES = ("full", "collapsed")
TEMPERATURES = (1.0, 2.0)
BLOCK = 10
LAM = 0.5


def _time(fn, reps):
    ev = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1000.0 for a, b in ev]


def _setup(config):
    B, T, S, C, r = CONFIGS[config]
    dev = torch.device("cuda:0")
    os.environ.pop("FTR_PRUNED_ROUTE", None)
    inp = make_inputs(B, T, S, C, seed=1000, device=dev)
    sym, bd, blank = inp["symbols"], inp["boundary"], inp["blank"]
    _, (gx, gy) = ft.rnnt_loss_simple(inp["lm"], inp["am"], sym, blank, bd, reduction="sum", calc_gradients=True)
    ranges = ft.get_rnnt_prune_ranges(gx, gy, bd, r)
    g = torch.Generator(device="cpu").manual_seed(2000)
    x32 = torch.randn((B, T, r, C), generator=g, dtype=torch.float32).to(dev)
    y32 = torch.randn((B, T, r, C), generator=g, dtype=torch.float32).to(dev)
    return dev, sym, bd, blank, ranges, x32, y32


def run(config, setup, dtype_name, mode, tau, reps, warmup):
    B, T, S, C, r = CONFIGS[config]
    dev, sym, bd, blank, ranges, x32, y32 = setup
    x = x32.to(DTYPES[dtype_name]).requires_grad_(True)
    y = y32.to(DTYPES[dtype_name])
    values = {}

    def fused():
        loss, kd = ft.rnnt_loss_pruned_kd(x, y, sym, ranges, blank, bd, mode=mode, temperature=tau)
        values["fused"] = (loss, kd)
        return loss + LAM * kd

    def composition():
        loss = ft.rnnt_loss_pruned(x, sym, ranges, blank, bd)
        kd = ft.rnnt_kd_loss_pruned(x, y, sym, ranges, blank, bd, mode=mode, temperature=tau)
        values["composition"] = (loss, kd)
        return loss + LAM * kd

    def make(fn):
        def step():
            grad, = torch.autograd.grad(fn(), x)
            return grad
        return step

    cands = {"fused": make(fused), "composition": make(composition)}
    calls = []
    ft._lib.set_profile_hook(lambda name: calls.append(name) or contextlib.nullcontext())
    try:
        cands["fused"]()
    finally:
        ft._lib.set_profile_hook(None)
    assert "ftr_pruned_band_kd_fwd_dt" in calls and "ftr_pruned_band_kd_bwd_scaled_dt" in calls, "the fused route was not taken"
    for _ in range(warmup):
        for step in cands.values():
            step()
    torch.cuda.synchronize()
    # the two ways agree: the values bit for bit, the gradients up to their roundings (not a test: tests/test_gpu_kd_loss.py)
    ga, gb = cands["fused"]().float(), cands["composition"]().float()
    agree = float((ga - gb).abs().max() / gb.abs().max())
    same = all(torch.equal(u, v) for u, v in zip(values["fused"], values["composition"]))
    del ga, gb
    peak = {}
    for k, step in cands.items():       # the allocator's peak above what is held between steps (inputs, ranges, both logits)
        values.clear()
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
    out = {"config": config, "B": B, "T": T, "S": S, "C": C, "s_range": r, "reps": reps, "dtype": dtype_name, "mode": mode,
           "temperature": tau, "lam": LAM}
    for k, bl in blocks.items():
        meds = [statistics.median(b) for b in bl]
        out[k + "_us_median"] = round(statistics.median([v for b in bl for v in b]), 1)
        out[k + "_us_block_median_min"] = round(min(meds), 1)
        out[k + "_us_block_median_max"] = round(max(meds), 1)
        out[k + "_loss"], out[k + "_kd"] = (float(v.detach()) for v in values[k])
        out[k + "_peak_bytes_above_inputs"] = int(peak[k])
    out["values_bit_identical"] = same
    out["fused_vs_composition_grad_max_rel"] = agree
    out["composition_over_fused"] = round(out["composition_us_median"] / out["fused_us_median"], 3)
    # the time rule: the new function's slowest block against the composition's fastest
    out["fused_beats_composition_by_more_than_the_spread"] = out["fused_us_block_median_max"] < out["composition_us_block_median_min"]
    out["memory_saved_bytes"] = int(peak["composition"] - peak["fused"])
    out["memory_saved_expected_bytes"] = x.element_size() * B * T * r * C       # one tensor of the size of logits
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", choices=sorted(CONFIGS))
    ap.add_argument("--dtype", action="append", choices=sorted(DTYPES))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    for c in a.config or ["c3", "c4", "c5"]:
        setup = _setup(c)
        for dtype_name in a.dtype or ["f32", "bf16"]:
            for mode in MODES:
                for tau in TEMPERATURES:
                    line = json.dumps(run(c, setup, dtype_name, mode, tau, a.reps, a.warmup))
                    print(line, flush=True)
                    if a.out:
                        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                        with open(a.out, "a") as f:
                            f.write(line + "\n")
                    torch.cuda.empty_cache()
        del setup


if __name__ == "__main__":
    main()
