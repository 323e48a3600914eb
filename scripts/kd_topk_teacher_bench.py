"""rnnt_kd_topk_cache (one HIP row kernel) against rnnt_kd_topk_teacher (plain torch) on the same device tensor: device-event
timings after warm-up, the two interleaved in one process in blocks of 10, the median over all calls and the lowest and
highest block median; the peak of torch's allocator above the input during one call of each; the new function's bytes of
logits per second.  One JSON line per config, dtype, K and rest form, appended to --out.

    python scripts/kd_topk_teacher_bench.py --config c3 --config c4 --config c5 [--reps 60] [--out profiles/kd_topk_teacher_bench_c3_c4_c5.jsonl]

Input: a seeded standard normal teacher tensor [B,T,s_range,C] of the BASELINE config, in float32 and bfloat16.

What the lines are judged by: at K = 8, the new function's highest block median below the torch
maker's lowest.  K = 64 lines, the memory figures and the byte rate are recorded without a gate."""
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
from bench import CONFIGS  # noqa: E402

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
KS = (8, 64)
BLOCK = 10


def _time(fn, reps):
    ev = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1000.0 for a, b in ev]


def run(config, y, dtype_name, K, with_rest, reps, warmup):
    B, T, S, C, r = CONFIGS[config]
    dev = y.device
    cands = {"cache": lambda: ft.rnnt_kd_topk_cache(y, K, 1.0, with_rest), "torch": lambda: ft.rnnt_kd_topk_teacher(y, K, 1.0, with_rest)}
    for _ in range(warmup):
        for fn in cands.values():
            fn()
    torch.cuda.synchronize()
    out = {"config": config, "B": B, "T": T, "C": C, "s_range": r, "reps": reps, "dtype": dtype_name, "K": K, "rest": with_rest,
           "input_bytes": y.numel() * y.element_size()}
    (v0, i0, _), (v1, i1, _) = cands["cache"](), cands["torch"]()      # not a test: tests/test_gpu_kd_topk_teacher.py
    out["values_equal_torch"] = bool(torch.equal(v0, v1))
    out["rows_with_other_columns_than_torch"] = int((i0 != i1).any(-1).sum())   # ties: torch.topk's choice is its own
    del v0, i0, v1, i1
    for k, fn in cands.items():       # the allocator's peak above what is held between calls
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        fn()
        torch.cuda.synchronize()
        out[k + "_peak_bytes_above_input"] = int(torch.cuda.max_memory_allocated(dev) - base)
    blocks = {k: [] for k in cands}
    for _ in range((reps + BLOCK - 1) // BLOCK):
        for k, fn in cands.items():
            blocks[k].append(_time(fn, BLOCK))
    for k, bl in blocks.items():
        meds = [statistics.median(b) for b in bl]
        out[k + "_us_median"] = round(statistics.median([v for b in bl for v in b]), 1)
        out[k + "_us_block_median_min"] = round(min(meds), 1)
        out[k + "_us_block_median_max"] = round(max(meds), 1)
    out["cache_over_torch"] = round(out["cache_us_median"] / out["torch_us_median"], 4)
    out["cache_logits_GB_per_s"] = round(out["input_bytes"] / out["cache_us_median"] / 1e3, 1)
    # the time rule: the new function's slowest block against the other's fastest
    out["cache_beats_torch_by_more_than_the_spread"] = out["cache_us_block_median_max"] < out["torch_us_block_median_min"]
    out["gated"] = K == 8
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", choices=sorted(CONFIGS))
    ap.add_argument("--dtype", action="append", choices=sorted(DTYPES))
    ap.add_argument("--k", action="append", type=int)
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for c in a.config or ["c3", "c4", "c5"]:
        B, T, S, C, r = CONFIGS[c]
        g = torch.Generator(device="cpu").manual_seed(2000)
        y32 = torch.randn((B, T, r, C), generator=g, dtype=torch.float32)
        for dtype_name in a.dtype or ["f32", "bf16"]:
            y = y32.to(DTYPES[dtype_name]).to(dev)
            for K in a.k or KS:
                for with_rest in (True, False):
                    line = json.dumps(run(c, y, dtype_name, K, with_rest, a.reps, a.warmup))
                    print(line, flush=True)
                    if a.out:
                        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                        with open(a.out, "a") as f:
                            f.write(line + "\n")
                    torch.cuda.empty_cache()
            del y


if __name__ == "__main__":
    main()
