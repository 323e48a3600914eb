"""rnnt_path_logprob_pruned (one wave per arc, csrc/pruned_path.hip) against the torch composition a caller writes without
it -- log_softmax(logits.float()), two gathers, a sum, autograd -- on the same device tensors: forward + backward,
device-event timings after warm-up, the two arms interleaved in one process in blocks of 10, the median over all steps and
the lowest and highest block median; the peak of torch's allocator above the inputs during one step of each.  One JSON line
per config and dtype, appended to --out.

    python scripts/path_logprob_bench.py --config c3 --config c4 --config c5 [--reps 60] [--out profiles/path_logprob_bench_c3_c4_c5.jsonl]

Input: seeded standard normal joiner logits [B,T,s_range,C] of the BASELINE config in float32 and bfloat16, a diagonal band,
softmax rows, the regular type; the path is the best path (rnnt_alignment_pruned).  The gather indices of the torch arm are
built once, outside the timed region.

What the lines are judged by: the new function's highest block median below the composition's lowest."""
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
BLOCK = 10


def _time(fn, reps):
    ev = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1000.0 for a, b in ev]


def diagonal_band(B, T, S, r, dev):
    s0 = (torch.arange(T, dtype=torch.float64) * (S / T)).long() - r // 2
    s0 = s0.clamp(0, max(S + 1 - r, 0))
    return (s0[None, :, None] + torch.arange(r)[None, None, :]).expand(B, T, r).contiguous().to(torch.int32).to(dev)


def run(config, x, dtype_name, reps, warmup):
    B, T, S, C, r = CONFIGS[config]
    dev = x.device
    blank = C - 1
    sym = torch.randint(0, C - 1, (B, S), generator=torch.Generator().manual_seed(2001)).to(torch.int32).to(dev)
    ranges = diagonal_band(B, T, S, r, dev)
    score, frames = ft.rnnt_alignment_pruned(x, sym, ranges, blank)
    # the torch arm's indices: node (s, frames[s]) and column symbols[s]; node (#{frames <= t}, t) and the blank column
    f = frames.long()
    bi = torch.arange(B, device=dev)[:, None]
    sym_k = torch.arange(S, device=dev)[None, :] - ranges[bi, f, 0].long()
    ts = torch.arange(T, device=dev)[None, :].expand(B, T)
    blank_k = torch.searchsorted(f, ts.contiguous(), right=True) - ranges[:, :, 0].long()
    assert bool(((sym_k >= 0) & (sym_k < r)).all()) and bool(((blank_k >= 0) & (blank_k < r)).all()) and bool(torch.isfinite(score).all())
    x.requires_grad_(True)

    def composed():
        x.grad = None
        lp = torch.log_softmax(x.float(), -1)
        out = lp[bi, f, sym_k, sym.long()].sum(1) + lp[bi, ts, blank_k, blank].sum(1)
        out.sum().backward()
        return out

    def native():
        x.grad = None
        out = ft.rnnt_path_logprob_pruned(x, sym, ranges, blank, frames)
        out.sum().backward()
        return out

    cands = {"path": native, "torch": composed}
    for _ in range(warmup):
        for fn in cands.values():
            fn()
    torch.cuda.synchronize()
    out = {"config": config, "B": B, "T": T, "S": S, "C": C, "s_range": r, "reps": reps, "dtype": dtype_name,
           "logits_bytes": x.numel() * x.element_size(), "rows_on_path_fraction": round((S + T) / (T * r), 4)}
    a, b = native().detach(), composed().detach()          # not a test: tests/test_gpu_wave_per_path_arc_logprob.py
    out["max_abs_diff_to_torch"] = float((a - b).abs().max())
    out["max_abs_diff_to_viterbi_score"] = float((a - score).abs().max())
    del a, b
    for k, fn in cands.items():       # the allocator's peak above what is held between steps
        x.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        fn()
        torch.cuda.synchronize()
        out[k + "_peak_bytes_above_inputs"] = int(torch.cuda.max_memory_allocated(dev) - base)
    blocks = {k: [] for k in cands}
    for _ in range((reps + BLOCK - 1) // BLOCK):
        for k, fn in cands.items():
            blocks[k].append(_time(fn, BLOCK))
    for k, bl in blocks.items():
        meds = [statistics.median(v) for v in bl]
        out[k + "_us_median"] = round(statistics.median([v for blk in bl for v in blk]), 1)
        out[k + "_us_block_median_min"] = round(min(meds), 1)
        out[k + "_us_block_median_max"] = round(max(meds), 1)
    out["path_over_torch"] = round(out["path_us_median"] / out["torch_us_median"], 4)
    # the time rule: the new function's slowest block against the composition's fastest
    out["path_beats_torch_by_more_than_the_spread"] = out["path_us_block_median_max"] < out["torch_us_block_median_min"]
    x.requires_grad_(False)
    x.grad = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", choices=sorted(CONFIGS))
    ap.add_argument("--dtype", action="append", choices=sorted(DTYPES))
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for c in a.config or ["c3", "c4", "c5"]:
        B, T, S, C, r = CONFIGS[c]
        x32 = torch.randn((B, T, r, C), generator=torch.Generator(device="cpu").manual_seed(2000), dtype=torch.float32)
        for dtype_name in a.dtype or ["f32", "bf16"]:
            x = x32.to(DTYPES[dtype_name]).to(dev)
            line = json.dumps(run(c, x, dtype_name, a.reps, a.warmup))
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as fh:
                    fh.write(line + "\n")
            del x
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
