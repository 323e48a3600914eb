"""rnnt_kd_loss_pruned_topk against the two ways to distil on the same nodes without it, forward + backward: device-event
timings after warm-up, the candidates interleaved in one process in blocks of 10, the median over all steps and the lowest
and highest block median; the peak of torch's allocator above the inputs during one step of each, and the bytes of the
teacher inputs each holds.  One JSON line per config, dtype, K and rest form, appended to --out.

    python scripts/kd_topk_bench.py --config c3 --config c4 --config c5 [--reps 50] [--out profiles/kd_topk_bench_c3_c4_c5.jsonl]

Candidates:
  topk      rnnt_kd_loss_pruned_topk(x, values, indices, ranges, boundary, teacher_ranges, teacher_rest)
  dense     the shipped op in full mode with a dense teacher [B,T,r,C] in the student's dtype, on the nodes `topk` distils: the
            match mask goes in as node_weights of rnnt_kd_loss_pruned_factored, so both do the same number of rows
  scatter   (renormalised lines only) what a holder of the cache writes without the new op: gather the cache rows onto the
            student's nodes, scatter them into a -inf-filled float32 [B,T,r,C], the match mask as node_weights, the shipped op
Inputs: the seeded BASELINE inputs of bench.py, prune ranges from get_rnnt_prune_ranges on the occupancies of
rnnt_loss_simple, seeded random student logits; the teacher's ranges are the student's, shifted by one row on every other
frame (r_t = r), and the cache is rnnt_kd_topk_teacher of a seeded random dense teacher on them, values in the student's dtype.

What the lines are judged by: at K = 8, `topk`'s highest block median below `dense`'s lowest and below
`scatter`'s lowest.  K = 32 lines and the memory figures are recorded without a gate."""
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

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
KS = (8, 32)
BLOCK = 10


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
    ranges = ft.get_rnnt_prune_ranges(gx, gy, bd, r).to(torch.int32).contiguous()
    tranges = ranges.clone()
    tranges[:, 1::2] += 1                     # the teacher's band: one row up on every other frame
    g = torch.Generator(device="cpu").manual_seed(2000)
    x32 = torch.randn((B, T, r, C), generator=g, dtype=torch.float32).to(dev)
    y32 = torch.randn((B, T, r, C), generator=g, dtype=torch.float32).to(dev)
    return dev, sym, bd, blank, ranges, tranges, x32, y32


def _nbytes(*tensors):
    return int(sum(t.numel() * t.element_size() for t in tensors if t is not None))


def run(config, setup, dtype_name, K, with_rest, reps, warmup):
    B, T, S, C, r = CONFIGS[config]
    dev, sym, bd, blank, ranges, tranges, x32, y32 = setup
    x = x32.to(DTYPES[dtype_name]).requires_grad_(True)
    y = y32.to(DTYPES[dtype_name])            # `dense`: a teacher on the student's ranges; `topk`: the teacher on its own
    vals, idx, rest = ft.rnnt_kd_topk_teacher(y, K, 1.0, with_rest)
    kp = ranges - tranges[:, :, :1]
    match = (kp >= 0) & (kp < r)
    mask = match.to(torch.float32)
    kp = kp.clamp(0, r - 1).long()[..., None].expand(B, T, r, K)
    values = {}

    def topk():
        values["topk"] = ft.rnnt_kd_loss_pruned_topk(x, vals, idx, ranges, bd, teacher_ranges=tranges, teacher_rest=rest)
        return values["topk"]

    def dense():
        values["dense"] = ft.rnnt_kd_loss_pruned_factored(x, y, sym, ranges, blank, bd, node_weights=mask)
        return values["dense"]

    def scatter():
        full = torch.full((B, T, r, C), float("-inf"), dtype=torch.float32, device=dev)
        full.scatter_(3, torch.gather(idx, 2, kp).long(), torch.gather(vals, 2, kp).float())
        values["scatter"] = ft.rnnt_kd_loss_pruned_factored(x, full, sym, ranges, blank, bd, node_weights=mask)
        return values["scatter"]

    def make(fn):
        def step():
            grad, = torch.autograd.grad(fn(), x)
            return grad
        return step

    cands = {"topk": make(topk), "dense": make(dense)}
    if not with_rest:
        cands["scatter"] = make(scatter)
    for _ in range(warmup):
        for step in cands.values():
            step()
    torch.cuda.synchronize()
    out = {"config": config, "B": B, "T": T, "S": S, "C": C, "s_range": r, "r_t": r, "reps": reps, "dtype": dtype_name, "K": K,
           "rest": with_rest, "distilled_nodes": int(match.sum()), "nodes": B * T * r}
    if not with_rest:     # the same loss two ways (not a test: tests/test_gpu_kd_topk.py)
        ga, gb = cands["topk"]().float(), cands["scatter"]().float()
        out["topk_vs_scatter_grad_max_rel"] = float((ga - gb).abs().max() / gb.abs().max())
        del ga, gb
    peak = {}
    for k, step in cands.items():       # the allocator's peak above what is held between steps
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
    cache_bytes = _nbytes(vals, idx, rest, tranges)
    teacher_bytes = {"topk": cache_bytes, "dense": _nbytes(y, mask), "scatter": cache_bytes + _nbytes(mask)}
    for k, bl in blocks.items():
        meds = [statistics.median(b) for b in bl]
        out[k + "_us_median"] = round(statistics.median([v for b in bl for v in b]), 1)
        out[k + "_us_block_median_min"] = round(min(meds), 1)
        out[k + "_us_block_median_max"] = round(max(meds), 1)
        out[k + "_loss"] = float(values[k].detach())
        out[k + "_peak_bytes_above_inputs"] = int(peak[k])
        out[k + "_teacher_input_bytes"] = teacher_bytes[k]
    out["topk_over_dense"] = round(out["topk_us_median"] / out["dense_us_median"], 3)
    out["topk_over_dense_expected_from_bytes"] = 0.6
    # the time rule: the new function's slowest block against the other's fastest
    out["topk_beats_dense_by_more_than_the_spread"] = out["topk_us_block_median_max"] < out["dense_us_block_median_min"]
    if not with_rest:
        out["topk_over_scatter"] = round(out["topk_us_median"] / out["scatter_us_median"], 3)
        out["topk_beats_scatter_by_more_than_the_spread"] = out["topk_us_block_median_max"] < out["scatter_us_block_median_min"]
    out["gated"] = K == 8
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", choices=sorted(CONFIGS))
    ap.add_argument("--dtype", action="append", choices=sorted(DTYPES))
    ap.add_argument("--k", action="append", type=int)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    for c in a.config or ["c3", "c4", "c5"]:
        setup = _setup(c)
        for dtype_name in a.dtype or ["f32", "bf16"]:
            for K in a.k or KS:
                for with_rest in (True, False):
                    line = json.dumps(run(c, setup, dtype_name, K, with_rest, a.reps, a.warmup))
                    print(line, flush=True)
                    if a.out:
                        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                        with open(a.out, "a") as f:
                            f.write(line + "\n")
                    torch.cuda.empty_cache()
        del setup


if __name__ == "__main__":
    main()
