"""Best-path alignment (mutual_information_viterbi, csrc/mi_viterbi.hip) against the recursion's forward on the same
px / py: device-event timings after warm-up, the two calls alternated in one process.  One JSON line per config.

    python scripts/viterbi_bench.py --config c3 [--config c5 ...] [--reps 50] [--rnnt-type regular|modified]

px / py come from get_rnnt_logprobs on the seeded BASELINE inputs of bench.py.  Under rocprofv3 --kernel-trace --stats
the per-kernel times of mi_viterbi_kernel and mi_bidir_fwd_kernel are the ones to compare."""
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
    B, T, S, C, _ = CONFIGS[config]
    dev = torch.device("cuda:0")
    inp = make_inputs(B, T, S, C, seed=1000, device=dev)
    px, py = ft.get_rnnt_logprobs(inp["lm"], inp["am"], inp["symbols"], inp["blank"], rnnt_type=rnnt_type, boundary=inp["boundary"])
    bd = inp["boundary"]
    vit = lambda: ft.mutual_information_viterbi(px, py, bd)
    fwd = lambda: ft.mutual_information_recursion(px, py, bd)
    for _ in range(warmup):
        vit(); fwd()
    torch.cuda.synchronize()
    tv, tf = [], []
    for _ in range(reps // 10 + (reps % 10 > 0)):            # alternate in blocks of 10
        tv += _time(vit, 10)
        tf += _time(fwd, 10)
    tv.sort(); tf.sort()
    score, frames = vit()
    torch.cuda.synchronize()
    med = lambda x: x[len(x) // 2]
    steps = T + S
    return {
        "config": config, "B": B, "T": T, "S": S, "rnnt_type": rnnt_type, "reps": len(tv),
        "viterbi_us_median": round(med(tv), 2), "viterbi_us_min": round(tv[0], 2),
        "mi_fwd_us_median": round(med(tf), 2), "mi_fwd_us_min": round(tf[0], 2),
        "ratio_median": round(med(tv) / med(tf), 3),
        "viterbi_ns_per_dp_step": round(med(tv) * 1000.0 / steps, 2),
        "workspace_bytes": int(ft._lib.lib().ftr_mutual_information_viterbi_workspace_bytes(B, S, T)),
        "score_sum": float(score.double().sum()), "frames_sum": int(frames.long().sum()),
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
