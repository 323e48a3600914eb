"""Best-path alignment over the TDT / multi-blank lattice (mutual_information_viterbi_tdt, csrc/mi_viterbi_tdt.hip):
device-event timings after warm-up, each candidate alternated with its yardstick in one process.  Two JSON lines per
config and run:

  * moves (0,) / (1,), the ordinary lattice, against mutual_information_viterbi on the same px / py;
  * moves (0,1,2,3,4) / (1,2,3,4) against the forward of mutual_information_recursion_tdt on the same operands.

    python scripts/viterbi_tdt_bench.py --config c3 [--config c5 ...] [--reps 50] [--runs 3] [--out FILE]

px / py come from get_rnnt_logprobs on the seeded BASELINE inputs of bench.py; the nine-move operands add a seeded
duration head (log_softmax of N(0,1) logits per cell) to them.  Under rocprofv3 --kernel-trace --stats the per-kernel
times of mi_viterbi_tdt_kernel, mi_viterbi_kernel and mi_tdt_kernel are the ones to compare."""
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

TOK, BLK = (0, 1, 2, 3, 4), (1, 2, 3, 4)


def _time(fn, reps):
    ev = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1000.0 for a, b in ev]


def _alternate(cand, ref, reps, warmup):
    for _ in range(warmup):
        cand(); ref()
    torch.cuda.synchronize()
    tc, tr = [], []
    for _ in range(reps // 10 + (reps % 10 > 0)):            # alternate in blocks of 10
        tc += _time(cand, 10)
        tr += _time(ref, 10)
    tc.sort(); tr.sort()
    return tc, tr


def run(config, reps, warmup, run_index):
    B, T, S, C, _ = CONFIGS[config]
    dev = torch.device("cuda:0")
    inp = make_inputs(B, T, S, C, seed=1000, device=dev)
    px, py = ft.get_rnnt_logprobs(inp["lm"], inp["am"], inp["symbols"], inp["blank"], boundary=inp["boundary"])
    bd = inp["boundary"]
    g = torch.Generator(device="cpu").manual_seed(1001)
    dur = torch.log_softmax(torch.randn(B, len(TOK), S + 1, T + 1, generator=g), dim=1).to(dev)
    px9 = (px[:, None] + dur[:, :, :S, :]).contiguous()
    py9 = (py[:, None] + dur[:, 1:, :, :T]).contiguous()
    px1, py1 = px[:, None].contiguous(), py[:, None].contiguous()
    med = lambda x: x[len(x) // 2]
    nbytes = int(ft._lib.lib().ftr_mutual_information_viterbi_tdt_workspace_bytes(B, S, T))
    lines = []
    for name, cand, ref, ref_name in (
            ("0/1", lambda: ft.mutual_information_viterbi_tdt(px1, py1, (0,), (1,), bd),
             lambda: ft.mutual_information_viterbi(px, py, bd), "mutual_information_viterbi"),
            ("01234/1234", lambda: ft.mutual_information_viterbi_tdt(px9, py9, TOK, BLK, bd),
             lambda: ft.mutual_information_recursion_tdt(px9, py9, TOK, BLK, bd), "mutual_information_recursion_tdt forward")):
        tc, tr = _alternate(cand, ref, reps, warmup)
        score, frames, durs, steps = cand()
        torch.cuda.synchronize()
        lines.append({
            "config": config, "B": B, "T": T, "S": S, "moves": name, "run": run_index, "reps": len(tc),
            "viterbi_tdt_us_median": round(med(tc), 2), "viterbi_tdt_us_min": round(tc[0], 2),
            "yardstick": ref_name, "yardstick_us_median": round(med(tr), 2), "yardstick_us_min": round(tr[0], 2),
            "ratio_median": round(med(tc) / med(tr), 3), "workspace_bytes": nbytes,
            "score_sum": float(score.double().sum()), "frames_sum": int(frames.long().sum()),
            "durations_sum": int(durs.long().sum()), "blank_steps_sum": int(steps.long().sum()),
        })
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    for i in range(args.runs):
        for c in args.config or ["c3"]:
            for line in run(c, max(args.reps, 10), args.warmup, i):
                text = json.dumps(line)
                print(text, flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(text + "\n")


if __name__ == "__main__":
    main()
