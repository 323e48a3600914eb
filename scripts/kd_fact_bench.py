"""rnnt_kd_loss_pruned_factored (forward + backward), HAT and TDT rows, against (a) a torch composition of the same loss on
the same tensors and (b) rnnt_kd_loss_pruned on tensors of the same size: float32 and bfloat16, both modes, device-event
timings after warm-up, everything interleaved in one process in blocks of ten.  One JSON line per config.

    python scripts/kd_fact_bench.py --config c3 --config c4 --config c5 [--reps 30] [--zero-share 0.5]
                                    [--out profiles/kd_fact_bench_c3_c4_c5.jsonl]

Inputs as in scripts/kd_bench.py: the seeded BASELINE inputs of bench.py, prune ranges from get_rnnt_prune_ranges on the
occupancies of rnnt_loss_simple, student and teacher logits seeded random tensors rounded to bfloat16, a full boundary.  HAT
rows have the config's C columns; TDT rows have C + 4 (N = 4 durations behind the C token columns, so the width stays a
multiple of four), and (b) runs on a tensor of that same width.

(a) is what one would write without the op: float32 log_softmax / logsigmoid of both tensors, the blank masked out of the
HAT softmax, kl_div (full) or gathers and a masked logsumexp (collapsed), the duration head's kl_div, the validity mask, the
sums -- and autograd's backward of that.  (b) is the plain row form of the same kernels (csrc/pruned_kd.hip).
Per variant <dtype>_<fact>_<mode>: _fused / _torch / _kd medians, minima and the lowest and highest block median;
_fused_over_torch and _fused_over_kd (medians); _condition: the fused op's slowest block median is below the composition's
fastest.  --zero-share S adds a line (first config only) with node weights that are exact zeros on a share S of the nodes:
_fused_w (those weights) and _fused_w1 (weights of 1 everywhere) next to _fused."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tf-fast-rnnt_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import tf_fast_rnnt as ft  # noqa: E402
from bench import CONFIGS, make_inputs  # noqa: E402

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
MODES = ("full", "collapsed")
FACTS = {"hat": 0, "tdt": 4}      # factorization: duration columns


def torch_kd_fact(x, y, symbols, ranges, blank, boundary, fact, N, mode, tau):
    """mean over the batch of the per-utterance sums, composed from torch ops (inputs finite: the mask is a product)"""
    B, T, r, W = x.shape
    C = W - N
    S = symbols.shape[1]
    ranges, bd = ranges.long(), boundary.long()
    t = torch.arange(T, device=x.device)[None, :, None]
    sb, tb, se, te = (bd[:, i][:, None, None] for i in range(4))
    valid = (t >= tb) & (t < te) & (ranges >= sb) & (ranges <= se)
    a, b = x.float() / tau, y.float() / tau
    cols = torch.arange(C, device=x.device)

    def rows(v):      # one normalised log-distribution over the C columns
        if fact == "tdt":
            return F.log_softmax(v[..., :C], dim=-1)
        inner = F.log_softmax(v.masked_fill(cols == blank, float("-inf")), dim=-1)
        return torch.where(cols == blank, F.logsigmoid(v[..., blank])[..., None], F.logsigmoid(-v[..., blank])[..., None] + inner)
    logq, logp = rows(a), rows(b)
    if mode == "full":
        node = F.kl_div(logq, logp, reduction="none", log_target=True).sum(-1)
    else:
        sym_at = torch.gather(F.pad(symbols.long(), (0, 1), value=blank), 1, ranges.clamp(0, S).reshape(B, T * r)).reshape(B, T, r)
        has_sym = (ranges < se) & (sym_at != blank)
        sym_at = torch.where(has_sym, sym_at, torch.full_like(sym_at, blank))
        taken = (cols == blank) | (cols[None, None, None, :] == sym_at[..., None])

        def classes(lp):
            ls = torch.gather(lp, 3, sym_at[..., None])[..., 0].masked_fill(~has_sym, float("-inf"))
            return torch.stack([lp[..., blank], ls, torch.logsumexp(lp.masked_fill(taken, float("-inf")), dim=-1)], -1)
        cq, cp = classes(logq), classes(logp)
        p = cp.exp()
        node = torch.where(p == 0, torch.zeros_like(p), p * (cp - cq)).sum(-1)
    if N:
        node = node + F.kl_div(F.log_softmax(a[..., C:], dim=-1), F.log_softmax(b[..., C:], dim=-1), reduction="none", log_target=True).sum(-1)
    return (node * valid).sum((1, 2)).mean()


def _time(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1000.0 for a, b in ev]


def run(config, reps, warmup, tau, zero_share=None):
    B, T, S, C, r = CONFIGS[config]
    dev = torch.device("cuda:0")
    inp = make_inputs(B, T, S, C, seed=1000, device=dev)
    sym, bd, blank = inp["symbols"], inp["boundary"], inp["blank"]
    _, (gx, gy) = ft.rnnt_loss_simple(inp["lm"], inp["am"], sym, blank, bd, "regular", reduction="sum", calc_gradients=True)
    ranges = ft.get_rnnt_prune_ranges(gx, gy, bd, r)
    del inp, gx, gy
    out = {"config": config, "B": B, "T": T, "S": S, "C": C, "s_range": r, "temperature": tau, "tdt_durations": FACTS["tdt"]}
    weights = ones = None
    if zero_share is not None:
        g = torch.Generator(device="cpu").manual_seed(3000)
        u = torch.rand((B, T, r), generator=g)
        weights = torch.where(u < zero_share, torch.zeros(()), 0.5 + u).to(dev)
        ones = torch.ones((B, T, r), device=dev)
        out["zero_share"] = zero_share
        out["zero_share_drawn"] = round(float((weights == 0).float().mean()), 4)
    steps = {}
    for fact, N in FACTS.items():
        W = C + N
        g = torch.Generator(device="cpu").manual_seed(2000)
        xs = torch.randn((B, T, r, W), generator=g, dtype=torch.float32).to(dev).to(torch.bfloat16)
        ys = torch.randn((B, T, r, W), generator=g, dtype=torch.float32).to(dev).to(torch.bfloat16)
        for n, dt in DTYPES.items():
            x = xs.to(dt).requires_grad_(True)
            y = ys.to(dt)
            for mode in MODES:
                def fused(x=x, y=y, mode=mode, fact=fact, N=N, w=None):
                    loss = ft.rnnt_kd_loss_pruned_factored(x, y, sym, ranges, blank, bd, factorization=fact, num_durations=N, mode=mode,
                                                           temperature=tau, node_weights=w)
                    torch.autograd.grad(loss, x)
                    return loss

                def composed(x=x, y=y, mode=mode, fact=fact, N=N):
                    loss = torch_kd_fact(x, y, sym, ranges, blank, bd, fact, N, mode, tau)
                    torch.autograd.grad(loss, x)
                    return loss

                def kd(x=x, y=y, mode=mode):
                    loss = ft.rnnt_kd_loss_pruned(x, y, sym, ranges, blank, bd, mode=mode, temperature=tau)
                    torch.autograd.grad(loss, x)
                    return loss
                key = f"{n}_{fact}_{mode}"
                steps[f"{key}_fused"] = fused
                if weights is None:
                    steps[f"{key}_torch"] = composed
                    steps[f"{key}_kd"] = kd
                else:
                    steps[f"{key}_fused_w"] = lambda fused=fused: fused(w=weights)
                    steps[f"{key}_fused_w1"] = lambda fused=fused: fused(w=ones)
        del xs, ys
    names = list(steps)
    for n in names:
        if not n.endswith("_kd"):
            out[f"{n}_loss"] = float(steps[n]().detach())
    for _ in range(warmup):
        for n in names:
            steps[n]()
    torch.cuda.synchronize()
    times = {n: [] for n in names}
    for _ in range(reps // 10 + (reps % 10 > 0)):                   # interleaved in blocks of 10
        for n in names:
            times[n] += _time(steps[n], 10)
    med = lambda v: sorted(v)[len(v) // 2]
    blocks = {n: [med(times[n][i:i + 10]) for i in range(0, len(times[n]), 10)] for n in names}
    out["reps"] = len(times[names[0]])
    for n in names:
        out[f"{n}_us_median"] = round(med(times[n]), 2)
        out[f"{n}_us_min"] = round(min(times[n]), 2)
        out[f"{n}_block_median_us_min_max"] = [round(min(blocks[n]), 2), round(max(blocks[n]), 2)]
    ok = True
    for n in names:
        if n.endswith("_fused"):
            key = n[:-6]
            if weights is None:
                out[f"{n}_over_torch"] = round(med(times[n]) / med(times[key + "_torch"]), 4)
                out[f"{n}_over_kd"] = round(med(times[n]) / med(times[key + "_kd"]), 4)
                out[f"{key}_condition"] = max(blocks[n]) < min(blocks[key + "_torch"])
                ok = ok and out[f"{key}_condition"]
            else:
                out[f"{n}_w_over_fused"] = round(med(times[n + "_w"]) / med(times[n]), 4)
                out[f"{n}_w1_over_fused"] = round(med(times[n + "_w1"]) / med(times[n]), 4)
    if weights is None:
        out["condition_holds_everywhere"] = ok
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--temperature", type=float, default=2.0)
    ap.add_argument("--zero-share", type=float, help="one more line, first config: node weights with this share of exact zeros")
    ap.add_argument("--out", help="append the JSON lines to this file as well")
    args = ap.parse_args()
    configs = args.config or ["c3"]
    jobs = [(c, None) for c in configs] + ([(configs[0], args.zero_share)] if args.zero_share is not None else [])
    for c, share in jobs:
        line = json.dumps(run(c, max(args.reps, 10), args.warmup, args.temperature, share))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
