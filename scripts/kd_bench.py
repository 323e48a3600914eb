"""rnnt_kd_loss_pruned (forward + backward) against a torch composition of the same loss on the same tensors: float32 and
bfloat16, both modes, device-event timings after warm-up, everything interleaved in one process.  One JSON line per config.

    python scripts/kd_bench.py --config c3 --config c4 --config c5 [--reps 30] [--out profiles/kd_bench_c3_c4_c5.jsonl]

Inputs are the seeded BASELINE inputs of bench.py; the prune ranges come from get_rnnt_prune_ranges on the occupancies of
rnnt_loss_simple, student and teacher logits [B,T,r,C] are seeded random tensors rounded to bfloat16, so both dtypes see the
same numbers.  The boundary is full: every node is valid and every row is read.

The torch composition is what one would write without the op (tests/kd_cases.py holds the checked, NaN-safe version of it):
log_softmax of both tensors in float32, kl_div (full) or two gathers and a masked logsumexp per tensor (collapsed), the
validity mask, the sums -- and autograd's backward of that.  Per variant: <name>_us_median, _us_min, the spread of the block
medians, <name>_over_torch (fused / torch, medians), and the achieved rate <name>_gbs = algorithmic bytes / median with
  forward  = both tensors read once; backward = student read + gradient written (+ teacher read in full mode).
lse_band_fwd_*: ftr_pruned_band_fwd on the student tensor in the same run -- lse_rows_reg_kernel plus the [B,T,r]-sized band
gather, so its rate (one tensor read) is a lower bound on what lse_rows_reg_kernel alone reaches here."""
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


def torch_kd(x, y, symbols, ranges, blank, boundary, mode, tau):
    """mean over the batch of the per-utterance sums, composed from torch ops (inputs finite: the mask is a product)"""
    B, T, r, C = x.shape
    S = symbols.shape[1]
    ranges, bd = ranges.long(), boundary.long()
    t = torch.arange(T, device=x.device)[None, :, None]
    sb, tb, se, te = (bd[:, i][:, None, None] for i in range(4))
    valid = (t >= tb) & (t < te) & (ranges >= sb) & (ranges <= se)
    logq = F.log_softmax(x.float() / tau, dim=-1)
    logp = F.log_softmax(y.float() / tau, dim=-1)
    if mode == "full":
        node = F.kl_div(logq, logp, reduction="none", log_target=True).sum(-1)
    else:
        sym_at = torch.gather(F.pad(symbols.long(), (0, 1), value=blank), 1, ranges.clamp(0, S).reshape(B, T * r)).reshape(B, T, r)
        has_sym = (ranges < se) & (sym_at != blank)
        sym_at = torch.where(has_sym, sym_at, torch.full_like(sym_at, blank))
        cols = torch.arange(C, device=x.device)
        taken = (cols == blank) | (cols[None, None, None, :] == sym_at[..., None])

        def classes(lp):
            ls = torch.gather(lp, 3, sym_at[..., None])[..., 0].masked_fill(~has_sym, float("-inf"))
            return torch.stack([lp[..., blank], ls, torch.logsumexp(lp.masked_fill(taken, float("-inf")), dim=-1)], -1)
        cq, cp = classes(logq), classes(logp)
        p = cp.exp()
        node = torch.where(p == 0, torch.zeros_like(p), p * (cp - cq)).sum(-1)
    return (node * valid).sum((1, 2)).mean()


def _time(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1000.0 for a, b in ev]


def run(config, reps, warmup, tau):
    B, T, S, C, r = CONFIGS[config]
    dev = torch.device("cuda:0")
    inp = make_inputs(B, T, S, C, seed=1000, device=dev)
    sym, bd, blank = inp["symbols"], inp["boundary"], inp["blank"]
    _, (gx, gy) = ft.rnnt_loss_simple(inp["lm"], inp["am"], sym, blank, bd, "regular", reduction="sum", calc_gradients=True)
    ranges = ft.get_rnnt_prune_ranges(gx, gy, bd, r)
    del inp, gx, gy
    g = torch.Generator(device="cpu").manual_seed(2000)
    xs = torch.randn((B, T, r, C), generator=g, dtype=torch.float32).to(dev).to(torch.bfloat16)
    ys = torch.randn((B, T, r, C), generator=g, dtype=torch.float32).to(dev).to(torch.bfloat16)
    out = {"config": config, "B": B, "T": T, "S": S, "C": C, "s_range": r, "temperature": tau}
    steps, nbytes = {}, {}
    elems = B * T * r * C
    for n, dt in DTYPES.items():
        x = xs.to(dt).requires_grad_(True)
        y = ys.to(dt)
        size = x.element_size()
        for mode in MODES:
            def fused(x=x, y=y, mode=mode):
                loss = ft.rnnt_kd_loss_pruned(x, y, sym, ranges, blank, bd, mode=mode, temperature=tau)
                torch.autograd.grad(loss, x)
                return loss

            def composed(x=x, y=y, mode=mode):
                loss = torch_kd(x, y, sym, ranges, blank, bd, mode, tau)
                torch.autograd.grad(loss, x)
                return loss
            steps[f"{n}_{mode}_fused"] = fused
            steps[f"{n}_{mode}_torch"] = composed
            nbytes[f"{n}_{mode}_fused"] = elems * size * (5 if mode == "full" else 4)

        band = [torch.empty((B, T, r), dtype=torch.float32, device=dev) for _ in range(3)]   # lse, px_band, py_band

        def lse(x=x.detach(), band=band):
            rl = sys.modules["tf_fast_rnnt.rnnt_loss"]        # the module: the package attribute of that name is the function
            rl._pruned_call("pruned_band_fwd", False, x, (rl._ptr(sym), rl._ptr(ranges), rl._ptr(bd), blank, 0.0, *map(rl._ptr, band),
                                                          B, T, S, C, r, 0), (rl._stream_ptr(x),))
        steps[f"{n}_lse_band_fwd"] = lse
        nbytes[f"{n}_lse_band_fwd"] = elems * size
    del xs, ys
    names = list(steps)
    for n in names:
        if n.endswith("_lse_band_fwd"):
            continue
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
    out["reps"] = len(times[names[0]])
    for n in names:
        m = med(times[n])
        out[f"{n}_us_median"] = round(m, 2)
        out[f"{n}_us_min"] = round(min(times[n]), 2)
        blocks = [med(times[n][i:i + 10]) for i in range(0, len(times[n]), 10)]     # what one run of 10 steps moves by
        out[f"{n}_block_median_us_min_max"] = [round(min(blocks), 2), round(max(blocks), 2)]
        if n in nbytes:
            out[f"{n}_gbs"] = round(nbytes[n] / m / 1e3, 1)
        if n.endswith("_fused"):
            out[f"{n}_over_torch"] = round(m / med(times[n[:-6] + "_torch"]), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--temperature", type=float, default=2.0)
    ap.add_argument("--out", help="append the JSON lines to this file as well")
    args = ap.parse_args()
    for c in args.config or ["c3"]:
        line = json.dumps(run(c, max(args.reps, 10), args.warmup, args.temperature))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
