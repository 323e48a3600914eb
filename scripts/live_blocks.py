"""Counts the lattice blocks of the simple loss's backward that hold any non-zero occupancy: the GPU's own px_grad / py_grad
of rnnt_loss_simple on bench.py's inputs (make_inputs, seed 1000), per utterance and as a mean.  A cell of the [S+1, T]
lattice is live iff g_px[s,t] != 0 (s < S, the cells the forward overwrote masked) or g_py[s,t] != 0 or either is NaN;
W = -(g_px + g_py) / (prod + tiny) is zero exactly where both are.  Reported for 16-row x 64-frame and 16-row x 32-frame
blocks: the fraction of live blocks, and the fraction covered by ONE contiguous run of row chunks per frame tile (what an
interval per tile walks).  --smoothed: the occupancies of rnnt_loss_smoothed (lm_only_scale 0.1, am_only_scale 0.2), the first
pass bench.py runs at c4.  python scripts/live_blocks.py [config | B T S C] [--scale X] [--modified] [--smoothed]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tf-fast-rnnt_amd"))
import torch
import bench
import tf_fast_rnnt as ft

argv = sys.argv[1:]
scale = 1.0
if "--scale" in argv:
    i = argv.index("--scale"); scale = float(argv[i + 1]); del argv[i:i + 2]
modified, smoothed = "--modified" in argv, "--smoothed" in argv
argv = [a for a in argv if a not in ("--modified", "--smoothed")]
if len(argv) >= 4:
    name, (B, T, S, C) = "custom", (int(v) for v in argv[:4])
else:
    name = argv[0] if argv else "c3"
    B, T, S, C, _ = bench.CONFIGS[name]
dev = torch.device("cuda:0")
inp = bench.make_inputs(B, T, S, C, 1000, dev)
kw = dict(lm=inp["lm"] * scale, am=inp["am"] * scale, symbols=inp["symbols"], termination_symbol=inp["blank"], boundary=inp["boundary"],
          reduction="sum", calc_gradients=True, rnnt_type="modified" if modified else "regular")
_, (gx, gy) = ft.rnnt_loss_smoothed(lm_only_scale=0.1, am_only_scale=0.2, **kw) if smoothed else ft.rnnt_loss_simple(**kw)


def live_cells(gx, gy, boundary, modified):
    """[B, S+1, T] bool: the cells whose x, y (and with them W) are not all exactly zero."""
    B, S1, T = gy.shape
    x = torch.zeros_like(gy)
    x[:, :S1 - 1, :] = gx[:, :, :T]
    if not modified:                              # the forward wrote -inf at t = t_end: its occupancy does not count
        te = boundary[:, 3].long().clamp(max=T - 1).view(B, 1, 1).expand(B, S1, 1)
        keep = (boundary[:, 3].long() < T).view(B, 1, 1).expand(B, S1, 1)
        x.scatter_(2, te, torch.where(keep, torch.zeros_like(x[:, :, :1]), x.gather(2, te)))
    return (x != 0) | (gy != 0)                   # NaN != 0 is true


def blocks(live, rows, frames):
    """live fraction and contiguous-run fraction of rows x frames blocks, per utterance"""
    B, S1, T = live.shape
    ns, nt = (S1 + rows - 1) // rows, (T + frames - 1) // frames
    pad = torch.zeros((B, ns * rows, nt * frames), dtype=torch.bool, device=live.device)
    pad[:, :S1, :T] = live
    blk = pad.view(B, ns, rows, nt, frames).any(dim=4).any(dim=2)            # [B, ns, nt]
    frac = blk.float().mean(dim=(1, 2))
    idx = torch.arange(ns, device=live.device).view(1, ns, 1).expand(B, ns, nt)
    lo = torch.where(blk, idx, torch.full_like(idx, ns)).amin(dim=1)
    hi = torch.where(blk, idx + 1, torch.zeros_like(idx)).amax(dim=1)
    run = (hi - lo).clamp(min=0).float().sum(dim=1) / (ns * nt)              # one run of row chunks per frame tile
    idt = torch.arange(nt, device=live.device).view(1, 1, nt).expand(B, ns, nt)
    lo_t = torch.where(blk, idt, torch.full_like(idt, nt)).amin(dim=2)
    hi_t = torch.where(blk, idt + 1, torch.zeros_like(idt)).amax(dim=2)
    run_t = (hi_t - lo_t).clamp(min=0).float().sum(dim=1) / (ns * nt)        # one run of frame chunks per row block
    return frac, run, run_t


live = live_cells(gx, gy, inp["boundary"], modified)
cells = live.float().mean(dim=(1, 2))
f64, r64, rt64 = blocks(live, 16, 64)
f32, r32, rt32 = blocks(live, 16, 32)
print(f"{name} B={B} T={T} S={S} C={C} input scale {scale} {'modified' if modified else 'regular'} {'smoothed' if smoothed else 'simple'}: live fractions on the GPU's px_grad / py_grad")
print("| b | cells | 16x64 live | 16x64 row-chunk run per frame tile | 16x32 live | 16x32 frame-chunk run per row block |")
print("|---|---|---|---|---|---|")
for b in range(B):
    print(f"| {b} | {cells[b]:.3f} | {f64[b]:.3f} | {r64[b]:.3f} | {f32[b]:.3f} | {rt32[b]:.3f} |")
print(f"| mean | {cells.mean():.3f} | {f64.mean():.3f} | {r64.mean():.3f} | {f32.mean():.3f} | {rt32.mean():.3f} |")
print(f"| min / max | {cells.min():.3f} / {cells.max():.3f} | {f64.min():.3f} / {f64.max():.3f} | {r64.min():.3f} / {r64.max():.3f} | "
      f"{f32.min():.3f} / {f32.max():.3f} | {rt32.min():.3f} / {rt32.max():.3f} |")
