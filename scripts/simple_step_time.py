"""Times rnnt_loss_simple forward + backward (bench.py's simple_step) on bench.py's inputs multiplied by --scale: 0.05 is a
near-uniform model, the start of training, where nearly every lattice block is live and the backward has nothing to skip.
--root DIR imports the package of another checkout (a built parent tree), so that scripts/live_noskip_ab.sh can interleave
two builds.  Prints one line: us per step of each of --repeats timed loops.
python scripts/simple_step_time.py [--config c3] [--scale 0.05] [--steps 50] [--warmup 10] [--repeats 3] [--root DIR]"""
import argparse, os, sys
ap = argparse.ArgumentParser()
ap.add_argument("--config", default="c3"); ap.add_argument("--scale", type=float, default=0.05)
ap.add_argument("--steps", type=int, default=50); ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--repeats", type=int, default=3); ap.add_argument("--root", default=None); ap.add_argument("--label", default="")
args = ap.parse_args()
ROOT = os.path.abspath(args.root) if args.root else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tf-fast-rnnt_amd"))
os.environ.setdefault("FTR_GEMM_TUNE", "second")     # the library GEMMs with their measured kernel choice, as bench.py runs them
import torch
import bench
B, T, S, C, _ = bench.CONFIGS[args.config]
dev = torch.device("cuda:0")
inp = bench.make_inputs(B, T, S, C, 1000, dev)
inp["am"] = inp["am"] * args.scale; inp["lm"] = inp["lm"] * args.scale
for _ in range(args.warmup):
    bench.simple_step(inp)
torch.cuda.synchronize()
out = []
for _ in range(args.repeats):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        loss = bench.simple_step(inp)
    e1.record(); torch.cuda.synchronize()
    out.append(e0.elapsed_time(e1) * 1000 / args.steps)
print(f"{args.label or ROOT} {args.config} scale {args.scale} FTR_BWD_LIVE={os.environ.get('FTR_BWD_LIVE', '')}: "
      + " ".join(f"{v:.1f}" for v in out) + f" us/step, loss {float(loss):.6g}")
