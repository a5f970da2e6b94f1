"""Times forward + backward of the consistency loss with class weights (the cw entries of csrc/loss_lp.hip) against
class_weights=None on the same operands, with device events:

  (a) weighted:   calc_segmentation_consistency(..., class_weights=w), w cycling through (0.25, 2.0, 0.0, 1.5, 0.5);
  (b) unweighted: calc_segmentation_consistency(..., class_weights=None) -- fp32 / fp32: the register kernels of csrc/loss.hip
      up to 16 classes and the unweighted fp32 kernels of csrc/loss_lp.hip above; bf16 / bf16: the unweighted kernels of csrc/loss_lp.hip.

Both operands require grad (a teacher / student pair); one-channel mask, mse+kl+contour.  Two storage pairs: fp32 / fp32 and
bf16 / bf16.  The paths alternate over --rounds; the best round of each is reported (median of --iters).  One JSON line per
shape and pair; --out DIR keeps them.

    python tools/class_weights_bench.py [--iters 20] [--warmup 5] [--rounds 3] [--cases 0,2] [--unweighted-only] [--out DIR]

--unweighted-only times (b) alone and passes no weights: this file copied into a checkout of an earlier commit gives that
commit's unweighted timings (profiles/r11/class_weights/summary.md takes them at the parent commit, in the same session).
Every GPU step runs under a time limit of its own, set on the command line:

    timeout -k 10 300 python tools/class_weights_bench.py --out DIR

(all three shapes and both pairs take well under a minute in one process).  Needs a GPU (no fall-back)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TYPES, WEIGHTS = ["mse", "kl", "contour"], [0.7, 1.3, 0.5]
SHAPES = [(32, 4, 256, 256), (32, 20, 256, 256), (4, 4, 128, 128, 64)]
PAIRS = {"fp32/fp32": (torch.float32, torch.float32), "bf16/bf16": (torch.bfloat16, torch.bfloat16)}
CYCLE = (0.25, 2.0, 0.0, 1.5, 0.5)


def selected(spec):
    return SHAPES if not spec else [SHAPES[int(i)] for i in spec.split(",")]


def time_step(step, iters, warmup):
    """Median ms of one forward + backward: device events around `step`, `iters` evaluations."""
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(iters)]
    for a, b in ev:
        a.record()
        step()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[len(t) // 2]


def run(args):
    if not torch.cuda.is_available():
        raise SystemExit("class_weights_bench needs a GPU")
    from advchain_amd.common.loss import calc_segmentation_consistency
    rows = []
    for shape in selected(args.cases):
        g = torch.Generator(device="cuda").manual_seed(0)
        pred32 = torch.randn(shape, device="cuda", generator=g) * 2
        ref32 = torch.randn(shape, device="cuda", generator=g) * 2
        mask = (torch.rand((shape[0], 1) + tuple(shape[2:]), device="cuda", generator=g) > 0.1).float()
        w = [CYCLE[k % len(CYCLE)] for k in range(shape[1])]
        for pair, (pt, rt) in PAIRS.items():
            pred = pred32.to(pt).requires_grad_(True)
            ref = ref32.to(rt).requires_grad_(True)

            def unweighted():
                v = calc_segmentation_consistency(pred, ref, TYPES, WEIGHTS, scales=[0], mask=mask)
                return torch.autograd.grad(v, (pred, ref))

            def weighted():
                v = calc_segmentation_consistency(pred, ref, TYPES, WEIGHTS, class_weights=w, scales=[0], mask=mask)
                return torch.autograd.grad(v, (pred, ref))
            paths = {"unweighted": unweighted} if args.unweighted_only else {"weighted": weighted, "unweighted": unweighted}
            times = {k: [] for k in paths}
            for _ in range(args.rounds):                   # alternate the paths
                for k, fn in paths.items():
                    times[k].append(time_step(fn, args.iters, args.warmup))
            row = dict(shape=list(shape), pair=pair, terms="+".join(TYPES))
            for k in paths:
                row[k + "_us"] = 1e3 * min(times[k])
            if "weighted_us" in row:
                row["weighted_over_unweighted"] = row["weighted_us"] / row["unweighted_us"]
            rows.append(row)
            print(json.dumps(row), flush=True)
            del pred, ref
        del pred32, ref32, mask
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "class_weights_bench%s.json" % ("_unweighted_only" if args.unweighted_only else "")), "w") as f:
            json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--unweighted-only", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default=None, help="comma-separated indices into SHAPES (default: all)")
    run(ap.parse_args())


if __name__ == "__main__":
    main()
