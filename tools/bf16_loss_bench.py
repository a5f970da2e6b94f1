"""Times forward + backward of the consistency loss with bf16 logits (csrc/loss_lp.hip) with device events:

  (a) native: calc_segmentation_consistency on the operands as they are stored;
  (b) the workaround a bf16 user had before, in the same process: calc_segmentation_consistency(pred.float(), ref.float(), ...)
      -- the cast launch per bf16 operand, the fp32 kernels, and autograd's cast of the gradient back to bf16.

Two storage pairs: bf16 / bf16 (a chain without a geometric transform) and fp32 / bf16 (a geometric solver step: the
warped-back prediction is fp32, init_output bf16).  The prediction requires grad, the reference is a constant, as in the solver.
One-channel mask, mse+kl+contour.  The paths alternate over --rounds; the best round of each is reported (median of --iters).
One JSON line per shape and pair; --out DIR keeps them.

    python tools/bf16_loss_bench.py [--iters 20] [--warmup 5] [--rounds 3] [--cases 0,2] [--native-only] [--out DIR]

Every GPU step runs under a time limit of its own, set on the command line, as for profiles/r10/bf16_loss:

    timeout -k 10 300 python tools/bf16_loss_bench.py --out DIR
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d DIR -- python tools/bf16_loss_bench.py --native-only --cases 1 --rounds 1

(all three shapes and both pairs take well under a minute in one process; --cases I gives a shape a process and a limit of its
own).  --native-only --cases I is the run for `rocprofv3 --kernel-trace --stats`: ONE shape, so that each kernel's time belongs
to it.  Needs a GPU (no fall-back)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TYPES, WEIGHTS = ["mse", "kl", "contour"], [0.7, 1.3, 0.5]
SHAPES = [(32, 4, 256, 256), (32, 20, 256, 256), (4, 4, 128, 128, 64)]
PAIRS = {"bf16/bf16": (torch.bfloat16, torch.bfloat16), "fp32/bf16": (torch.float32, torch.bfloat16)}


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
        raise SystemExit("bf16_loss_bench needs a GPU")
    from advchain_amd.common.loss import calc_segmentation_consistency
    rows = []
    for shape in selected(args.cases):
        g = torch.Generator(device="cuda").manual_seed(0)
        pred32 = torch.randn(shape, device="cuda", generator=g) * 2
        ref32 = torch.randn(shape, device="cuda", generator=g) * 2
        mask = (torch.rand((shape[0], 1) + tuple(shape[2:]), device="cuda", generator=g) > 0.1).float()
        for pair, (pt, rt) in PAIRS.items():
            pred = pred32.to(pt).requires_grad_(True)
            ref = ref32.to(rt)

            def native():
                v = calc_segmentation_consistency(pred, ref, TYPES, WEIGHTS, scales=[0], mask=mask)
                return torch.autograd.grad(v, pred)[0]

            def workaround():
                v = calc_segmentation_consistency(pred.float(), ref.float(), TYPES, WEIGHTS, scales=[0], mask=mask)
                return torch.autograd.grad(v, pred)[0]
            paths = {"native": native} if args.native_only else {"native": native, "workaround": workaround}
            assert native().dtype == pt
            times = {k: [] for k in paths}
            for _ in range(args.rounds):                   # alternate the paths
                for k, fn in paths.items():
                    times[k].append(time_step(fn, args.iters, args.warmup))
            row = dict(shape=list(shape), pair=pair, terms="+".join(TYPES))
            for k in paths:
                row[k + "_us"] = 1e3 * min(times[k])
            if "workaround_us" in row:
                row["native_over_workaround"] = row["native_us"] / row["workaround_us"]
                gn, gw = native().float(), workaround().float()
                row["max_grad_diff_over_max"] = float((gn - gw).abs().max() / gw.abs().max())
            rows.append(row)
            print(json.dumps(row), flush=True)
            del pred, ref
        del pred32, ref32, mask
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bf16_loss_bench%s.json" % ("_native_only" if args.native_only else "")), "w") as f:
            json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default=None, help="comma-separated indices into SHAPES (default: all)")
    run(ap.parse_args())


if __name__ == "__main__":
    main()
