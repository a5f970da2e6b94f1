"""Times common.loss.cldice_loss (csrc/seg_skeleton.hip), forward plus backward, on one GPU:

  hip      cldice_loss(logits, labels, iterations) and its gradient for the logits
  torch    the stock composition on the same device: the published soft_cldice (tests/skeleton_forms.py: max_pool launches and
           elementwise glue, autograd keeps every intermediate) on softmax(logits) and the one-hot labels, and its gradient
  dice     dice_loss at the same shape and its gradient, for scale
  routes   the forward of the soft skeleton alone by its two routes, `fused` (LDS tiles) and `levels`, where both can run

at (32, 4, 256, 256), (4, 4, 128, 128, 64) and (32, 20, 256, 256), iterations 3 and 10, fp32 and bf16 logits.  The variants
alternate inside every round (tools/boundary_bench.py: device events around `iters` steps, median of the rounds).  One JSON line
per case; --out DIR keeps them in DIR/cldice_bench.json.

    timeout -k 10 900 python tools/cldice_bench.py [--iters 10] [--warmup 3] [--rounds 5] [--out DIR]

Needs a GPU (no fall-back)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.boundary_bench import rounds_of, stats  # noqa: E402

SHAPES = [(32, 4, 256, 256), (4, 4, 128, 128, 64), (32, 20, 256, 256)]
ITERATIONS = [3, 10]


def run(args):
    if not torch.cuda.is_available():
        raise SystemExit("cldice_bench needs a GPU")
    from advchain_amd import ops
    from advchain_amd.common.loss import cldice_loss, dice_loss
    from tests.skeleton_forms import one_hot_no_class, soft_cldice_published
    dev = torch.device("cuda")
    rows = []
    shapes = [s for s in SHAPES if args.only is None or len(s) - 2 == args.only]
    for shape in shapes:
        K = shape[1]
        g = torch.Generator().manual_seed(0)
        x32 = (torch.randn(shape, generator=g) * 2).to(dev)
        y = torch.randint(0, K, (shape[0],) + tuple(shape[2:]), generator=g).to(dev)
        t = one_hot_no_class(y, K, torch.float32)
        for dtype in (torch.float32, torch.bfloat16):
            x = x32.to(dtype).requires_grad_(True)
            for iterations in ITERATIONS:
                def hip():
                    return torch.autograd.grad(cldice_loss(x, y, iterations=iterations, ignore_background=True, batch=True), x)

                def stock():
                    p = torch.softmax(x.float(), 1)
                    return torch.autograd.grad(soft_cldice_published(t, p, iterations, 1.0), x)

                def dice():
                    return torch.autograd.grad(dice_loss(x, y), x)

                v_hip = float(cldice_loss(x, y, iterations=iterations, ignore_background=True, batch=True))
                v_torch = float(soft_cldice_published(t, torch.softmax(x.float(), 1), iterations, 1.0)) if K == 2 else None
                ts = rounds_of({"hip": hip, "torch": stock, "dice": dice}, args.iters, args.warmup, args.rounds)
                row = dict(shape=list(shape), dtype=str(dtype).replace("torch.", ""), iterations=iterations, value=v_hip,
                           value_torch_pooled=v_torch, ms={k: stats(v) for k, v in ts.items()})
                row["torch_over_hip"] = row["ms"]["torch"]["median_ms"] / row["ms"]["hip"]["median_ms"]
                row["hip_over_dice"] = row["ms"]["hip"]["median_ms"] / row["ms"]["dice"]["median_ms"]
                if dtype == torch.float32 and iterations <= ops.SKELETON_FUSED_MAX_ITERATIONS:
                    with torch.no_grad():
                        p = torch.softmax(x32, 1)
                        rs = rounds_of({r: (lambda r=r: ops.soft_skeletonize(p, iterations=iterations, route=r))
                                        for r in ("fused", "levels")}, args.iters, args.warmup, args.rounds)
                        row["skeleton_forward_ms"] = {k: stats(v) for k, v in rs.items()}
                        del p
                rows.append(row)
                print(json.dumps(row), flush=True)
                torch.cuda.empty_cache()
            del x
        del x32, y, t
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        name = "cldice_bench.json" if args.only is None else "cldice_bench_%dd.json" % args.only
        with open(os.path.join(args.out, name), "w") as f:
            json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", type=int, default=None, choices=(2, 3), help="only the 2D or only the 3D shapes")
    ap.add_argument("--out", default=None)
    run(ap.parse_args())


if __name__ == "__main__":
    main()
