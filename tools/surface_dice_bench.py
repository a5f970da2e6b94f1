"""Times surface_dice (csrc/seg_surface.hip: the ball route k_surface_ball, the field route on the fields of csrc/edt.hip) on one
GPU, at the shapes of tools/boundary_bench.py and tolerances of 1, 2, 3 and 5 voxels:

  routes   ops.surface_dice(pred, target, K, tolerance, route="ball") and route="fields", next to
           surface_distance_metrics(pred, target, K) at the same shape (the three alternate inside every round), and against what
           a user does without it: both label maps to the host, per class and entry scipy.ndimage.binary_erosion of both masks,
           distance_transform_edt of both borders, <= tolerance, and the (N, K) result back to the device (host clock around the
           whole round trip, device synchronised, at one tolerance: its cost does not depend on it; left out with a note when
           scipy is not installed);
  passes   the kernels of one call of each route from the device activity records of torch.profiler in a pass of its own,
           grouped into clear / finish, the ball kernel, the edge pass, the distance fields and the count pass.

Labels are the blobs of tools/surface_bench.py.  Timings as in tools/boundary_bench.py: events around --iters steps after
--warmup steps, the mean of a round, median and (min-max) of --rounds rounds, in ms.  One JSON line per shape; --out DIR keeps
them in DIR/surface_dice_bench.json.  The two routes must return the same bits: the tool stops if they do not.

    timeout -k 10 900 python tools/surface_dice_bench.py [--iters 20] [--warmup 5] [--rounds 5] [--cases 0,2] [--out DIR]

Needs a GPU (no fall-back)."""
import argparse
import json
import os
import re
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.boundary_bench import SHAPES, rounds_of, stats  # noqa: E402
from tools.surface_bench import blob_pair  # noqa: E402

TOLERANCES = (1, 2, 3, 5)
GROUPS = (("k_surface_dice_clear", "clear and finish"), ("k_surface_dice_finish", "clear and finish"), ("k_surface_ball", "ball"),
          ("k_surface_edges", "edge pass"), ("k_edt_", "distance fields"), ("k_surface_within", "count pass"))


def scipy_dice(pred, target, K, tau, ndi):
    """The user's path today: the (N, K) surface Dice on the host, back on the device."""
    import numpy as np
    p, y = pred.cpu().numpy(), target.cpu().numpy()
    out = np.full((p.shape[0], K), np.nan, dtype=np.float32)
    for n in range(p.shape[0]):
        for k in range(K):
            A, B = p[n] == k, y[n] == k
            ea, eb = A ^ ndi.binary_erosion(A), B ^ ndi.binary_erosion(B)
            m = int(ea.sum()) + int(eb.sum())
            if m == 0:
                continue
            c = 0
            if ea.any() and eb.any():
                c = int((ndi.distance_transform_edt(~eb)[ea] <= tau).sum()) + int((ndi.distance_transform_edt(~ea)[eb] <= tau).sum())
            out[n, k] = c / m
    return torch.from_numpy(out).to(pred.device)


def kernel_groups(step, steps):
    """{group: us per step}, {kernel: us per step} and the launches per step from the device activity records of `steps` steps."""
    from torch.profiler import ProfilerActivity, profile
    step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
    groups, kernels, launches = {}, {}, 0
    for e in prof.events():
        if getattr(e, "device_type", None) is None or "cuda" not in str(e.device_type).lower():
            continue
        if any(w in e.name.lower() for w in ("memcpy", "memset")):
            continue
        t = float(getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0))
        group = next((g for key, g in GROUPS if key in e.name), "other")
        found = re.search(r"k_\w+(<[^>]*>)?", e.name)
        short = found.group(0) if found else e.name[:60]
        groups[group] = groups.get(group, 0.0) + t / steps
        kernels[short] = kernels.get(short, 0.0) + t / steps
        launches += 1
    return groups, kernels, launches / steps


def run(args):
    if not torch.cuda.is_available():
        raise SystemExit("surface_dice_bench needs a GPU")
    from advchain_amd import ops
    from advchain_amd.common.metrics import surface_distance_metrics
    try:
        import scipy.ndimage as ndi
    except ImportError:
        ndi = None
    rows = []
    shapes = SHAPES if not args.cases else [SHAPES[int(i)] for i in args.cases.split(",")]
    for shape in shapes:
        N, K, sp = shape[0], shape[1], tuple(shape[2:])
        pred, target = blob_pair(shape)
        row = dict(shape=list(shape), tolerances={})
        for tau in TOLERANCES:
            ball = ops.surface_dice(pred, target, K, tau, route="ball")
            fields = ops.surface_dice(pred, target, K, tau, route="fields")
            if not all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                   b.view(torch.int32) if b.dtype == torch.float32 else b) for a, b in zip(ball, fields)):
                raise SystemExit("the two routes differ at %s, tolerance %g" % (shape, tau))
            ok = torch.isfinite(ball.surface_dice)
            cell = dict(dispatch=ops.surface_dice_route(N, K, sp, tau), mean_surface_dice=float(ball.surface_dice[ok].mean()),
                        border_fraction=float(ball.surface_voxels.sum()) / (2.0 * pred.numel()))
            ts = rounds_of({"ball": lambda: ops.surface_dice(pred, target, K, tau, route="ball"),
                            "fields": lambda: ops.surface_dice(pred, target, K, tau, route="fields"),
                            "surface_distance_metrics": lambda: surface_distance_metrics(pred, target, K)},
                           args.iters, args.warmup, args.rounds)
            cell["device"] = {k: stats(v) for k, v in ts.items()}
            cell["passes"] = {}
            for route in ("ball", "fields"):
                groups, kernels, launches = kernel_groups(lambda: ops.surface_dice(pred, target, K, tau, route=route), args.profile_steps)
                cell["passes"][route] = dict(groups_us=groups, kernels_us=kernels, launches=launches)
            row["tolerances"][str(tau)] = cell
        if ndi is None:
            row["scipy"] = "scipy is not installed: no host baseline taken"
        else:
            host = []
            for _ in range(args.scipy_rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ref = scipy_dice(pred, target, K, 2, ndi)
                torch.cuda.synchronize()
                host.append(1e3 * (time.perf_counter() - t0))
            row["scipy"] = stats(host)
            got = ops.surface_dice(pred, target, K, 2).surface_dice
            row["equal_to_scipy_at_2"] = bool(torch.equal(torch.isnan(got), torch.isnan(ref))
                                              and torch.equal(got[~torch.isnan(got)], ref[~torch.isnan(ref)]))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del pred, target
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "surface_dice_bench.json"), "w") as f:
            json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scipy-rounds", type=int, default=2)
    ap.add_argument("--profile-steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default=None, help="comma-separated indices into SHAPES (default: all)")
    run(ap.parse_args())


if __name__ == "__main__":
    main()
