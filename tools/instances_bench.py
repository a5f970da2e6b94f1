"""Times common.metrics.instance_metrics (csrc/seg_components.hip) on one GPU:

  calls    instance_metrics(pred, target, K) with and without the status maps, next to its yardstick on the device: two
           connected_components(return_sizes=True) calls on the same maps, the labelling the call contains (the variants alternate
           inside every round), and against what a user does without it: both maps to the host, scipy.ndimage.label per entry
           and class, a numpy contingency table per entry and class, the match rule on it (host clock around the whole round
           trip, device synchronised; left out with a note when scipy is not installed).  The host counts are compared with the
           device's: they must be equal.
  passes   the kernels of one call from the device activity records of torch.profiler in a pass of its own.

Label pairs: the blob pair of tools/surface_bench.py at the three shapes of tools/boundary_bench.py, and a lesion pair at the
same shapes: cells of 16 voxels per axis, in 7 of 10 a box of 2-10 voxels per axis in target and the box shifted by -1..1 and
resized by -2..2 per axis in pred, one box in ten missing from each map.  Connectivity 1 and full.  Timings as in
tools/boundary_bench.py.  One JSON line per case; --out DIR keeps them in DIR/instances_bench.json.

    timeout -k 10 900 python tools/instances_bench.py [--iters 20] [--warmup 5] [--rounds 5] [--cases 0,3] [--out DIR]

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

CELL = 16


def cases():
    return [(s, "blobs") for s in SHAPES] + [(s, "lesions") for s in SHAPES]


def lesion_pair(shape, seed=0, device="cuda"):
    """(pred, target) (N, dims) int64 on the device, classes 1 .. K-1 on background 0; the spatial sizes are multiples of CELL."""
    N, K, sp = shape[0], shape[1], tuple(shape[2:])
    g = torch.Generator(device=device).manual_seed(seed)
    grid = (N,) + tuple(s // CELL for s in sp)

    def draw(lo, hi):
        return torch.randint(lo, hi, grid, device=device, generator=g)

    def per_voxel(t):
        for a in range(len(sp)):
            t = t.repeat_interleave(CELL, dim=a + 1)
        return t

    klass, present = per_voxel(draw(1, K)), per_voxel(draw(0, 10))
    inside = [present >= 3, present >= 3]                                       # pred, target
    for a, s in enumerate(sp):
        size = draw(2, 11)
        start = 1 + draw(0, 1 << 20) % (CELL - 1 - size)
        local = (torch.arange(s, device=device) % CELL).view((1,) * (a + 1) + (s,) + (1,) * (len(sp) - a - 1))
        for which, (lo, n) in enumerate(((start + draw(-1, 2), size + draw(-2, 3)), (start, size))):
            inside[which] = inside[which] & (local >= per_voxel(lo)) & (local < per_voxel(lo + n))
    pred = torch.where(inside[0] & (present != 3), klass, 0)
    target = torch.where(inside[1] & (present != 4), klass, 0)
    return pred.contiguous(), target.contiguous()


def pair_of(shape, name):
    return blob_pair(shape) if name == "blobs" else lesion_pair(shape)


def host_counts(pred, target, K, connectivity, threshold, ndi):
    """The user's path today: (components (N,K,2), matched (N,K), iou_fixed (N,K)) from scipy.ndimage.label per entry and class
    and a contingency table in numpy."""
    import numpy as np
    p, t = pred.cpu().numpy(), target.cpu().numpy()
    structure = ndi.generate_binary_structure(p.ndim - 1, connectivity)
    N = p.shape[0]
    components = np.zeros((N, K, 2), dtype=np.int64)
    matched = np.zeros((N, K), dtype=np.int64)
    iou_fixed = np.zeros((N, K), dtype=np.int64)
    for n in range(N):
        for k in range(1, K):
            lp, mp = ndi.label(p[n] == k, structure=structure)
            lt, mt = ndi.label(t[n] == k, structure=structure)
            components[n, k] = (mp, mt)
            if mp == 0 or mt == 0:
                continue
            both = (lp > 0) & (lt > 0)
            keys, I = np.unique(lp[both].astype(np.int64) * (mt + 1) + lt[both], return_counts=True)
            U = np.bincount(lp.reshape(-1))[keys // (mt + 1)] + np.bincount(lt.reshape(-1))[keys % (mt + 1)] - I
            match = I.astype(np.float64) > threshold * U.astype(np.float64)
            matched[n, k] = int(match.sum())
            iou_fixed[n, k] = sum((int(i) << 32) // int(u) for i, u in zip(I[match], U[match]))
    return components, matched, iou_fixed


def kernel_times(step, steps):
    """({kernel: us per step}, launches per step) from the device activity records of `steps` steps."""
    from torch.profiler import ProfilerActivity, profile
    step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
    kernels, launches = {}, 0
    for e in prof.events():
        if getattr(e, "device_type", None) is None or "cuda" not in str(e.device_type).lower():
            continue
        if any(w in e.name.lower() for w in ("memcpy", "memset")):
            continue
        t = float(getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0))
        found = re.search(r"k_(cc|inst)_\w+", e.name)
        short = found.group(0) if found else e.name[:60]
        kernels[short] = kernels.get(short, 0.0) + t / steps
        launches += 1
    return kernels, launches / steps


def run(args):
    if not torch.cuda.is_available():
        raise SystemExit("instances_bench needs a GPU")
    from advchain_amd import _lib
    from advchain_amd.common.metrics import instance_metrics
    from advchain_amd.common.postprocess import connected_components
    try:
        import scipy.ndimage as ndi
    except ImportError:
        ndi = None
    rows = []
    todo = cases() if not args.cases else [cases()[int(i)] for i in args.cases.split(",")]
    for shape, name in todo:
        K, nd = shape[1], len(shape) - 2
        pred, target = pair_of(shape, name)
        words = _lib.load().advchain_instance_match_workspace(shape[0], nd, _lib.dims_array(tuple(shape[2:])))
        for connectivity in (1, nd):
            m = instance_metrics(pred, target, K, connectivity=connectivity)
            row = dict(shape=list(shape), map=name, connectivity=connectivity, voxels=pred.numel(),
                       workspace_bytes_per_voxel=4.0 * words / pred.numel(),
                       components_per_entry=[float(x) for x in m.components.sum(1).double().mean(0)],
                       matched_per_entry=float(m.matched.sum(1).double().mean()),
                       overlapping_per_entry=[float(x) for x in m.overlapping.sum(1).double().mean(0)])
            variants = {"instance_metrics": lambda: instance_metrics(pred, target, K, connectivity=connectivity),
                        "instance_metrics_maps": lambda: instance_metrics(pred, target, K, connectivity=connectivity,
                                                                          return_maps=True),
                        "two_labellings": lambda: (connected_components(pred, connectivity=connectivity, num_classes=K,
                                                                        return_sizes=True),
                                                   connected_components(target, connectivity=connectivity, num_classes=K,
                                                                        return_sizes=True))}
            ts = rounds_of(variants, args.iters, args.warmup, args.rounds)
            row["device"] = {k: stats(v) for k, v in ts.items()}
            if ndi is None or args.scipy_rounds < 1:
                row["scipy"] = "no host baseline taken (scipy is not installed, or --scipy-rounds 0)"
            else:
                host = []
                for _ in range(args.scipy_rounds):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    got = host_counts(pred, target, K, connectivity, 0.5, ndi)
                    host.append(1e3 * (time.perf_counter() - t0))
                row["scipy"] = stats(host)
                row["equal_to_scipy"] = all(bool((torch.from_numpy(h) == d.cpu()).all())
                                            for h, d in zip(got, (m.components, m.matched, m.iou_fixed)))
            kernels, launches = kernel_times(variants["instance_metrics_maps"], args.profile_steps)
            row["kernels_us"] = dict(kernels, launches=launches)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del pred, target
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "instances_bench.json"), "w") as f:
            json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scipy-rounds", type=int, default=1)
    ap.add_argument("--profile-steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default=None, help="comma-separated indices into cases() (default: all)")
    run(ap.parse_args())


if __name__ == "__main__":
    main()
