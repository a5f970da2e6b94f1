"""Times surface_distance_metrics (csrc/seg_surface.hip on the fields of csrc/edt.hip) on one GPU:

  metrics  surface_distance_metrics(pred, target, K) on the device, next to signed_distance_maps(target, K) at the same shape
           (the variants alternate inside every round), and against what a user does without it: both label maps to the host,
           per class and entry scipy.ndimage.binary_erosion and distance_transform_edt of both borders, numpy.percentile, and
           the (N, K) results back to the device (host clock around the whole round trip, device synchronised; left out with a
           note when scipy is not installed);
  passes   the kernels of one call from the device activity records of torch.profiler in a pass of its own, grouped into the
           edge pass (clear, edge label maps and counts), the distance fields (the transform's passes) and the reductions
           (digit histograms, selects, sums, finish).

Labels are blobs (tools/boundary_bench.py); pred comes from the same smooth fields with a perturbation, so the two maps differ
along the borders as a prediction does.  Timings as in tools/boundary_bench.py: events around --iters steps after --warmup
steps, the mean of a round, median and (min-max) of --rounds rounds, in ms.  One JSON line per shape; --out DIR keeps them in
DIR/surface_bench.json.

    timeout -k 10 900 python tools/surface_bench.py [--iters 20] [--warmup 5] [--rounds 5] [--cases 0,2] [--out DIR]

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

GROUPS = (("k_surface_clear", "edge pass"), ("k_surface_edges", "edge pass"), ("k_edt_", "distance fields"),
          ("k_surface_", "reductions"))


def blob_pair(shape, seed=0, wobble=0.25):
    """(pred, target) (N, dims) int64 on the device: the argmax over K smooth random fields, and over the same fields with a
    perturbation of `wobble` standard deviations."""
    N, K, sp = shape[0], shape[1], tuple(shape[2:])
    g = torch.Generator(device="cuda").manual_seed(seed)
    size = (N, K) + tuple(max(s // 16, 2) for s in sp)
    coarse = torch.randn(size, device="cuda", generator=g)
    other = coarse + wobble * torch.randn(size, device="cuda", generator=g)
    mode = "bilinear" if len(sp) == 2 else "trilinear"
    up = [torch.nn.functional.interpolate(c, size=sp, mode=mode, align_corners=True).argmax(1).contiguous() for c in (other, coarse)]
    return up[0], up[1]


def scipy_metrics(pred, target, K, q, ndi):
    """The user's path today: (hausdorff, its percentile, assd) per entry and class on the host, back on the device."""
    import numpy as np
    p, y = pred.cpu().numpy(), target.cpu().numpy()
    out = np.full((3, p.shape[0], K), np.nan, dtype=np.float32)
    for n in range(p.shape[0]):
        for k in range(K):
            A, B = p[n] == k, y[n] == k
            ea, eb = A ^ ndi.binary_erosion(A), B ^ ndi.binary_erosion(B)
            if not ea.any() or not eb.any():
                if ea.any() or eb.any():
                    out[:, n, k] = np.inf
                continue
            d0, d1 = ndi.distance_transform_edt(~eb)[ea], ndi.distance_transform_edt(~ea)[eb]
            out[:, n, k] = (max(d0.max(), d1.max()), max(np.percentile(d0, q), np.percentile(d1, q)),
                            (d0.sum() + d1.sum()) / (d0.size + d1.size))
    return torch.from_numpy(out).to(pred.device)


def kernel_groups(step, steps):
    """{group: us per step} and {kernel: us per step} from the device activity records of `steps` steps."""
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
        raise SystemExit("surface_bench needs a GPU")
    from advchain_amd.common.loss import signed_distance_maps
    from advchain_amd.common.metrics import surface_distance_metrics
    try:
        import scipy.ndimage as ndi
    except ImportError:
        ndi = None
    rows = []
    shapes = SHAPES if not args.cases else [SHAPES[int(i)] for i in args.cases.split(",")]
    for shape in shapes:
        K = shape[1]
        pred, target = blob_pair(shape)
        m = surface_distance_metrics(pred, target, K)
        ok = torch.isfinite(m.hausdorff)
        row = dict(shape=list(shape), border_fraction=float(m.surface_voxels.sum()) / (2.0 * pred.numel()),
                   mean_hausdorff=float(m.hausdorff[ok].mean()), mean_hd95=float(m.hausdorff_percentile[ok].mean()),
                   mean_assd=float(m.assd[ok].mean()), mean_dice=float(m.dice[ok].mean()))
        ts = rounds_of({"metrics": lambda: surface_distance_metrics(pred, target, K),
                        "signed_maps": lambda: signed_distance_maps(target, K)}, args.iters, args.warmup, args.rounds)
        row["device"] = {k: stats(v) for k, v in ts.items()}
        if ndi is None:
            row["scipy"] = "scipy is not installed: no host baseline taken"
        else:
            host = []
            for _ in range(args.scipy_rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ref = scipy_metrics(pred, target, K, 95.0, ndi)
                torch.cuda.synchronize()
                host.append(1e3 * (time.perf_counter() - t0))
            row["scipy"] = stats(host)
            got = torch.stack([m.hausdorff, m.hausdorff_percentile, m.assd])
            same = torch.isfinite(ref)
            row["max_rel_diff_to_scipy"] = float(((got - ref).abs()[same] / ref[same].clamp_min(1e-30)).max())
            row["special_values_agree"] = bool(torch.equal(torch.isnan(got), torch.isnan(ref))
                                               and torch.equal(torch.isinf(got), torch.isinf(ref)))
        groups, kernels, launches = kernel_groups(lambda: surface_distance_metrics(pred, target, K), args.profile_steps)
        row["groups_us"], row["kernels_us"], row["launches"] = groups, kernels, launches
        rows.append(row)
        print(json.dumps(row), flush=True)
        del pred, target, m
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "surface_bench.json"), "w") as f:
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
