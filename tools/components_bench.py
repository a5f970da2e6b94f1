"""Times common.postprocess (csrc/seg_components.hip) on one GPU:

  calls    connected_components(return_sizes=True), keep_largest_component and remove_small_components(min_size=50) on the
           device, next to signed_distance_maps at the same shape (the variants alternate inside every round), and against what
           a user does without them: the label map to the host, scipy.ndimage.label per entry and class, the same filter in
           numpy, and the result back to the device (host clock around the whole round trip, device synchronised; left out with
           a note when scipy is not installed).  The host results are compared with the device's: they must be equal.
  passes   the kernels of one call from the device activity records of torch.profiler in a pass of its own.

Label maps: the blobs of tools/boundary_bench.py at its three shapes, and a Bernoulli(0.59) mask of class 1 on class 0 -- near the
site-percolation threshold of the square lattice: large tortuous clusters, many seam crossings -- at the first two.  Connectivity
1 and full.  Timings as in tools/boundary_bench.py: events around --iters steps after --warmup steps, the mean of a round, median
and (min-max) of --rounds rounds, in ms.  One JSON line per case; --out DIR keeps them in DIR/components_bench.json.

    timeout -k 10 900 python tools/components_bench.py [--iters 20] [--warmup 5] [--rounds 5] [--cases 0,2] [--out DIR]

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

from tools.boundary_bench import SHAPES, blob_labels, rounds_of, stats  # noqa: E402

MIN_SIZE = 50


def cases():
    """[(shape, map name)]: blobs at every shape, the percolation mask at the first two."""
    return [(s, "blobs") for s in SHAPES] + [(s, "percolation") for s in SHAPES[:2]]


def labels_of(shape, name):
    if name == "blobs":
        return blob_labels(shape)
    g = torch.Generator(device="cuda").manual_seed(1)
    return (torch.rand((shape[0],) + tuple(shape[2:]), device="cuda", generator=g) < 0.59).long()


def host_filters(labels, K, connectivity, ndi):
    """The user's path today: (keep largest component, remove components below MIN_SIZE) per entry and class on the host, back on
    the device.  scipy numbers the components of a mask by their first voxel, and argmax takes the first of equals: the tie rule."""
    import numpy as np
    y = labels.cpu().numpy()
    structure = ndi.generate_binary_structure(y.ndim - 1, connectivity)
    kept, cleaned = y.copy(), y.copy()
    for n in range(y.shape[0]):
        for k in range(1, K):
            lab, m = ndi.label(y[n] == k, structure=structure)
            if m == 0:
                continue
            voxels = np.bincount(lab.reshape(-1))
            voxels[0] = 0
            kept[n][(lab > 0) & (lab != voxels.argmax())] = 0
            cleaned[n][(lab > 0) & (voxels[lab] < MIN_SIZE)] = 0
    return torch.from_numpy(kept).to(labels.device), torch.from_numpy(cleaned).to(labels.device)


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
        found = re.search(r"k_cc_\w+", e.name)
        short = found.group(0) if found else e.name[:60]
        kernels[short] = kernels.get(short, 0.0) + t / steps
        launches += 1
    return kernels, launches / steps


def run(args):
    if not torch.cuda.is_available():
        raise SystemExit("components_bench needs a GPU")
    from advchain_amd.common.loss import signed_distance_maps
    from advchain_amd.common.postprocess import connected_components, keep_largest_component, remove_small_components
    try:
        import scipy.ndimage as ndi
    except ImportError:
        ndi = None
    rows = []
    todo = cases() if not args.cases else [cases()[int(i)] for i in args.cases.split(",")]
    for shape, name in todo:
        K, nd = shape[1], len(shape) - 2
        labels = labels_of(shape, name)
        for connectivity in (1, nd):
            comp = connected_components(labels, connectivity=connectivity, num_classes=K, return_sizes=True)
            row = dict(shape=list(shape), map=name, connectivity=connectivity, voxels=labels.numel(),
                       components_per_entry=float(comp.count.double().mean()), largest=int(comp.sizes.max()))
            variants = {"connected_components": lambda: connected_components(labels, connectivity=connectivity, num_classes=K,
                                                                              return_sizes=True),
                        "keep_largest": lambda: keep_largest_component(labels, K, connectivity=connectivity),
                        "remove_small": lambda: remove_small_components(labels, MIN_SIZE, connectivity=connectivity, num_classes=K),
                        "signed_maps": lambda: signed_distance_maps(labels, K)}
            ts = rounds_of(variants, args.iters, args.warmup, args.rounds)
            row["device"] = {k: stats(v) for k, v in ts.items()}
            if ndi is None or args.scipy_rounds < 1:
                row["scipy"] = "no host baseline taken (scipy is not installed, or --scipy-rounds 0)"
            else:
                host = []
                for _ in range(args.scipy_rounds):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    kept, cleaned = host_filters(labels, K, connectivity, ndi)
                    torch.cuda.synchronize()
                    host.append(1e3 * (time.perf_counter() - t0))
                row["scipy"] = stats(host)                                  # (both filters from one labelling per class)
                row["equal_to_scipy"] = bool(torch.equal(kept, keep_largest_component(labels, K, connectivity=connectivity))
                                             and torch.equal(cleaned, remove_small_components(labels, MIN_SIZE,
                                                                                              connectivity=connectivity,
                                                                                              num_classes=K)))
            row["kernels_us"] = {}
            for call in ("connected_components", "keep_largest"):
                kernels, launches = kernel_times(variants[call], args.profile_steps)
                row["kernels_us"][call] = dict(kernels, launches=launches)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del labels
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "components_bench.json"), "w") as f:
            json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scipy-rounds", type=int, default=2)
    ap.add_argument("--profile-steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default=None, help="comma-separated indices into cases() (default: all)")
    run(ap.parse_args())


if __name__ == "__main__":
    main()
