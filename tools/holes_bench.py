"""Times common.postprocess.fill_holes / find_holes (csrc/seg_components.hip) on one GPU:

  calls    fill_holes and find_holes on the device, next to keep_largest_component on the same map (the variants alternate inside
           every round), and against what a user does without them: the label map to the host, scipy.ndimage.binary_fill_holes
           per entry and class, the single-class rule applied to its candidates (a component of the background is filled with k
           only when every neighbour of it that is not background is k), and the result back to the device (host clock around
           the whole round trip, device synchronised; left out with a note when scipy is not installed).  The host result is
           compared with the device's: it must be equal.
  passes   the kernels of one call from the device activity records of torch.profiler in a pass of its own.

Label maps: the blobs of tools/boundary_bench.py at its three shapes with --cavities cavities of mixed size (boxes of 1 to 6
voxels per axis) of class 0 punched into every entry, and the Bernoulli(0.59) mask of tools/components_bench.py at the first
two.  Connectivity 1 and full.  Timings as in tools/components_bench.py: events around --iters steps after --warmup steps, the
mean of a round, median and (min-max) of --rounds rounds, in ms.  One JSON line per case; --out DIR keeps them in
DIR/holes_bench.json.

    timeout -k 10 900 python tools/holes_bench.py [--iters 20] [--warmup 5] [--rounds 5] [--cases 0,2] [--out DIR]

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

from tools.boundary_bench import rounds_of, stats  # noqa: E402
from tools.components_bench import cases, labels_of  # noqa: E402


def punched(shape, name, cavities):
    """labels_of(shape, name); the blobs with `cavities` boxes of class 0 per entry, 1 to 6 voxels along every axis."""
    labels = labels_of(shape, name)
    if name != "blobs":
        return labels
    g = torch.Generator().manual_seed(3)
    sp = tuple(labels.shape[1:])
    for n in range(labels.shape[0]):
        for _ in range(cavities):
            size = [int(torch.randint(1, 7, (1,), generator=g)) for _ in sp]
            at = [int(torch.randint(1, s - e, (1,), generator=g)) for s, e in zip(sp, size)]
            labels[(n,) + tuple(slice(a, a + e) for a, e in zip(at, size))] = 0
    return labels


def host_fill(labels, K, connectivity, ndi):
    """The user's path today, for background 0.  binary_fill_holes of class k gives the background voxels that the class cuts off
    from the border; of those, the components of the background whose neighbours are all k are filled with k."""
    import numpy as np
    y = labels.cpu().numpy()
    structure = ndi.generate_binary_structure(y.ndim - 1, connectivity)
    out = y.copy()
    big = 1 << 40                                  # (beyond every label; the filters go through float64)
    for n in range(y.shape[0]):
        bg = y[n] == 0
        lab, m = ndi.label(bg, structure=structure)
        if m == 0:
            continue
        index = np.arange(1, m + 1)
        low = ndi.minimum(ndi.minimum_filter(np.where(bg, big, y[n]), footprint=structure, mode="nearest"), lab, index)
        high = ndi.maximum(ndi.maximum_filter(np.where(bg, -big, y[n]), footprint=structure, mode="nearest"), lab, index)
        for k in range(1, K):
            single = np.zeros(m + 1, dtype=bool)
            single[1:] = (low == k) & (high == k)
            if not single.any():
                continue
            mask = y[n] == k
            cut_off = ndi.binary_fill_holes(mask, structure=structure) & bg
            out[n][cut_off & single[lab]] = k
    return torch.from_numpy(out).to(labels.device)


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
        found = re.search(r"k_(cc|hole)_\w+", e.name)
        short = found.group(0) if found else e.name[:60]
        kernels[short] = kernels.get(short, 0.0) + t / steps
        launches += 1
    return kernels, launches / steps


def run(args):
    if not torch.cuda.is_available():
        raise SystemExit("holes_bench needs a GPU")
    from advchain_amd.common.postprocess import fill_holes, find_holes, keep_largest_component
    try:
        import scipy.ndimage as ndi
    except ImportError:
        ndi = None
    rows = []
    todo = cases() if not args.cases else [cases()[int(i)] for i in args.cases.split(",")]
    for shape, name in todo:
        K, nd = shape[1], len(shape) - 2
        labels = punched(shape, name, args.cavities)
        for connectivity in (1, nd):
            h = find_holes(labels, K, connectivity=connectivity)
            row = dict(shape=list(shape), map=name, connectivity=connectivity, voxels=labels.numel(),
                       background_share=float((labels == 0).double().mean()),
                       holes_per_entry=float(h.count.sum(1).double().mean()), voxels_filled_per_entry=float(h.voxels.sum(1).double().mean()))
            variants = {"fill_holes": lambda: fill_holes(labels, K, connectivity=connectivity),
                        "find_holes": lambda: find_holes(labels, K, connectivity=connectivity),
                        "keep_largest": lambda: keep_largest_component(labels, K, connectivity=connectivity)}
            ts = rounds_of(variants, args.iters, args.warmup, args.rounds)
            row["device"] = {k: stats(v) for k, v in ts.items()}
            if ndi is None or args.scipy_rounds < 1:
                row["scipy"] = "no host baseline taken (scipy is not installed, or --scipy-rounds 0)"
            else:
                host = []
                for _ in range(args.scipy_rounds):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    filled = host_fill(labels, K, connectivity, ndi)
                    torch.cuda.synchronize()
                    host.append(1e3 * (time.perf_counter() - t0))
                row["scipy"] = stats(host)
                row["equal_to_scipy"] = bool(torch.equal(filled, fill_holes(labels, K, connectivity=connectivity)))
            row["kernels_us"] = {}
            for call in ("fill_holes", "keep_largest"):
                kernels, launches = kernel_times(variants[call], args.profile_steps)
                row["kernels_us"][call] = dict(kernels, launches=launches)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del labels
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "holes_bench.json"), "w") as f:
            json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scipy-rounds", type=int, default=2)
    ap.add_argument("--profile-steps", type=int, default=5)
    ap.add_argument("--cavities", type=int, default=40)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default=None, help="comma-separated indices into cases() (default: all)")
    run(ap.parse_args())


if __name__ == "__main__":
    main()
