"""Times common.metrics.betti_numbers (csrc/seg_components.hip) on one GPU:

  calls    betti_numbers(labels, K) at connectivity 1 and ndim, next to its yardstick on the device: connected_components of the
           same map with num_classes=K, one labelling (the variants alternate inside every round), and against the form on the
           host: the map to the host, scipy.ndimage.label per entry and class for the components and the complement and the cells
           of the Euler characteristic counted in numpy (tests/topology_forms.py; host clock around the whole round trip, device
           synchronised).  The host numbers are compared with the device's: they must be equal.
  passes   the kernels of one call from the device activity records of torch.profiler in a pass of its own.

Label maps: the blobs of tools/boundary_bench.py (argmax over K smooth random fields) at (4, 4, 256, 256) and (2, 4, 64, 128, 128).
Timings as in tools/boundary_bench.py.  One JSON line per case; --out DIR keeps them in DIR/topology_bench.json.

    timeout -k 10 600 python tools/topology_bench.py [--iters 20] [--warmup 5] [--rounds 5] [--out DIR]

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

from tools.boundary_bench import blob_labels, rounds_of, stats  # noqa: E402

SHAPES = [(4, 4, 256, 256), (2, 4, 64, 128, 128)]


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
        found = re.search(r"k_(cc|betti)_\w+", e.name)
        short = found.group(0) if found else e.name[:60]
        if found and re.search(r"k_cc_(tile|seam)<2>", e.name):                 # (the labelling of a complement)
            short += "<complement>"
        kernels[short] = kernels.get(short, 0.0) + t / steps
        launches += 1
    return kernels, launches / steps


def run(args):
    if not torch.cuda.is_available():
        raise SystemExit("topology_bench needs a GPU")
    from advchain_amd.common.metrics import betti_numbers
    from advchain_amd.common.postprocess import connected_components
    from tests import topology_forms as T
    rows = []
    for shape in SHAPES:
        K, nd = shape[1], len(shape) - 2
        labels = blob_labels(shape)
        for connectivity in (1, nd):
            got = betti_numbers(labels, K, connectivity=connectivity)
            row = dict(shape=list(shape), connectivity=connectivity, voxels=labels.numel(),
                       betti_per_entry=[float(x) for x in got.betti.sum(1).double().mean(0)])
            variants = {"betti_numbers": lambda: betti_numbers(labels, K, connectivity=connectivity),
                        "one_labelling": lambda: connected_components(labels, connectivity=connectivity, num_classes=K,
                                                                      background=-1)}
            ts = rounds_of(variants, args.iters, args.warmup, args.rounds)
            row["device"] = {k: stats(v) for k, v in ts.items()}
            host = []
            for _ in range(args.scipy_rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                want = T.betti_form(labels, K, connectivity)
                host.append(1e3 * (time.perf_counter() - t0))
            if host:
                row["scipy"] = stats(host)
                row["equal_to_scipy"] = bool(torch.equal(got.betti.cpu(), want[0]) and torch.equal(got.euler.cpu(), want[1]))
            kernels, launches = kernel_times(variants["betti_numbers"], args.profile_steps)
            row["kernels_us"] = dict(kernels, launches=launches)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del labels
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "topology_bench.json"), "w") as f:
            json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scipy-rounds", type=int, default=1)
    ap.add_argument("--profile-steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    run(ap.parse_args())


if __name__ == "__main__":
    main()
