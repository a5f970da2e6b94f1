"""Times the gradient of the consistency loss with respect to the REFERENCE (csrc/loss_ref.hip, through ops.consistency_sums
with a reference that requires grad), backward only, with device events:

  (a) the new entry alone (prediction detached) -- for K <= 4 in both of its forms (ops.REF_GRAD_REG_MAX_K = 4 against = 0);
  (b) the prediction-side backward of the same call (reference detached): the existing kernels, unchanged;
  (c) ATen autograd of the same loss written out in torch (tools/wide_loss_bench.py: aten_loss) with only the reference
      requiring grad -- the outside yardstick.

One-channel mask, mse+kl+contour.  The paths alternate over --rounds; the best round of each is reported.  One JSON line per
shape; --out DIR keeps them.

    python tools/ref_grad_bench.py [--iters 20] [--warmup 5] [--rounds 3] [--cases 0,2] [--hip-only] [--out DIR]
    python tools/ref_grad_bench.py --summarize STATS_CSV --cases 1 [--out DIR]

--hip-only --cases I is the run for `rocprofv3 --kernel-trace --stats` (program after `--`): ONE shape, so that each kernel's
time belongs to it; --summarize turns its stats file into per-kernel times and bandwidth.  Needs a GPU (no fall-back).

Algorithmic bytes per voxel and sample of (a), from the shapes (fp32, one-channel mask):
  pred 4K + ref 4K + mask 4 + R 8(K-1) + grad_ref 4K  (+ statistics 16 where the wide forward saved them).
What the run-time form moves beyond that -- its prologue sweep over the logits for K <= 16, the re-read of ref and grad_ref in
the second sweep, the halo of the R tiles -- is its own overhead and shows as a lower share of the peak."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from wide_loss_bench import PEAK_BPS, aten_loss, coefficients      # noqa: E402

MIX = "mse+kl+contour"
SHAPES = [(32, 4, 256, 256), (32, 20, 256, 256), (4, 4, 128, 128, 64)]
PRED_SIDE = ("k_consistency_bwd", "k_loss_fused_bwd", "k_lp_bwd")


def selected(spec):
    return SHAPES if not spec else [SHAPES[int(i)] for i in spec.split(",")]


def algorithmic_bytes(shape):
    N, K = shape[:2]
    pts = N
    for s in shape[2:]:
        pts *= s
    return pts * (12 * K + 4 + 8 * (K - 1) + (16 if K >= 17 else 0))


def time_backward(fwd, x, iters, warmup):
    """Median ms of the backward alone: device events around torch.autograd.grad, `iters` evaluations."""
    for _ in range(warmup):
        torch.autograd.grad(fwd(), x)
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(iters)]
    for a, b in ev:
        v = fwd()
        a.record()
        torch.autograd.grad(v, x)
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[len(t) // 2]


def run(args):
    if not torch.cuda.is_available():
        raise SystemExit("ref_grad_bench needs a GPU")
    from advchain_amd import ops
    rows = []
    for shape in selected(args.cases):
        g = torch.Generator(device="cuda").manual_seed(0)
        pred = torch.randn(shape, device="cuda", generator=g) * 2
        ref = torch.randn(shape, device="cuda", generator=g) * 2
        mask = (torch.rand((shape[0], 1) + tuple(shape[2:]), device="cuda", generator=g) > 0.1).float()
        coef = coefficients(shape, MIX)
        K = shape[1]
        pred_g, ref_g = pred.clone().requires_grad_(True), ref.clone().requires_grad_(True)

        def ref_side(reg_max_k):
            def f():
                ops.REF_GRAD_REG_MAX_K = reg_max_k      # (read when the backward runs: set for the whole timed region below)
                return ops.consistency_sums(pred, ref_g, mask, coef)[0]
            return f
        paths = {"ref_grad": (ref_side(4), ref_g)}
        if K <= 4:
            paths["ref_grad_run_time_form"] = (ref_side(0), ref_g)
        paths["pred_grad"] = (lambda: ops.consistency_sums(pred_g, ref, mask, coef)[0], pred_g)
        if not args.hip_only:
            paths["aten_ref_grad"] = (lambda: aten_loss(pred, ref_g, mask, coef), ref_g)
        times = {k: [] for k in paths}
        try:
            for _ in range(args.rounds):                   # alternate the paths
                for k, (fn, x) in paths.items():
                    times[k].append(time_backward(fn, x, args.iters, args.warmup))
        finally:
            ops.REF_GRAD_REG_MAX_K = 4
        row = dict(shape=list(shape), terms=MIX)
        for k in paths:
            row[k + "_us"] = 1e3 * min(times[k])
        nb = algorithmic_bytes(shape)
        row["ref_grad_bytes"] = nb
        row["ref_grad_share_of_8tbps"] = nb / (row["ref_grad_us"] * 1e-6) / PEAK_BPS
        row["ref_over_pred"] = row["ref_grad_us"] / row["pred_grad_us"]
        if "ref_grad_run_time_form_us" in row:
            row["run_time_over_register"] = row["ref_grad_run_time_form_us"] / row["ref_grad_us"]
        if "aten_ref_grad_us" in row:
            row["aten_over_ref"] = row["aten_ref_grad_us"] / row["ref_grad_us"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del pred, ref, mask, pred_g, ref_g
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "ref_grad_bench%s.json" % ("_hip_only" if args.hip_only else "")), "w") as f:
            json.dump(rows, f, indent=1)


def summarize(stats_csv, out, spec):
    """Per-kernel mean time of a --hip-only run of ONE shape under rocprofv3 --stats: the reference-side kernel(s) with their
    algorithmic bandwidth, and the prediction-side backward kernel of the same call."""
    import csv
    cases = selected(spec)
    assert len(cases) == 1, "--summarize takes the one shape the profiled run timed (--cases I)"
    shape = cases[0]
    nb = algorithmic_bytes(shape)
    lines = []
    for r in csv.DictReader(open(stats_csv)):
        name = r["Name"]
        us = float(r["AverageNs"]) / 1e3
        if "k_loss_ref_grad" in name:
            lines.append(dict(shape="x".join(map(str, shape)), kernel=name[:90], calls=int(r["Calls"]), avg_us=us, bytes=nb,
                              tbps=nb / (us * 1e-6) / 1e12, share_of_8tbps=nb / (us * 1e-6) / PEAK_BPS))
        elif any(p in name for p in PRED_SIDE):
            lines.append(dict(shape="x".join(map(str, shape)), kernel=name[:90], calls=int(r["Calls"]), avg_us=us))
    for row in lines:
        print(json.dumps(row))
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "kernel_times_%s.json" % "x".join(map(str, shape))), "w") as f:
            json.dump(lines, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default=None, help="comma-separated indices into SHAPES (default: all)")
    ap.add_argument("--summarize", metavar="STATS_CSV", default=None)
    args = ap.parse_args()
    if args.summarize:
        summarize(args.summarize, args.out, args.cases)
    else:
        run(args)


if __name__ == "__main__":
    main()
