"""Times the consistency loss for a run-time class count (csrc/loss_lp.hip, through ops.consistency_sums), forward and
backward separately with device events, against (a) an ATen expression of the same loss written out below (the outside
yardstick) and (b), for K <= 16, the register / three-kernel path of csrc/loss.hip on the same tensors in the same process
(ops.WIDE_LOSS_MIN_K = 17 against = 2, alternating).  One JSON line per case; --out DIR keeps them.

    python tools/wide_loss_bench.py [--iters 20] [--warmup 5] [--rounds 3] [--cases 0,3] [--no-ref] [--out DIR]
    python tools/wide_loss_bench.py --summarize STATS_CSV --cases 3 [--out DIR]

--no-ref --cases I is the run for `rocprofv3 --kernel-trace --stats` (program after `--`): ONE case, so that each kernel's
time belongs to one shape; --summarize turns its stats file into bandwidth.  Needs a GPU (no fall-back).

Algorithmic bytes per voxel and sample, from the shapes (fp32, one-channel mask, S = 16: the softmax statistics, 4 floats):
  fwd: pred 4K + ref 4K + mask 4 + statistics S + R 8(K-1)        bwd: pred 4K + ref 4K + mask 4 + statistics S + R 8(K-1) + grad 4K
(without 'contour' R drops out).  What the kernels move beyond that -- the second sweep over the logits in the statistics
pass and in the backward, the halo of the tiles -- is their own overhead and shows as a lower share of the peak."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BPS = 8.0e12          # MI355X HBM3E

MIXES = {"mse+contour": (1.0, 0.5, 0.0), "mse+kl+contour": (0.7, 0.5, 1.3)}      # weights of mse, contour, kl
SHAPES = [(32, 16, 256, 256), (32, 20, 256, 256), (32, 32, 256, 256), (4, 16, 128, 128, 64), (4, 20, 128, 128, 64),
          (2, 20, 160, 160, 80), (32, 8, 256, 256), (4, 8, 128, 128, 64)]
CASES = [(s, m) for s in SHAPES for m in ("mse+contour", "mse+kl+contour")]


def selected(spec):
    return CASES if not spec else [CASES[int(i)] for i in spec.split(",")]


def algorithmic_bytes(shape, direction, contour=True):
    N, K = shape[:2]
    pts = N
    for s in shape[2:]:
        pts *= s
    per = 8 * K + 4 + 16 + (8 * (K - 1) if contour else 0)
    if direction == "bwd":
        per += 4 * K
    return pts * per


def coefficients(shape, mix):
    """The normalisers of calc_segmentation_consistency for a one-channel mask (common/loss.py)."""
    N, K = shape[:2]
    V = 1
    for s in shape[2:]:
        V *= s
    w_mse, w_cnt, w_kl = MIXES[mix]
    c_mse = w_mse / (float(N) * K * V * (float(N) * 1 * V / K))
    if len(shape) == 4:
        c_a = c_b = w_cnt * 0.5 / (float(N) * V * (K - 1))
    else:
        c_a = w_cnt * (2.0 / 3.0) / (float(N) * V * (K - 1))
        c_b = w_cnt * (1.0 / 3.0) / (float(N) * V * (K - 1))
    return [c_mse, c_a, c_b, w_kl / (float(N) * V)]


def aten_loss(pred, ref, mask, coef):
    """The same four sums in ATen: softmax over the classes, masked squared error, the 3^d stencils on P - T of the object
    classes (one convolution per stencil over all classes as a batch), KL from the two log-softmaxes."""
    nd = pred.dim() - 2
    K = pred.shape[1]
    P, T = torch.softmax(pred, 1), torch.softmax(ref, 1)
    total = coef[0] * ((P * mask - T * mask) ** 2).sum()
    h = torch.tensor([1.0, 2.0, 1.0], device=pred.device)
    hp = torch.tensor([1.0, 0.0, -1.0], device=pred.device)
    if nd == 2:
        ka, kb = (h[:, None] * hp[None, :])[None, None], (hp[:, None] * h[None, :])[None, None]
        conv = F.conv2d
    else:
        ka = (h[:, None, None] * hp[None, :, None] * h[None, None, :])[None, None]
        kb = (h[:, None, None] * h[None, :, None] * hp[None, None, :])[None, None]
        conv = F.conv3d
    D = (P - T)[:, 1:].reshape((-1, 1) + tuple(pred.shape[2:]))
    m = mask.expand(-1, K - 1, *mask.shape[2:]).reshape(D.shape)
    total = total + coef[1] * ((conv(D, ka, padding=1) * m) ** 2).sum() + coef[2] * ((conv(D, kb, padding=1) * m) ** 2).sum()
    if coef[3] != 0.0:
        total = total + coef[3] * (mask * (T * (F.log_softmax(ref, 1) - F.log_softmax(pred, 1)))).sum()
    return total


def time_pair(fwd, x, iters, warmup):
    """(forward ms, backward ms): device events around each of the two, `iters` evaluations."""
    for _ in range(warmup):
        torch.autograd.grad(fwd(), x)
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(iters)]
    for a, b, c in ev:
        a.record()
        v = fwd()
        b.record()
        torch.autograd.grad(v, x)
        c.record()
    torch.cuda.synchronize()
    f = sorted(a.elapsed_time(b) for a, b, c in ev)
    g = sorted(b.elapsed_time(c) for a, b, c in ev)
    return f[len(f) // 2], g[len(g) // 2]


def run(args):
    if not torch.cuda.is_available():
        raise SystemExit("wide_loss_bench needs a GPU")
    from advchain_amd import ops
    rows = []
    for shape, mix in selected(args.cases):
        g = torch.Generator(device="cuda").manual_seed(0)
        pred = (torch.randn(shape, device="cuda", generator=g) * 2).requires_grad_(True)
        ref = torch.randn(shape, device="cuda", generator=g) * 2
        mask = (torch.rand((shape[0], 1) + tuple(shape[2:]), device="cuda", generator=g) > 0.1).float()
        coef = coefficients(shape, mix)
        K = shape[1]

        def ours(min_k):
            def f():
                ops.WIDE_LOSS_MIN_K = min_k
                try:
                    return ops.consistency_sums(pred, ref, mask, coef)[0]
                finally:
                    ops.WIDE_LOSS_MIN_K = 17
            return f
        paths = {"wide": ours(2)}
        if K <= 16:
            paths["register"] = ours(17)
        if not args.no_ref:
            paths["aten"] = lambda: aten_loss(pred, ref, mask, coef)
        times = {k: [] for k in paths}
        for _ in range(args.rounds):                   # alternate the paths
            for k, fn in paths.items():
                times[k].append(time_pair(fn, pred, args.iters, args.warmup))
        row = dict(shape=list(shape), terms=mix)
        for k in paths:
            row[k + "_fwd_us"] = 1e3 * min(t[0] for t in times[k])
            row[k + "_bwd_us"] = 1e3 * min(t[1] for t in times[k])
        for d in ("fwd", "bwd"):
            nb = algorithmic_bytes(shape, d)
            row[d + "_bytes"] = nb
            row["wide_%s_share_of_8tbps" % d] = nb / (row["wide_%s_us" % d] * 1e-6) / PEAK_BPS
        row["wide_us_per_class"] = (row["wide_fwd_us"] + row["wide_bwd_us"]) / K
        rows.append(row)
        print(json.dumps(row), flush=True)
        del pred, ref, mask
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "wide_loss_bench%s.json" % ("_hip_only" if args.no_ref else "")), "w") as f:
            json.dump(rows, f, indent=1)


KERNELS = {"k_lp_stats": "fwd", "k_lp_edge": "fwd", "k_lp_bwd": "bwd", "k_consistency_finish": None}


def summarize(stats_csv, out, spec):
    """Per-kernel mean time of a --no-ref run of ONE case under rocprofv3 --stats -> per direction: kernel time, algorithmic
    bytes of the case, achieved bandwidth and share of PEAK_BPS."""
    import csv
    cases = selected(spec)
    assert len(cases) == 1, "--summarize takes the one case the profiled run timed (--cases I)"
    shape, mix = cases[0]
    lines, per_dir = [], {"fwd": 0.0, "bwd": 0.0}
    for r in csv.DictReader(open(stats_csv)):
        base = next((k for k in KERNELS if k in r["Name"]), None)
        if base is None:
            continue
        us = float(r["AverageNs"]) / 1e3
        lines.append(dict(kernel=r["Name"][:90], calls=int(r["Calls"]), avg_us=us))
        if KERNELS[base]:
            per_dir[KERNELS[base]] += us
    for d, us in per_dir.items():
        nb = algorithmic_bytes(shape, d)
        lines.append(dict(case="%s %s" % ("x".join(map(str, shape)), mix), direction=d, kernel_us=us, bytes=nb,
                          tbps=nb / (us * 1e-6) / 1e12 if us else None, share_of_8tbps=nb / (us * 1e-6) / PEAK_BPS if us else None))
    for row in lines:
        print(json.dumps(row))
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "kernel_bandwidth_%s_%s.json" % ("x".join(map(str, shape)), mix.replace("+", "_"))), "w") as f:
            json.dump(lines, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default=None, help="comma-separated indices into CASES (default: all)")
    ap.add_argument("--summarize", metavar="STATS_CSV", default=None)
    args = ap.parse_args()
    if args.summarize:
        summarize(args.summarize, args.out, args.cases)
    else:
        run(args)


if __name__ == "__main__":
    main()
