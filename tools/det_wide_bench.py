"""Times forward + backward of the warp of a K-channel tensor through ops.grid_sample and ops.affine_warp in deterministic
mode (the int64 fixed-point twins of the general kernels: advchain_grid_sample_bwd_det, advchain_affine_warp_bwd_det) against
the default mode (float atomics: the same code as before the twins existed), on the same inputs in the same process, with
device events:

  grid_sample: a smooth field of a few voxels (what AdvMorph's prediction warp sees), gradients w.r.t. the input and the grid;
  affine_warp: a rotation of 0.2 rad with mild scale, gradients w.r.t. the input and theta.

The modes alternate over --rounds; the best round of each is reported (median of --iters, each timing one forward + backward),
with the spread between rounds, and the largest difference between the two modes' gradients.  One JSON line per shape and
operator; --out DIR keeps them.

    python tools/det_wide_bench.py [--iters 20] [--warmup 5] [--rounds 3] [--cases 0,2] [--out DIR]

Every GPU step runs under a time limit of its own, set on the command line:

    timeout -k 10 300 python tools/det_wide_bench.py --out DIR

Needs a GPU (no fall-back)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(8, 20, 256, 256), (8, 6, 256, 256), (1, 20, 128, 128, 64)]


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


def smooth_grid(N, dims, amp_vox, gen):
    """identity + a smooth displacement of up to amp_vox voxels, planar (N, d, dims)"""
    d = len(dims)
    axes = [torch.linspace(-1, 1, s, device="cuda") for s in dims]
    mesh = torch.meshgrid(*axes, indexing="ij")
    ident = torch.stack(list(reversed(mesh)))[None].expand(N, d, *dims)        # channel 0 = x (fastest axis)
    low = torch.rand((N, d) + tuple(max(2, s // 16) for s in dims), device="cuda", generator=gen) * 2 - 1
    up = F.interpolate(low, size=dims, mode="trilinear" if d == 3 else "bilinear", align_corners=True)
    scale = torch.tensor([2.0 * amp_vox / (dims[d - 1 - a] - 1) for a in range(d)], device="cuda").view(1, d, *([1] * d))
    return (ident + up * scale).contiguous()


def rotation(N, d):
    th = torch.zeros(N, d, d + 1, device="cuda")
    c, s = float(torch.cos(torch.tensor(0.2))), float(torch.sin(torch.tensor(0.2)))
    for a in range(d):
        th[:, a, a] = 1.0
    th[:, 0, 0], th[:, 0, 1], th[:, 1, 0], th[:, 1, 1] = 1.05 * c, -s, s, 0.95 * c
    th[:, :, d] = 0.03
    return th


def run(args):
    if not torch.cuda.is_available():
        raise SystemExit("det_wide_bench needs a GPU")
    from advchain_amd import ops
    rows = []
    for shape in selected(args.cases):
        N, dims = shape[0], tuple(shape[2:])
        g = torch.Generator(device="cuda").manual_seed(0)
        inp = torch.randn(shape, device="cuda", generator=g).requires_grad_(True)
        wv = torch.randn(shape, device="cuda", generator=g)
        grid = smooth_grid(N, dims, 3.0, g).requires_grad_(True)
        theta = rotation(N, len(dims)).requires_grad_(True)

        def warp():
            return torch.autograd.grad((ops.grid_sample(inp, grid, "bilinear", "zeros") * wv).sum(), (inp, grid))

        def affine():
            return torch.autograd.grad((ops.affine_warp(inp, theta, "bilinear", "zeros") * wv).sum(), (inp, theta))
        for name, fn in (("grid_sample", warp), ("affine_warp", affine)):
            times = {"default": [], "deterministic": []}
            grads = {}
            try:
                for _ in range(args.rounds):                   # alternate the modes
                    for mode in times:
                        ops.set_deterministic(mode == "deterministic")
                        times[mode].append(time_step(fn, args.iters, args.warmup))
                        grads[mode] = [t.detach().clone() for t in fn()]
            finally:
                ops.set_deterministic(False)
            row = dict(shape=list(shape), op=name, what="forward + backward, both gradients")
            for mode, t in times.items():
                row[mode + "_us"] = 1e3 * min(t)
                row[mode + "_us_rounds"] = [round(1e3 * x, 1) for x in t]
            row["deterministic_over_default"] = row["deterministic_us"] / row["default_us"]
            row["max_abs_diff_grad_in"] = float((grads["default"][0] - grads["deterministic"][0]).abs().max())
            row["max_abs_grad_in"] = float(grads["default"][0].abs().max())
            row["second_gradient_equal_bits"] = bool(torch.equal(grads["default"][1], grads["deterministic"][1]))
            rows.append(row)
            print(json.dumps(row), flush=True)
        del inp, wv, grid, theta
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "det_wide_bench.json"), "w") as f:
            json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default=None, help="comma-separated indices into SHAPES (default: all)")
    run(ap.parse_args())


if __name__ == "__main__":
    main()
