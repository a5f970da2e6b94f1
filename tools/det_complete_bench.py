"""Cost of what completes the deterministic mode, against the default mode on the same inputs in the same process, with device
events (modelled on tools/det_wide_bench.py):

  loss     the consistency-loss FORWARD ('mse' + 'contour' + 'kl', no gradient) at 32 x 4 x 256 x 256 (the fused kernel) and
           32 x 20 x 256 x 256 (the run-time-K kernels): 64 slots + finisher against one partial per workgroup + ordered finisher;
  bicubic  forward + backward (both gradients) of ops.grid_sample(..., 'bicubic') at 8 x 4 x 256 x 256 through a smooth field of
           a few pixels: float atomics against the int64 fixed-point twin;
  norm     ops.field_sumsq for a 4 x 3 x 128 x 128 x 64 field from 8 x 8 x 32 coefficients (bench.py's cfg-5 convention: // 16,
           // 16, // 2): 64 slots against the ordered reduction.

The modes alternate over --rounds; the best round of each is reported (median of --iters), with every round, so the spread
between rounds is there to compare a difference with.  One JSON line per case; --out DIR keeps them.

    timeout -k 10 600 python tools/det_complete_bench.py [--iters 50] [--warmup 10] [--rounds 3] [--only loss,bicubic,norm] [--out DIR]

Needs a GPU (no fall-back)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.det_wide_bench import smooth_grid, time_step      # noqa: E402

LOSS_SHAPES = [(32, 4, 256, 256), (32, 20, 256, 256)]
BICUBIC_SHAPE = (8, 4, 256, 256)
NORM_SHAPE = (4, 3, 128, 128, 64)


def ab(fn, args, ops):
    """times[mode] = median ms per round, the modes alternating; result[mode] = what fn returned last in that mode"""
    times = {"default": [], "deterministic": []}
    result = {}
    try:
        for _ in range(args.rounds):
            for mode in times:
                ops.set_deterministic(mode == "deterministic")
                times[mode].append(time_step(fn, args.iters, args.warmup))
                result[mode] = fn()
    finally:
        ops.set_deterministic(False)
    return times, result


def row_of(what, shape, times):
    row = dict(case=what, shape=list(shape))
    for mode, t in times.items():
        row[mode + "_us"] = round(1e3 * min(t), 2)
        row[mode + "_us_rounds"] = [round(1e3 * x, 2) for x in t]
    row["deterministic_over_default"] = round(row["deterministic_us"] / row["default_us"], 4)
    return row


def run(args):
    if not torch.cuda.is_available():
        raise SystemExit("det_complete_bench needs a GPU")
    from advchain_amd import bands, ops
    from advchain_amd.common.loss import calc_segmentation_consistency
    only = set(args.only.split(",")) if args.only else {"loss", "bicubic", "norm"}
    rows = []
    g = torch.Generator(device="cuda").manual_seed(0)
    if "loss" in only:
        for shape in LOSS_SHAPES:
            pred = torch.randn(shape, device="cuda", generator=g) * 3
            ref = torch.randn(shape, device="cuda", generator=g) * 3

            def loss():
                with torch.no_grad():
                    return calc_segmentation_consistency(pred, ref, ["mse", "contour", "kl"], [0.7, 0.5, 1.3], scales=[0])
            times, res = ab(loss, args, ops)
            row = row_of("loss forward (mse + contour + kl)", shape, times)
            row["value_default"], row["value_deterministic"] = float(res["default"]), float(res["deterministic"])
            rows.append(row)
            print(json.dumps(row), flush=True)
            del pred, ref
            torch.cuda.empty_cache()
    if "bicubic" in only:
        shape = BICUBIC_SHAPE
        inp = torch.randn(shape, device="cuda", generator=g).requires_grad_(True)
        wv = torch.randn(shape, device="cuda", generator=g)
        grid = smooth_grid(shape[0], tuple(shape[2:]), 3.0, g).requires_grad_(True)

        def warp():
            return torch.autograd.grad((ops.grid_sample(inp, grid, "bicubic", "zeros") * wv).sum(), (inp, grid))
        times, res = ab(warp, args, ops)
        row = row_of("bicubic warp forward + backward, both gradients", shape, times)
        row["max_abs_diff_grad_in"] = float((res["default"][0] - res["deterministic"][0]).abs().max())
        row["max_abs_grad_in"] = float(res["default"][0].abs().max())
        row["grad_grid_equal_bits"] = bool(torch.equal(res["default"][1], res["deterministic"][1]))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del inp, wv, grid
        torch.cuda.empty_cache()
    if "norm" in only:
        shape = NORM_SHAPE
        full = list(shape[2:])
        low = [full[0] // 16, full[1] // 16, full[2] // 2]
        tables = bands.upsample_tables(low, full, torch.device("cuda"))
        coef = torch.randn((shape[0], shape[1]) + tuple(low), device="cuda", generator=g)

        def norm():
            return ops.field_sumsq(coef, tables, 3)
        times, res = ab(norm, args, ops)
        row = row_of("3D step-count norm (field not materialised)", shape, times)
        row["value_default"], row["value_deterministic"] = float(res["default"]), float(res["deterministic"])
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "det_complete_bench.json"), "w") as f:
            json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None, help="comma-separated subset of loss,bicubic,norm")
    ap.add_argument("--out", default=None)
    run(ap.parse_args())


if __name__ == "__main__":
    main()
