"""The 2D image-warp backward of a cfg-2 step in its three forms, in one process, with device events (modelled on
tools/det_complete_bench.py):

  float-atomic   the default mode: k_scatter_window2d flushes its LDS windows with float atomics into a zero-filled grad_in;
  int64 twin     deterministic mode, ops.WINDOW_STAGED = False: clear of the int64 image, k_det_absmax, 64-bit integer atomics,
                 k_det_convert;
  staged         deterministic mode, ops.WINDOW_STAGED = True: the stage instantiation of k_scatter_window2d + k_window_merge2d.

solver   the arguments are those of the LAST window-scatter backward of each channel count in a cfg-2 solver call (32 x 1 x 256
         x 256, full chain, five ascent steps: the morph field the call ends with, its grad_out and its input) -- C = 1 (the
         image) and C = 4 (the warped-back prediction);
rough    one launch on a uniformly random grid at 32 x 4 x 256 x 256, twin and staged: every window is capped and the merge
         kernel walks every tile's samples for every rectangle (no acceptance threshold: written down).

The forms alternate over --rounds; the best round of each is reported (median of --iters), with every round, so the spread
between rounds is there to compare a difference with.  One JSON line per case; --out DIR keeps them.

    timeout -k 10 600 python tools/window_staged_bench.py [--iters 50] [--warmup 10] [--rounds 3] [--only solver,rough] [--out DIR]

Needs a GPU (no fall-back)."""
import argparse
import contextlib
import io
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.det_wide_bench import time_step      # noqa: E402

FORMS = ("float_atomic", "int64_twin", "staged")
WANT_ROUTE = {"float_atomic": "window_float", "int64_twin": "window_int64", "staged": "window_staged"}


@contextlib.contextmanager
def form(ops, name):
    was = ops.WINDOW_STAGED
    ops.set_deterministic(name != "float_atomic")
    ops.WINDOW_STAGED = name == "staged"
    try:
        yield
    finally:
        ops.WINDOW_STAGED = was
        ops.set_deterministic(False)


def solver_calls(ops):
    """the arguments of the last window-scatter backward per channel count of one cfg-2 solver call (cloned)"""
    import bench
    wl = bench.WORKLOADS["cfg2"]
    dev = torch.device("cuda")
    solver = bench.build_solver(wl, dev, None, hip_graph=False)
    solver.deterministic = True
    torch.manual_seed(0)
    data = torch.rand(wl["batch"], 1, *wl["dims"], device=dev)
    model = bench.make_model(2).to(dev)
    seen = {}
    real = ops.raw_grid_sample_bwd

    def noting(gout, inp, grid, *rest, **kw):
        out = real(gout, inp, grid, *rest, **kw)
        if ops.last_bwd_route().startswith("window"):
            seen[inp.shape[1]] = (gout.detach().clone(), inp.detach().clone(), grid.detach().clone()) + tuple(rest)
        return out
    ops.raw_grid_sample_bwd = noting
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            solver.adversarial_training(data=data, model=model, **bench.solver_kwargs(wl, dev))
        torch.cuda.synchronize()
    finally:
        ops.raw_grid_sample_bwd = real
        ops.set_deterministic(False)
    return seen


def ab(ops, call_args, names, args):
    times = {n: [] for n in names}
    outs = {}
    for _ in range(args.rounds):
        for n in names:
            with form(ops, n):
                fn = lambda: ops.raw_grid_sample_bwd(*call_args)      # noqa: E731
                times[n].append(time_step(fn, args.iters, args.warmup))
                outs[n] = fn()
                assert ops.last_bwd_route() == WANT_ROUTE[n], (n, ops.last_bwd_route())
    return times, outs


def row_of(case, shape, times, outs):
    row = dict(case=case, shape=list(shape))
    for n, t in times.items():
        row[n + "_us"] = round(1e3 * min(t), 2)
        row[n + "_us_rounds"] = [round(1e3 * x, 2) for x in t]
    if "int64_twin" in times and "staged" in times:
        tw = times["int64_twin"]
        row["twin_spread_us"] = round(1e3 * (max(tw) - min(tw)), 2)
        row["twin_minus_staged_us"] = round(row["int64_twin_us"] - row["staged_us"], 2)
        row["staged_below_twin_by_more_than_its_spread"] = bool(row["twin_minus_staged_us"] > row["twin_spread_us"])
        row["equal_bits_staged_twin"] = bool(all(
            (a is None and b is None) or torch.equal(a.view(torch.int32), b.view(torch.int32))
            for a, b in zip(outs["staged"], outs["int64_twin"])))
    if "float_atomic" in times:
        row["staged_over_float_atomic"] = round(row["staged_us"] / row["float_atomic_us"], 4)
    return row


def run(args):
    if not torch.cuda.is_available():
        raise SystemExit("window_staged_bench needs a GPU")
    from advchain_amd import ops
    only = set(args.only.split(",")) if args.only else {"solver", "rough"}
    rows = []
    if "solver" in only:
        seen = solver_calls(ops)
        for C in sorted(seen):
            call = seen[C]
            times, outs = ab(ops, call, FORMS, args)
            row = row_of("cfg-2 image-warp backward, the field the call ends with, C = %d" % C, call[1].shape, times, outs)
            row["args"] = dict(interp=call[3], padding=call[4], clamp_grid=bool(call[5]), need_gin=bool(call[6]),
                               need_ggrid=bool(call[7]), halo=call[8] if len(call) > 8 else 0)
            row["max_displacement_px"] = round(float(ops.raw_max_displacement(call[2]).item()), 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del seen
        torch.cuda.empty_cache()
    if "rough" in only:
        g = torch.Generator(device="cuda").manual_seed(0)
        shape = (32, 4, 256, 256)
        grid = (torch.rand((shape[0], 2) + shape[2:], device="cuda", generator=g) * 2 - 1).contiguous()
        inp = torch.randn(shape, device="cuda", generator=g)
        gout = torch.randn(shape, device="cuda", generator=g)
        rough = argparse.Namespace(iters=max(3, args.iters // 10), warmup=2, rounds=args.rounds)
        times, outs = ab(ops, (gout, inp, grid, 0, 0, False, True, True, 16), ("int64_twin", "staged"), rough)
        row = row_of("uniformly random grid: every window capped", shape, times, outs)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "window_staged_bench.json"), "w") as f:
            json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None, help="comma-separated subset of solver,rough")
    ap.add_argument("--out", default=None)
    run(ap.parse_args())


if __name__ == "__main__":
    main()
