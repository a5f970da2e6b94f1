"""The bias forward and backward per rows-per-workgroup value, in one process, with device events (the timing pattern of
tools/window_staged_bench.py):

  forward    advchain_bias_field_fwd_rows (data * field and the field) at rows_per_wg = 32 (the grid of every launch before the
             argument existed), 16, 8, 4;
  backward   to t1, the result of the adjoint's innermost pass, with grad_data:
             two_launches_<rows>   advchain_bias_field_bwd_rows + advchain_band_reduce_rows_dense over grad_L,
             reduced_<rows>        advchain_bias_field_bwd_reduced (one launch, no grad_L);

at bench.py's cfg-2 (32 x 1 x 256 x 256) and cfg-3 (4 x 1 x 128 x 128 x 64) bias geometry.  The forms alternate over --rounds; the
best round of each is reported (median of --iters), with every round.  Outputs are preallocated: kernels only.  One JSON line
per case; --out DIR keeps them.  The rule of advchain_bias_rows_per_wg was set from this table (profiles/r16/bias_rows).

    timeout -k 10 300 python tools/bias_rows_bench.py [--iters 50] [--warmup 10] [--rounds 3] [--out DIR]

Needs a GPU (no fall-back)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.det_wide_bench import time_step      # noqa: E402

ROWS = (32, 16, 8, 4)


def geometry(workload):
    import bench
    from advchain_amd.augmentor import AdvBias
    wl = bench.WORKLOADS[workload]
    cfg = dict(bench.transform_configs(wl["dims"], wl["batch"], ["bias"]))["bias"]
    t = AdvBias(len(wl["dims"]), cfg, device=torch.device("cuda"))
    t.init_parameters()
    return t._tables, t.param.detach().clone(), tuple(cfg["data_size"])


def run(args):
    if not torch.cuda.is_available():
        raise SystemExit("bias_rows_bench needs a GPU")
    from advchain_amd import _lib, ops
    lib = _lib.load()
    rows_out = []
    for workload in ("cfg2", "cfg3"):
        tables, cp, shape = geometry(workload)
        N, C = shape[:2]
        g = torch.Generator(device="cuda").manual_seed(0)
        data = torch.rand(shape, device="cuda", generator=g) + 0.5
        gout = torch.randn(shape, device="cuda", generator=g)
        out, field, gL, gdata = (torch.empty(shape, device="cuda") for _ in range(4))
        t1 = torch.empty((N, 1) + tuple(shape[2:-1]) + (int(tables.g[2]),), device="cuda")
        t1b = torch.empty_like(t1)
        wd, lo, WB = tables.dense_inner
        tab = (ops._ptr(tables.itab), ops._ptr(tables.ftab), _lib.dims_array(tables.S), _lib.dims_array(tables.g),
               _lib.dims_array(tables.B))
        eps, st = 0.3, ops._stream()

        def fwd(rows):
            _lib.check(lib.advchain_bias_field_fwd_rows(ops._ptr(cp), ops._ptr(data), ops._ptr(out), ops._ptr(field), *tab, N, C,
                                                        eps, 1, 1.0, rows, st), "fwd")

        def two(rows):
            _lib.check(lib.advchain_bias_field_bwd_rows(ops._ptr(cp), ops._ptr(data), ops._ptr(gout), ops._ptr(gL), ops._ptr(gdata),
                                                        *tab, N, C, eps, 1, 1.0, rows, st), "bwd")
            _lib.check(lib.advchain_band_reduce_rows_dense(ops._ptr(gL), None, ops._ptr(t1), ops._ptr(wd), ops._ptr(lo),
                                                           t1.numel() // t1.shape[-1], tables.S[2], tables.g[2], WB, 1.0, st), "rows")

        def red(rows):
            _lib.check(lib.advchain_bias_field_bwd_reduced(ops._ptr(cp), ops._ptr(data), ops._ptr(gout), ops._ptr(t1b),
                                                           ops._ptr(gdata), *tab, N, C, eps, 1, 1.0, ops._ptr(wd), ops._ptr(lo), WB,
                                                           rows, st), "reduced")
        forms = {}
        for r in ROWS:
            forms["forward_%d" % r] = (fwd, r)
        for r in ROWS:
            forms["two_launches_%d" % r] = (two, r)
        for r in ROWS:
            forms["reduced_%d" % r] = (red, r)
        times = {n: [] for n in forms}
        for _ in range(args.rounds):
            for n, (fn, r) in forms.items():
                times[n].append(time_step(lambda: fn(r), args.iters, args.warmup))
        two(32)
        red(0)
        torch.cuda.synchronize()
        row = dict(case=workload, shape=list(shape), g=list(tables.g), WB=WB,
                   rule=int(lib.advchain_bias_rows_per_wg(_lib.dims_array(tables.S), N)),
                   equal_bits_reduced_two_launches=bool(torch.equal(t1.view(torch.int32), t1b.view(torch.int32))))
        for n, t in times.items():
            row[n + "_us"] = round(1e3 * min(t), 2)
            row[n + "_us_rounds"] = [round(1e3 * x, 2) for x in t]
        rows_out.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bias_rows_bench.json"), "w") as f:
            json.dump(rows_out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    run(ap.parse_args())


if __name__ == "__main__":
    main()
