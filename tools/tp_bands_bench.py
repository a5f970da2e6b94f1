"""The row-blended kernels with their band tables by dword loads and by 16-byte requests (ops.set_tp_wide_loads), per rows per
workgroup, in one process, with device events (the timing pattern of tools/bias_rows_bench.py):

  upsample   advchain_tp_interp_fwd_smoothed_pair_rows (k_tp_interp_fwd_gs: smoothing + upsampling + identity of a paired 2D field)
             at rows_per_wg = 32 (what the entry without the argument takes), 16, 8 -- cfg-2 only (the fused form is 2D);
  forward    advchain_bias_field_fwd_rows (data * field and the field) at 32, 16, 8, 4;
  reduced    advchain_bias_field_bwd_reduced (to t1, with grad_data) at 32, 16, 8, 4;

at bench.py's cfg-2 (32 x 1 x 256 x 256) and cfg-3 (4 x 1 x 128 x 128 x 64) geometry.  Every (entry, rows, form) is timed once per
round, the forms alternating; each round's median of --iters is kept.  Outputs are preallocated: kernels only.  The two forms'
outputs are compared bit for bit.  One JSON line per case; --out DIR keeps them.

    timeout -k 10 300 python tools/tp_bands_bench.py [--iters 50] [--warmup 10] [--rounds 3] [--out DIR]

Needs a GPU (no fall-back)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bias_rows_bench import geometry      # noqa: E402
from tools.det_wide_bench import time_step      # noqa: E402

BIAS_ROWS = (32, 16, 8, 4)
UP_ROWS = (32, 16, 8)


def morph_geometry(workload):
    import bench
    from advchain_amd import bands
    wl = bench.WORKLOADS[workload]
    cfg = dict(bench.transform_configs(wl["dims"], wl["batch"], ["morph"]))["morph"]
    vs = list(cfg["vector_size"])
    return bands.upsample_tables(vs, list(wl["dims"]), torch.device("cuda")), (wl["batch"], len(vs)) + tuple(vs), tuple(wl["dims"])


def run(args):
    if not torch.cuda.is_available():
        raise SystemExit("tp_bands_bench needs a GPU")
    from advchain_amd import _lib, ops
    lib = _lib.load()
    rows_out = []
    for workload in ("cfg2", "cfg3"):
        tables, cp, shape = geometry(workload)
        N, C = shape[:2]
        g = torch.Generator(device="cuda").manual_seed(0)
        data = torch.rand(shape, device="cuda", generator=g) + 0.5
        gout = torch.randn(shape, device="cuda", generator=g)
        out, field, gdata = (torch.empty(shape, device="cuda") for _ in range(3))
        t1 = torch.empty((N, 1) + tuple(shape[2:-1]) + (int(tables.g[2]),), device="cuda")
        wd, lo, WB = tables.dense_inner
        tab = (ops._ptr(tables.itab), ops._ptr(tables.ftab), _lib.dims_array(tables.S), _lib.dims_array(tables.g),
               _lib.dims_array(tables.B))
        eps, st = 0.3, ops._stream()

        def fwd(rows):
            _lib.check(lib.advchain_bias_field_fwd_rows(ops._ptr(cp), ops._ptr(data), ops._ptr(out), ops._ptr(field), *tab, N, C,
                                                        eps, 1, 1.0, rows, st), "fwd")
            return out, field

        def red(rows):
            _lib.check(lib.advchain_bias_field_bwd_reduced(ops._ptr(cp), ops._ptr(data), ops._ptr(gout), ops._ptr(t1),
                                                           ops._ptr(gdata), *tab, N, C, eps, 1, 1.0, ops._ptr(wd), ops._ptr(lo), WB,
                                                           rows, st), "reduced")
            return t1, gdata
        entries = {}
        for r in BIAS_ROWS:
            entries["forward_%d" % r] = (fwd, r)
        for r in BIAS_ROWS:
            entries["reduced_%d" % r] = (red, r)
        row = dict(case=workload, shape=list(shape), g=list(tables.g), B=list(tables.B),
                   bias_rule=int(lib.advchain_bias_rows_per_wg(_lib.dims_array(tables.S), N)))
        if len(shape) == 4:
            mt, vshape, dims = morph_geometry(workload)
            vel = torch.randn(vshape, device="cuda", generator=g)
            P = vshape[0] * vshape[1]
            s1 = torch.empty((2 * vshape[0],) + vshape[1:], device="cuda")
            phi = torch.empty((2 * vshape[0], vshape[1]) + dims, device="cuda")
            disp = torch.zeros(ops.DISP_SLOTS, device="cuda")
            mtab = (ops._ptr(mt.itab), ops._ptr(mt.ftab), _lib.dims_array(mt.S), _lib.dims_array(mt.g), _lib.dims_array(mt.B))

            def up(rows):
                rc = lib.advchain_tp_interp_fwd_smoothed_pair_rows(ops._ptr(vel), ops._ptr(s1), ops._ptr(phi), *mtab, P, vshape[1], 1,
                                                                   1.0 / 256, ops._ptr(disp), ops._GAUSS9, 1.5, rows, st)
                assert rc == 0, rc
                return s1, phi
            for r in UP_ROWS:
                entries["upsample_%d" % r] = (up, r)
            row.update(morph_g=list(mt.g), morph_B=list(mt.B), planes=2 * P)
        forms = [(n, w) for n in entries for w in (False, True)]
        times = {f: [] for f in forms}
        was = ops.tp_wide_loads()
        try:
            for _ in range(args.rounds):
                for n, w in forms:
                    fn, r = entries[n]
                    ops.set_tp_wide_loads(w)
                    times[(n, w)].append(time_step(lambda: fn(r), args.iters, args.warmup))
            equal = {}
            for n, (fn, r) in entries.items():
                ops.set_tp_wide_loads(False)
                a = [t.clone() for t in fn(r)]
                ops.set_tp_wide_loads(True)
                b = fn(r)
                torch.cuda.synchronize()
                equal[n] = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
        finally:
            ops.set_tp_wide_loads(was)
        row["equal_bits"] = all(equal.values())
        for (n, w), t in times.items():
            key = "%s_%s" % (n, "wide" if w else "dword")
            t = [round(1e3 * x, 2) for x in t]
            row[key + "_us"] = sorted(t)[len(t) // 2]
            row[key + "_us_rounds"] = t
        rows_out.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "tp_bands_bench.json"), "w") as f:
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
