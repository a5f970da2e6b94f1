"""The x+y Gaussian launch per form and tile, in one process, with device events (the timing pattern of tools/bias_rows_bench.py):

  staged          advchain_gauss_xy_staged (k_gauss_xy: x pass LDS -> LDS, two barriers);
  lanes_<ty>_<nt> advchain_gauss_xy_lanes (k_gauss_xy_lanes: x taps from the neighbouring lanes) with ty rows and nt threads a
                  workgroup, for each of the five tiles the library is built for;

at the shapes of the solver step:

  cfg2_fwd   128 planes of 256 x 256 (the paired field [v; -v] of 32 x 2), pre 2 / post 1;
  cfg2_adj   the same planes, pre 0 / post 2, the input in two halves, aux = the positions;
  cfg3_fwd   24 planes of 128 x 128 x 64 (the paired field of 4 x 3), pre 2 (the z pass that follows is not timed).

The forms alternate over --rounds; every round's median of --iters is kept.  Outputs are preallocated: kernels only.  A form is
adopted for a shape only if its median lies below the staged kernel's by more than three times the spread between the staged
kernel's own rounds (`beats_staged`).  Every form's output is compared with the staged kernel's bit for bit (`equal_bits`).
One JSON line per case; --out DIR keeps them.  The rule of advchain_gauss_xy_plan was set from this table
(profiles/r20/gauss_lanes).

    timeout -k 10 300 python tools/gauss_xy_bench.py [--iters 50] [--warmup 10] [--rounds 3] [--out DIR]

Needs a GPU (no fall-back)."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.det_wide_bench import time_step      # noqa: E402

TILES = ((16, 256), (16, 512), (32, 256), (32, 512), (64, 1024))
CASES = (      # name, planes, C, dims, pre, post, split
    ("cfg2_fwd", 128, 2, (256, 256), 2, 1, False),
    ("cfg2_adj", 128, 2, (256, 256), 0, 2, True),
    ("cfg3_fwd", 24, 3, (128, 128, 64), 2, 0, False),
)


def positions(planes, C, dims, gen):
    """identity + a smooth displacement of a few voxels, planar: what the solver smooths"""
    axes = [torch.linspace(-1, 1, s, device="cuda") for s in dims]
    mesh = torch.meshgrid(*axes, indexing="ij")
    ident = torch.stack(list(reversed(mesh)))                                      # channel 0 = x (fastest axis)
    pos = ident.repeat(planes // C, *([1] * len(dims))).reshape((planes,) + tuple(dims))
    return (pos + 0.02 * torch.randn(pos.shape, device="cuda", generator=gen)).contiguous()


def run(args):
    if not torch.cuda.is_available():
        raise SystemExit("gauss_xy_bench needs a GPU")
    from advchain_amd import _lib, ops
    lib = _lib.load()
    w9 = ops._GAUSS9
    rows_out = []
    for name, planes, C, dims, pre, post, split in CASES:
        g = torch.Generator(device="cuda").manual_seed(0)
        pos = positions(planes, C, dims, g)
        x = pos if pre == 2 else torch.randn(pos.shape, device="cuda", generator=g)
        lo, hi = (x[:planes // 2].clone(), x[planes // 2:].clone()) if split else (x, None)
        aux = pos if post == 2 else None
        nd, da, st = len(dims), _lib.dims_array(dims), ops._stream()
        outs = {}

        def call(form, ty=0, nt=0):
            out = outs.setdefault((form, ty, nt), torch.empty_like(pos))
            a = (ops._ptr(lo), ops._ptr(out), ops._ptr(aux), planes, C, nd, da, w9, pre, post, 1.0, st, ops._ptr(hi),
                 planes // 2 if split else planes)
            if form == "staged":
                _lib.check(lib.advchain_gauss_xy_staged(*a), "gauss_xy_staged")
            else:
                _lib.check(lib.advchain_gauss_xy_lanes(*a, ty, nt), "gauss_xy_lanes")

        forms = {"staged": ("staged", 0, 0)}
        for ty, nt in TILES:
            forms["lanes_%d_%d" % (ty, nt)] = ("lanes", ty, nt)
        times = {n: [] for n in forms}
        for _ in range(args.rounds):
            for n, f in forms.items():
                times[n].append(1e3 * time_step(lambda: call(*f), args.iters, args.warmup))
        torch.cuda.synchronize()
        ref = outs[("staged", 0, 0)].view(torch.int32)
        form, ty, nt = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(lib.advchain_gauss_xy_plan(nd, da, planes, ctypes.byref(form), ctypes.byref(ty), ctypes.byref(nt)), "plan")
        med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
        spread = max(times["staged"]) - min(times["staged"])
        nbytes = 8 * pos.numel() + (4 * pos.numel() if post == 2 else 0)
        row = dict(case=name, planes=planes, dims=list(dims), pre=pre, post=post, split=split, bytes=nbytes,
                   plan=dict(form=form.value, ty=ty.value, nt=nt.value), staged_spread_us=round(spread, 2))
        for n, t in times.items():
            row[n] = dict(us=round(med[n], 2), us_rounds=[round(v, 2) for v in t], tb_s=round(nbytes / med[n] / 1e6, 2),
                          equal_bits=bool(torch.equal(outs[forms[n]].view(torch.int32), ref)),
                          beats_staged=bool(n != "staged" and med["staged"] - med[n] > 3 * spread))
        rows_out.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "gauss_xy_bench.json"), "w") as f:
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
