"""Times the Jacobian operators -- determinant forward, determinant backward, folding statistics, image_diff3d forward +
backward -- against what a user could write before them: the fp32 torch closed form of tests/jacobian_forms.py (slicing
stencils, explicit determinant, autograd) on the same GPU and inputs.  The two paths alternate in one run, timed with device
events; prints one JSON line per case and writes them to --out.

    python tools/jacobian_bench.py [--iters 30] [--warmup 5] [--no-ref] [--cases 0,1] [--out DIR]

--no-ref times the HIP path only: the run to put under `rocprofv3 --kernel-trace --stats` (one case at a time, so that a
kernel's mean time belongs to one shape), whose csv `--summarize STATS_CSV --cases I` turns into bytes/s.  Algorithmic bytes
per voxel, d = 2 or 3 components of 4 B:
  det fwd : field 4d + det 4                    (3D: 16)         stats   : field 4d                      (3D: 12)
  det bwd : field 4d + grad_det 4 + grad 4d     (3D: 28; no workspace: the cofactors are recomputed at the neighbours)
  diff fwd: in 4 + out 4d (per element)         (3D: 16)         diff bwd: grads 4d + grad_in 4          (3D: 16)
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BPS = 8.0e12          # MI355X HBM3E

CASES = [
    ("displacement", (4, 3, 128, 128, 64)),
    ("positions+clamp", (8, 3, 160, 160, 80)),
    ("displacement", (32, 2, 256, 256)),
]


def bytes_per_voxel(op, d):
    return {"det_fwd": 4 * d + 4, "stats": 4 * d, "det_bwd": 4 * d + 4 + 4 * d, "diff_fwd": 4 + 4 * d, "diff_bwd": 4 * d + 4}[op]


def time_fn(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def make(mode, shape):
    from advchain.augmentor import get_base_grid
    g = torch.Generator(device="cuda").manual_seed(0)
    nd = len(shape) - 2
    coarse = torch.rand((shape[0], nd) + (6,) * nd, device="cuda", generator=g) * 2 - 1
    smooth = torch.nn.functional.interpolate(coarse, size=shape[2:], mode="trilinear" if nd == 3 else "bilinear",
                                             align_corners=True)
    if mode == "displacement":
        f = smooth * 6.0
    else:
        f = get_base_grid(shape[0], *shape[2:], device=torch.device("cuda")) + smooth * 0.08
    w = torch.rand((shape[0], 1) + tuple(shape[2:]), device="cuda", generator=g)
    return f.contiguous().requires_grad_(True), w


def paths(mode, f, w):
    """op -> (hip callable, torch callable); the backwards replay a retained graph, so only the backward is timed"""
    from advchain_amd import ops
    from tests import jacobian_forms as forms
    pos = mode != "displacement"
    det_h = ops.jacobian_det(f, positions=pos, clamp=pos)
    det_t = forms.jacobian_det32(f, pos, pos)
    out = {
        "det_fwd": (lambda: ops.jacobian_det(f.detach(), positions=pos, clamp=pos),
                    lambda: forms.jacobian_det32(f.detach(), pos, pos)),
        "det_bwd": (lambda: torch.autograd.grad(det_h, f, w, retain_graph=True),
                    lambda: torch.autograd.grad(det_t, f, w, retain_graph=True)),
        "stats": (lambda: ops.jacobian_stats(f, positions=pos, clamp=pos),
                  lambda: forms.stats_of(forms.jacobian_det32(f.detach(), pos, pos))),
    }
    if f.dim() == 5:
        x = f.detach()[:, :1].contiguous().requires_grad_(True)
        gs = tuple(w for _ in range(3))
        d_h, d_t = ops.image_diff3d(x), forms.image_diff(x)
        out["diff_fwd"] = (lambda: ops.image_diff3d(x.detach()), lambda: forms.image_diff(x.detach()))
        out["diff_bwd"] = (lambda: torch.autograd.grad(d_h, x, gs, retain_graph=True),
                           lambda: torch.autograd.grad(d_t, x, gs, retain_graph=True))
    return out


def selected(spec):
    return list(enumerate(CASES)) if not spec else [(int(i), CASES[int(i)]) for i in spec.split(",")]


def run(args):
    assert torch.cuda.is_available(), "jacobian_bench needs a GPU"
    rows = []
    for idx, (mode, shape) in selected(args.cases):
        f, w = make(mode, shape)
        nd = len(shape) - 2
        vox = shape[0]
        for s in shape[2:]:
            vox *= s
        for op, (hip, ref) in paths(mode, f, w).items():
            t_h, t_r = [], []
            for _ in range(args.rounds):                   # alternate the two paths
                t_h.append(time_fn(hip, args.iters, args.warmup))
                if not args.no_ref:
                    t_r.append(time_fn(ref, args.iters, args.warmup))
            nbytes = vox * bytes_per_voxel(op, nd if op.startswith(("det", "stats")) else 3)
            row = dict(case=idx, mode=mode, shape=list(shape), op=op, hip_ms=min(t_h), algorithmic_bytes=nbytes,
                       hip_tbps_by_event=nbytes / (min(t_h) * 1e-3) / 1e12)
            if t_r:
                row.update(torch_ms=min(t_r), speedup=min(t_r) / min(t_h))
            rows.append(row)
            print(json.dumps(row), flush=True)
        del f, w
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "jacobian_bench%s.json" % ("_hip_only" if args.no_ref else "")), "w") as fh:
            json.dump(rows, fh, indent=1)


KERNELS = {"k_jac3d_fwd": "det_fwd", "k_jac2d_fwd": "det_fwd", "k_jacobian2d_fwd": "det_fwd", "k_jac3d_bwd": "det_bwd",
           "k_jac2d_bwd": "det_bwd", "k_jacobian2d_bwd": "det_bwd", "k_diff3d_fwd": "diff_fwd", "k_diff3d_bwd": "diff_bwd"}


def summarize(stats_csv, out, spec):
    """Mean kernel times of a --no-ref run of ONE case (rocprofv3 --stats csv) -> achieved bytes/s and share of PEAK_BPS.  The
    statistics run the forward kernel's template with STATS = true (`true>` in the name)."""
    import csv
    (idx, (mode, shape)), = selected(spec)
    nd = len(shape) - 2
    vox = shape[0]
    for s in shape[2:]:
        vox *= s
    lines = []
    for r in csv.DictReader(open(stats_csv)):
        name = r["Name"]
        base = next((k for k in KERNELS if k in name), None)
        if base is None:
            continue
        op = KERNELS[base]
        if op == "det_fwd" and "true>" in name:
            op = "stats"
        ns = float(r["AverageNs"])
        nbytes = vox * bytes_per_voxel(op, nd if op.startswith(("det", "stats")) else 3)
        row = dict(case=idx, shape=list(shape), kernel=name[:100], op=op, calls=int(r["Calls"]), avg_us=ns / 1e3, bytes=nbytes,
                   tbps=nbytes / (ns * 1e-9) / 1e12, share_of_8tbps=nbytes / (ns * 1e-9) / PEAK_BPS)
        lines.append(row)
        print(json.dumps(row))
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "kernel_bandwidth_case%d.json" % idx), "w") as fh:
            json.dump(lines, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
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
