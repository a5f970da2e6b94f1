"""adversarial_training with a many-class model, for a kernel trace: where does a call spend its GPU time when the prediction
has K > 4 channels?  The K-channel prediction and the validity mask ride through grid_sample / affine_warp with C = K, i.e.
through the general-C kernels (k_grid_sample_fwd/bwd, k_affine_warp_fwd/bwd of csrc/sampler.hip: the fast formulations are
gated on C <= 4, and the backward's grad_in is a float-atomic scatter).

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k20 -- python tools/many_class_solver_trace.py [--classes 20] [--deterministic]
    python tools/many_class_solver_trace.py --summarize DIR/.../k20_kernel_stats.csv --ms-per-call MS [--out FILE]

Needs a GPU (no fall-back)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUPS = (("general-C warps (C = K)", ("k_grid_sample_fwd", "k_grid_sample_bwd", "k_affine_warp_fwd", "k_affine_warp_bwd")),
          ("passes around the int64 image (deterministic mode)", ("k_det_absmax", "k_det_convert", "k_det_convert_bits")),
          ("wide loss", ("k_lp_stats", "k_lp_edge", "k_lp_bwd", "k_consistency_finish")))


def run(args):
    if not torch.cuda.is_available():
        raise SystemExit("many_class_solver_trace needs a GPU")
    import bench
    from advchain_amd.augmentor import AdvAffine, AdvBias, AdvMorph, AdvNoise, ComposeAdversarialTransformSolver
    dev = torch.device("cuda")
    dims = tuple(args.dims)
    names = ["noise", "bias", "morph", "affine"] if len(dims) == 2 else ["bias", "morph", "affine"]
    cls = {"noise": AdvNoise, "bias": AdvBias, "morph": AdvMorph, "affine": AdvAffine}
    chain = [cls[nm](spatial_dims=len(dims), config_dict=cfg, device=dev) for nm, cfg in bench.transform_configs(dims, args.batch, names)]
    solver = ComposeAdversarialTransformSolver(chain_of_transforms=chain, deterministic=True if args.deterministic else None)
    conv = torch.nn.Conv2d if len(dims) == 2 else torch.nn.Conv3d
    torch.manual_seed(0)
    model = conv(1, args.classes, 3, 1, 1).to(dev).eval()
    data = torch.rand(args.batch, 1, *dims, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for i in range(args.warmup + args.calls):
        if i == args.warmup:
            ev[0].record()
        loss = solver.adversarial_training(data=data, model=model, n_iter=args.n_iter, lazy_load=False, step_sizes=1)
    ev[1].record()
    torch.cuda.synchronize()
    print(json.dumps(dict(classes=args.classes, deterministic=bool(args.deterministic), batch=args.batch, dims=list(dims), n_iter=args.n_iter, calls=args.warmup + args.calls,
                          ms_per_call=ev[0].elapsed_time(ev[1]) / args.calls, loss=float(loss))))


def summarize(stats_csv, out, calls, ms_per_call):
    """Kernel time per traced adversarial_training call, by group.  `naive_conv_*` rows are MIOpen's one-off find pass for the
    user model's convolutions during the first call (profiles/README.md) and are left out of the total."""
    import csv
    rows = [(r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(open(stats_csv))
            if not r["Name"].startswith("naive_conv")]
    total = sum(t for _, _, t in rows)
    lines = [dict(traced_calls=calls, kernel_ms_per_call=total / 1e6 / calls, event_ms_per_call=ms_per_call)]
    for title, prefixes in GROUPS:
        t = sum(t for n, _, t in rows if any(("advchain::" + p + "<") in n or ("advchain::" + p + "(") in n for p in prefixes))
        lines.append(dict(group=title, ms_per_call=t / 1e6 / calls, share_of_kernel_time=t / total,
                          share_of_event_time=(t / 1e6 / calls / ms_per_call) if ms_per_call else None))
    for n, c, t in sorted(rows, key=lambda r: -r[2])[:15]:
        lines.append(dict(kernel=n[:100], calls=c, ms_per_call=t / 1e6 / calls, share_of_kernel_time=t / total))
    for row in lines:
        print(json.dumps(row))
    if out:
        with open(out, "w") as f:
            json.dump(lines, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--dims", type=int, nargs="+", default=[256, 256])
    ap.add_argument("--n-iter", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--deterministic", action="store_true", help="deterministic=True: the fixed-point twins of the general-C warps")
    ap.add_argument("--summarize", metavar="STATS_CSV", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--traced-calls", type=int, default=7, help="--summarize: adversarial_training calls of the traced run")
    ap.add_argument("--ms-per-call", type=float, default=None, help="--summarize: ms_per_call the traced run printed")
    args = ap.parse_args()
    if args.summarize:
        summarize(args.summarize, args.out, args.traced_calls, args.ms_per_call)
    else:
        run(args)


if __name__ == "__main__":
    main()
