"""Times the signed distance maps (csrc/edt.hip) and the boundary loss (csrc/seg_boundary.hip) on one GPU:

  maps   signed_distance_maps(labels, K) on the device against what a user does without it: labels to the host,
         scipy.ndimage.distance_transform_edt twice per class and entry, maps back to the device (host clock around the whole
         round trip, device synchronised; left out with a note when scipy is not installed);
  loss   boundary_loss(x, dist_maps=phi), forward + backward, fp32 and bf16 logits, against the stock torch composition on the
         same device maps, (softmax(x, 1) * phi * omega).sum() / (N V), forward + backward; and boundary_loss(x, target) --
         maps and loss in one call;
  passes the kernels of one signed_distance_maps + boundary_loss step, one by one, from the device activity records of
         torch.profiler in a pass of its own (mean over --profile-steps steps).

Labels are blobs (the argmax of smooth random fields), not noise: with noise every distance is about 1 and the outward scan of
the column passes stops at once.  Device timings: events around --iters steps after --warmup steps, the mean of a round; the
variants alternate inside every round; reported are the median and (min-max) of --rounds rounds, in ms.  One JSON line per
shape; --out DIR keeps them in DIR/boundary_bench.json.

    timeout -k 10 900 python tools/boundary_bench.py [--iters 20] [--warmup 5] [--rounds 5] [--cases 0,2] [--out DIR]

Needs a GPU (no fall-back)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(32, 4, 256, 256), (4, 4, 128, 128, 64), (32, 20, 256, 256)]     # those of profiles/r17/dice/summary.md


def blob_labels(shape, seed=0):
    """(N, dims) int64 on the device: argmax over K smooth random fields (blobs a few dozen voxels across)."""
    N, K, sp = shape[0], shape[1], tuple(shape[2:])
    g = torch.Generator(device="cuda").manual_seed(seed)
    coarse = torch.randn((N, K) + tuple(max(s // 16, 2) for s in sp), device="cuda", generator=g)
    smooth = torch.nn.functional.interpolate(coarse, size=sp, mode="bilinear" if len(sp) == 2 else "trilinear", align_corners=True)
    return smooth.argmax(1).contiguous()


def rounds_of(variants, iters, warmup, rounds):
    """{name: [mean ms of a round]}: device events around `iters` steps; the variants alternate inside every round."""
    out = {k: [] for k in variants}
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b) / iters)
    return out


def stats(ts):
    ts = sorted(ts)
    return dict(median_ms=ts[len(ts) // 2], min_ms=ts[0], max_ms=ts[-1])


def scipy_maps(labels, K, ndi):
    """The user's path today: labels to the host, two transforms per class and entry, the maps back to the device."""
    import numpy as np
    y = labels.cpu().numpy()
    out = np.zeros((y.shape[0], K) + y.shape[1:], dtype=np.float32)
    for n in range(y.shape[0]):
        for k in range(K):
            member = y[n] == k
            if member.any() and not member.all():
                out[n, k] = ndi.distance_transform_edt(~member) - ndi.distance_transform_edt(member)
    return torch.from_numpy(out).to(labels.device)


def kernel_times(step, steps):
    """{kernel name: mean us per step} from the device activity records of `steps` steps."""
    from torch.profiler import ProfilerActivity, profile
    step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
    acc = {}
    for e in prof.events():
        if getattr(e, "device_type", None) is None or "cuda" not in str(e.device_type).lower():
            continue
        name = e.name
        if any(w in name.lower() for w in ("memcpy", "memset")):
            continue
        for short in ("k_edt_rows", "k_boundary_fwd", "k_seg_finish", "k_boundary_bwd"):
            if short in name:
                name = short
        if "k_edt_axis" in name:                       # the template's MODE: 0 plain, 1 finish, 2 finish of the signed maps
            mode = name.split("k_edt_axis")[1]
            name = "k_edt_axis" + ("<finish_signed>" if "2>" in mode or "Li2" in mode else
                                   "<finish>" if "1>" in mode or "Li1" in mode else "<plain>")
        tot = acc.setdefault(name, [0.0, 0])
        tot[0] += float(getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0))
        tot[1] += 1
    return {k: dict(us_per_step=v[0] / steps, launches_per_step=v[1] / steps) for k, v in sorted(acc.items())}


def run(args):
    if not torch.cuda.is_available():
        raise SystemExit("boundary_bench needs a GPU")
    from advchain_amd.common.loss import boundary_loss, signed_distance_maps
    try:
        import scipy.ndimage as ndi
    except ImportError:
        ndi = None
    rows = []
    shapes = SHAPES if not args.cases else [SHAPES[int(i)] for i in args.cases.split(",")]
    for shape in shapes:
        N, K = shape[:2]
        V = 1
        for s in shape[2:]:
            V *= s
        y = blob_labels(shape)
        g = torch.Generator(device="cuda").manual_seed(1)
        x32 = torch.randn(shape, device="cuda", generator=g) * 2
        phi = signed_distance_maps(y, K)
        row = dict(shape=list(shape), mean_abs_phi=float(phi.abs().mean()), max_abs_phi=float(phi.abs().max()))

        row["maps_device"] = stats(rounds_of({"maps": lambda: signed_distance_maps(y, K)}, args.iters, args.warmup, args.rounds)["maps"])
        if ndi is None:
            row["maps_scipy"] = "scipy is not installed: not measured"
        else:
            ts = []
            for _ in range(args.scipy_rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ref = scipy_maps(y, K, ndi)
                torch.cuda.synchronize()
                ts.append(1e3 * (time.perf_counter() - t0))
            row["maps_scipy"] = stats(ts)
            row["maps_max_abs_diff_to_scipy"] = float((ref - phi).abs().max())
            del ref

        omega = torch.full((K,), 1.0 / (K - 1), device="cuda")
        omega[0] = 0.0
        om = omega.reshape((1, K) + (1,) * (len(shape) - 2))
        for tag, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            x = x32.to(dt).requires_grad_(True)

            def fused():
                return torch.autograd.grad(boundary_loss(x, dist_maps=phi), x)

            def composed():
                return torch.autograd.grad((torch.softmax(x.float(), 1) * phi * om).sum() / (N * V), x)

            def from_labels():
                return torch.autograd.grad(boundary_loss(x, y), x)
            ts = rounds_of({"fused": fused, "torch": composed, "from_labels": from_labels}, args.iters, args.warmup, args.rounds)
            row["loss_" + tag] = {k: stats(v) for k, v in ts.items()}
            row["loss_" + tag]["fused_slowest_below_torch_fastest"] = max(ts["fused"]) < min(ts["torch"])
            with torch.no_grad():
                a, b = float(boundary_loss(x, dist_maps=phi)), float((torch.softmax(x.float(), 1) * phi * om).sum() / (N * V))
            row["loss_" + tag]["values"] = [a, b]
            if tag == "fp32":
                row["kernels_fp32"] = kernel_times(from_labels, args.profile_steps)
            del x
        rows.append(row)
        print(json.dumps(row), flush=True)
        del y, x32, phi
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "boundary_bench.json"), "w") as f:
            json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scipy-rounds", type=int, default=3)
    ap.add_argument("--profile-steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default=None, help="comma-separated indices into SHAPES (default: all)")
    run(ap.parse_args())


if __name__ == "__main__":
    main()
