"""Times cross_entropy_2D and contour_loss (forward + backward through the Python API) against an ATen formulation of the
reference's computation (log_softmax + nll_loss / the class-repeated Sobel convolutions + masked MSE), alternated in one run
with device events; prints one JSON line per case and writes them to --out.

    python tools/seg_loss_bench.py [--iters 50] [--warmup 10] [--no-ref] [--out DIR]

--no-ref times the HIP path only (the run under `rocprofv3 --kernel-trace --stats`, with --cases 0,1,4,5, whose kernel times
the bytes below turn into bandwidth: tools/seg_loss_bench.py --summarize STATS_CSV --cases 0,1,4,5).  Algorithmic bytes per pixel / voxel, from the shapes:
  ce fwd  : logits 4K (2K bf16) + int64 label 8 + lse 4              ce bwd : logits 4K + label 8 + lse 4 + grad 4K
  contour fwd: input 4K + label 8 + R 8 (2 floats)                   contour bwd: R 8 + grad 4K
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BPS = 8.0e12          # MI355X HBM3E

CASES = [
    ("ce", (32, 4, 256, 256), torch.float32),
    ("ce", (32, 4, 256, 256), torch.bfloat16),
    ("ce", (8, 16, 256, 256), torch.float32),
    ("ce", (8, 40, 256, 256), torch.float32),
    ("contour", (32, 4, 256, 256), torch.float32),
    ("contour", (4, 4, 128, 128, 64), torch.float32),
]


def bytes_per_point(kind, K, dtype, direction):
    xb = 2 if dtype == torch.bfloat16 else 4
    if kind == "ce":
        return xb * K + 8 + 4 if direction == "fwd" else xb * K + 8 + 4 + xb * K
    return 4 * K + 8 + 8 if direction == "fwd" else 8 + 4 * K


def aten_ce(x, y):
    """The reference's cross_entropy_2D work in ATen: log_softmax, channels-last view, nll_loss(reduction none), sum, / NHW."""
    n, c, h, w = x.shape
    lp = F.log_softmax(x, dim=1).permute(0, 2, 3, 1).reshape(-1, c)
    return F.nll_loss(lp, y.reshape(-1), reduction="none").sum() / (n * h * w)


def aten_contour(x, y):
    """The reference's contour_loss work in ATen: one-hot of the labels, Sobel filters repeated over the object classes
    (2D) / one output channel (3D), masked MSE means."""
    K = x.shape[1]
    nd = x.dim() - 2
    oc = K - 1
    oh = torch.eye(K, device=x.device).index_select(0, y.reshape(-1)).view(y.shape + (K,)).movedim(-1, 1)
    h = torch.tensor([1.0, 2.0, 1.0], device=x.device)
    hp = torch.tensor([1.0, 0.0, -1.0], device=x.device)
    if nd == 2:
        ks = [h[:, None] * hp[None, :], hp[:, None] * h[None, :]]
        ws = [k.expand(oc, oc, 3, 3).contiguous() for k in ks]
        conv = F.conv2d
    else:
        a = h[:, None, None] * hp[None, :, None] * h[None, None, :]
        b = h[:, None, None] * h[None, :, None] * hp[None, None, :]
        ws = [k.expand(1, oc, 3, 3, 3).contiguous() for k in (a, a, b)]
        conv = F.conv3d
    mask = torch.ones_like(x)[:, :oc]
    terms = [F.mse_loss(conv(x[:, 1:], wk, padding=1) * mask, conv(oh[:, 1:], wk, padding=1) * mask) for wk in ws]
    return sum(terms) / len(terms)


def make(kind, shape, dtype):
    g = torch.Generator(device="cuda").manual_seed(0)
    K = shape[1]
    if kind == "ce":
        x = (torch.randn(shape, device="cuda", generator=g) * 2).to(dtype).requires_grad_(True)
        y = torch.randint(0, K, (shape[0],) + shape[2:], device="cuda", generator=g)
    else:
        x = torch.softmax(torch.randn(shape, device="cuda", generator=g), 1).requires_grad_(True)
        y = torch.randint(0, K, (shape[0],) + shape[2:], device="cuda", generator=g)
    return x, y


def time_fn(fn, x, iters, warmup):
    for _ in range(warmup):
        torch.autograd.grad(fn(), x)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        torch.autograd.grad(fn(), x)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def run(args):
    from advchain.common.loss import contour_loss, cross_entropy_2D
    assert torch.cuda.is_available(), "seg_loss_bench needs a GPU"
    rows = []
    for kind, shape, dtype in selected(args.cases):
        x, y = make(kind, shape, dtype)
        ours = (lambda: cross_entropy_2D(x, y)) if kind == "ce" else (lambda: contour_loss(x, y))
        ref = (lambda: aten_ce(x, y)) if kind == "ce" else (lambda: aten_contour(x, y))
        row = dict(kind=kind, shape=list(shape), dtype=str(dtype).replace("torch.", ""))
        t_ours, t_ref = [], []
        for _ in range(args.rounds):                   # alternate the two paths
            t_ours.append(time_fn(ours, x, args.iters, args.warmup))
            if not args.no_ref:
                t_ref.append(time_fn(ref, x, args.iters, args.warmup))
        row["hip_fwd_bwd_ms"] = min(t_ours)
        if t_ref:
            row["aten_fwd_bwd_ms"] = min(t_ref)
            row["speedup"] = row["aten_fwd_bwd_ms"] / row["hip_fwd_bwd_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x, y
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "seg_loss_bench%s.json" % ("_hip_only" if args.no_ref else "")), "w") as f:
            json.dump(rows, f, indent=1)


KERNELS = {   # kernel-name prefix -> (kind, direction)
    "k_ce_fwd": ("ce", "fwd"), "k_ce_bwd": ("ce", "bwd"), "k_contour_fwd": ("contour", "fwd"),
    "k_contour_bwd": ("contour", "bwd"), "k_seg_finish": (None, None),
}


def selected(spec):
    return CASES if not spec else [CASES[int(i)] for i in spec.split(",")]


def summarize(stats_csv, out, spec):
    """Per-kernel mean time of the --no-ref run (rocprofv3 --stats csv) -> achieved bandwidth and share of PEAK_BPS.  Each
    template instance runs for exactly one case of CASES (fp32 / bf16 x labels, 2D / 3D), matched by its name."""
    import csv
    cases = selected(spec)
    lines = []
    for r in csv.DictReader(open(stats_csv)):
        name = r["Name"]
        base = next((k for k in KERNELS if k in name), None)
        if base is None:
            continue
        kind, direction = KERNELS[base]
        ns = float(r["AverageNs"])
        case = None
        if kind == "ce":
            bf16 = "unsigned short" in name       # template argument: bf16 storage
            cands = [c for c in cases if c[0] == "ce" and (c[2] == torch.bfloat16) == bf16]
            case = cands[0] if len(cands) == 1 else None
        elif kind == "contour":
            dim = 3 if (base + "<3") in name else 2
            case = next((c for c in cases if c[0] == "contour" and len(c[1]) - 2 == dim), None)
        row = dict(kernel=name[:90], calls=int(r["Calls"]), avg_us=ns / 1e3)
        if case is not None:
            pts = 1
            for s in (case[1][:1] + case[1][2:]):
                pts *= s
            nbytes = pts * bytes_per_point(kind, case[1][1], case[2], direction)
            row.update(case="%s %s %s" % (kind, "x".join(map(str, case[1])), str(case[2]).replace("torch.", "")),
                       bytes=nbytes, tbps=nbytes / (ns * 1e-9) / 1e12, share_of_8tbps=nbytes / (ns * 1e-9) / PEAK_BPS)
        lines.append(row)
        print(json.dumps(row))
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "kernel_bandwidth.json"), "w") as f:
            json.dump(lines, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default=None, help="comma-separated indices into CASES (default: all); the profiled run "
                    "takes one case per kernel instance (0,1,4,5) so that each kernel's time belongs to one shape")
    ap.add_argument("--summarize", metavar="STATS_CSV", default=None)
    args = ap.parse_args()
    if args.summarize:
        summarize(args.summarize, args.out, args.cases)
    else:
        run(args)


if __name__ == "__main__":
    main()
