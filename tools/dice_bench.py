"""Times the supervised loss of a segmentation step, forward plus backward with label targets, three ways on the same GPU and
inputs:
  (a) torch     the composition a user writes without this package: softmax, one_hot, three reductions, F.cross_entropy
  (b) two_calls cross_entropy_2D / cross_entropy_3D plus dice_loss
  (c) fused     dice_ce_loss
The variants alternate inside every round of one process and are timed with device events after a warm-up; a round's figure is
the mean over --iters steps, the spread is min .. max over --rounds rounds.  One JSON line per case, all of them to --out.

    python tools/dice_bench.py [--iters 20] [--warmup 5] [--rounds 5] [--cases 0,3] [--out DIR]

--fused-only ITERS runs (c) alone, ITERS steps per case in the order of CASES: the run to put under
`rocprofv3 --kernel-trace --stats --output-format csv`.  `--summarize TRACE_CSV --fused-only ITERS` then maps the k_dice
dispatches of that kernel trace to the cases by their order and reports mean kernel times and the achieved bytes per second
against the algorithmic bytes, per voxel with e = 4 (fp32) or 2 (bf16) bytes per logit:
  forward : logits K e + labels 8 + lse 4             (sweep two reads the logits again: not counted)
  backward: logits K e + labels 8 + lse 4 + gradient K e
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

SHAPES = [(32, 4, 256, 256), (4, 4, 128, 128, 64), (32, 20, 256, 256)]
CASES = [(s, d) for s in SHAPES for d in ("fp32", "bf16")]
SMOOTH = 1e-5


def voxels(shape):
    n = shape[0]
    for s in shape[2:]:
        n *= s
    return n


def algorithmic_bytes(shape, dtype):
    e = 4 if dtype == "fp32" else 2
    K = shape[1]
    fwd = K * e + 8 + 4
    bwd = K * e + 8 + 4 + K * e
    return voxels(shape) * fwd, voxels(shape) * bwd


def make(shape, dtype):
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(shape, device="cuda", generator=g) * 2
    x = (x if dtype == "fp32" else x.to(torch.bfloat16)).requires_grad_(True)
    y = torch.randint(0, shape[1], (shape[0],) + tuple(shape[2:]), device="cuda", generator=g)
    return x, y


def torch_loss(x, y):
    """Soft Dice + cross entropy in stock torch ops (fp32 arithmetic on bf16 logits, as a careful user writes it)."""
    K = x.shape[1]
    xf = x.float()
    p = torch.softmax(xf, 1)
    t = F.one_hot(y, K).movedim(-1, 1).to(p.dtype)
    axes = tuple(range(2, x.dim()))
    inter, psum, tsum = (p * t).sum(axes), p.sum(axes), t.sum(axes)
    dice = (2 * inter + SMOOTH) / (psum + tsum + SMOOTH)
    return F.cross_entropy(xf, y) + 1 - dice.mean()


def variants(x, y):
    import advchain.common.loss as L
    ce = L.cross_entropy_2D if x.dim() == 4 else L.cross_entropy_3D
    one = torch.ones((), device=x.device)

    def step(loss):
        def run():
            torch.autograd.grad(loss(), x, grad_outputs=one)
        return run
    return {"torch": step(lambda: torch_loss(x, y)),
            "two_calls": step(lambda: ce(x, y) + L.dice_loss(x, y, smooth=SMOOTH)),
            "fused": step(lambda: L.dice_ce_loss(x, y, smooth=SMOOTH))}


def time_fn(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def selected(spec):
    idx = range(len(CASES)) if not spec else [int(i) for i in spec.split(",")]
    return [(i, CASES[i]) for i in idx]


def run(args):
    rows = []
    for idx, (shape, dtype) in selected(args.cases):
        x, y = make(shape, dtype)
        fns = variants(x, y)
        import advchain.common.loss as L
        with torch.no_grad():
            values = {"torch": float(torch_loss(x, y)), "fused": float(L.dice_ce_loss(x, y, smooth=SMOOTH))}
        if args.fused_only:
            for _ in range(args.fused_only):
                fns["fused"]()
            torch.cuda.synchronize()
            continue
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                times[k].append(time_fn(fn, args.iters))
        fb, bb = algorithmic_bytes(shape, dtype)
        row = dict(case=idx, shape=list(shape), dtype=dtype, values=values, algorithmic_bytes=fb + bb)
        for k, t in times.items():
            t = sorted(t)
            row[k + "_ms"] = dict(median=t[len(t) // 2], min=t[0], max=t[-1])
        med = {k: row[k + "_ms"]["median"] for k in times}
        row["torch_over_fused"] = med["torch"] / med["fused"]
        row["two_calls_over_fused"] = med["two_calls"] / med["fused"]
        # faster by more than the spread: the slowest fused round against the fastest torch round
        row["fused_faster_than_torch_beyond_spread"] = row["fused_ms"]["max"] < row["torch_ms"]["min"]
        row["fused_tbps_by_event"] = (fb + bb) / (med["fused"] * 1e-3) / 1e12
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x, y, fns
        torch.cuda.empty_cache()
    if args.out and rows:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "dice_bench.json"), "w") as fh:
            json.dump(rows, fh, indent=1)


def summarize(trace_csv, iters, spec, out):
    """The k_dice dispatches of a --fused-only run, in dispatch order: `iters` (+ 1 forward: the value check) per case."""
    import csv
    rows = sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Start_Timestamp"]))
    per = {}
    for k in ("k_dice_fwd", "k_dice_reduce", "k_dice_finish", "k_dice_bwd"):
        per[k] = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9 for r in rows if k in r["Kernel_Name"]]
    cases = selected(spec)
    nf = iters + 1
    assert len(per["k_dice_fwd"]) == nf * len(cases) and len(per["k_dice_bwd"]) == iters * len(cases), \
        (len(per["k_dice_fwd"]), len(per["k_dice_bwd"]), iters, len(cases))
    lines = []
    for j, (idx, (shape, dtype)) in enumerate(cases):
        fb, bb = algorithmic_bytes(shape, dtype)

        def mean(k, n):
            t = per[k][j * n:(j + 1) * n][1:]             # (the first dispatch of a case: cold caches)
            return sum(t) / len(t)
        tf, tr, tn, tb = mean("k_dice_fwd", nf), mean("k_dice_reduce", nf), mean("k_dice_finish", nf), mean("k_dice_bwd", iters)
        row = dict(case=idx, shape=list(shape), dtype=dtype, fwd_us=tf * 1e6, reduce_us=tr * 1e6, finish_us=tn * 1e6,
                   bwd_us=tb * 1e6, fwd_bytes=fb, bwd_bytes=bb, fwd_tbps=fb / tf / 1e12, bwd_tbps=bb / tb / 1e12,
                   fwd_share_of_8tbps=fb / tf / PEAK_BPS, bwd_share_of_8tbps=bb / tb / PEAK_BPS,
                   kernels_us_per_step=(tf + tr + tn + tb) * 1e6)
        lines.append(row)
        print(json.dumps(row))
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "kernel_bandwidth.json"), "w") as fh:
            json.dump(lines, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fused-only", type=int, default=0, metavar="ITERS")
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default=None, help="comma-separated indices into CASES (default: all)")
    ap.add_argument("--summarize", metavar="TRACE_CSV", default=None)
    args = ap.parse_args()
    if args.summarize:
        summarize(args.summarize, args.fused_only, args.cases, args.out)
    else:
        run(args)


if __name__ == "__main__":
    main()
