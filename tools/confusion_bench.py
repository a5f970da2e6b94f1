"""Times common.metrics.confusion_matrix and overlap_metrics (csrc/seg_confusion.hip) on one GPU, from label maps and from logits:

  matrix / overlap                   confusion_matrix / overlap_metrics on a pair of label maps (N, dims)
  matrix_fp32 / overlap_fp32 / ..    the same from fp32 or bf16 logits (N, K, dims): the argmax is taken inside the pass
  torch                              the stock composition on the same device: per entry bincount(target * K + pred,
                                     minlength=K * K) on the label maps; from logits torch.argmax first
  surface                            surface_distance_metrics, the only route to a voxel Dice before these operators

at (32, 4, 256, 256), (4, 4, 128, 128, 64) and (32, 20, 256, 256) on blob labels (tools/surface_bench.py); the logits are the
one-hot target times 4 plus Gaussian noise.  The variants alternate inside every round (tools/boundary_bench.py: device events
around `iters` steps, median of the rounds).  Each HIP route also reports the bytes the algorithm needs -- 16 a voxel for two label
maps, 4 K or 2 K + 8 from logits -- over its median time, and that rate over the HBM peak of 8 TB/s.  A call is the counter
clear, the pass and (overlap) the finish kernel, so the rate is that of the call, not of the pass alone; the kernel times of a
call come from the device activity records of a profiled run of its own, and the same bytes over the time of `k_confusion`
alone are reported beside them.  One JSON line per case; --out DIR keeps them in DIR/confusion_bench.json and writes DIR/summary.md.

    timeout -k 10 900 python tools/confusion_bench.py [--iters 20] [--warmup 3] [--rounds 7] [--out DIR]

Needs a GPU (no fall-back)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.boundary_bench import SHAPES, rounds_of, stats  # noqa: E402
from tools.surface_bench import blob_pair  # noqa: E402

HBM_PEAK = 8.0e12     # bytes per second (MI355X)


def stock_matrix(pred, target, K):
    """(N, K, K): the composition a user writes today; labels are in range here (it has no answer to -100)."""
    N = target.shape[0]
    key = (target * K + pred).reshape(N, -1)
    return torch.stack([torch.bincount(key[n], minlength=K * K) for n in range(N)]).view(N, K, K)


def kernel_times(step, steps):
    """{kernel: mean us per step} from the device activity records of `steps` steps (tools/boundary_bench.py: kernel_times)."""
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
        for short in ("k_confusion_clear", "k_confusion", "k_overlap_finish", "k_matrix_overlap"):
            if short in name:
                name = short
                break
        acc[name] = acc.get(name, 0.0) + float(getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0))
    return {k: v / steps for k, v in sorted(acc.items())}


def needed_bytes(shape, kind):
    N, K = shape[0], shape[1]
    V = 1
    for s in shape[2:]:
        V *= s
    return N * V * {"labels": 16, "fp32": 4 * K + 8, "bf16": 2 * K + 8}[kind]


def run(args):
    if not torch.cuda.is_available():
        raise SystemExit("confusion_bench needs a GPU")
    from advchain_amd.common.metrics import confusion_matrix, overlap_metrics, surface_distance_metrics
    rows = []
    for shape in SHAPES:
        K = shape[1]
        pred, target = blob_pair(shape)
        g = torch.Generator(device="cuda").manual_seed(1)
        x32 = torch.nn.functional.one_hot(pred, K).movedim(-1, 1).float() * 4
        x32 = (x32 + torch.randn(x32.shape, device="cuda", generator=g)).contiguous()
        logits = {"fp32": x32, "bf16": x32.to(torch.bfloat16)}
        want = stock_matrix(pred, target, K)
        assert torch.equal(confusion_matrix(pred, target, K).matrix, want)
        assert torch.equal(overlap_metrics(pred, target, K).dice, surface_distance_metrics(pred, target, K).dice)
        for x in logits.values():
            assert torch.equal(confusion_matrix(x, target, K).matrix, stock_matrix(x.argmax(1), target, K))
        variants = {"matrix": lambda: confusion_matrix(pred, target, K), "overlap": lambda: overlap_metrics(pred, target, K),
                    "torch": lambda: stock_matrix(pred, target, K), "surface": lambda: surface_distance_metrics(pred, target, K)}
        for name, x in logits.items():
            variants["matrix_" + name] = lambda x=x: confusion_matrix(x, target, K)
            variants["overlap_" + name] = lambda x=x: overlap_metrics(x, target, K)
            variants["labels_out_" + name] = lambda x=x: confusion_matrix(x, target, K, return_labels=True)
            variants["torch_" + name] = lambda x=x: stock_matrix(x.argmax(1), target, K)
        ts = rounds_of(variants, args.iters, args.warmup, args.rounds)
        row = dict(shape=list(shape), ms={k: stats(v) for k, v in ts.items()}, bytes={}, bytes_per_s={}, hbm_share={})
        for k in variants:
            if k.startswith(("torch", "surface")):
                continue
            kind = k.split("_")[-1] if k.split("_")[-1] in ("fp32", "bf16") else "labels"
            b = needed_bytes(shape, kind) + (needed_bytes(shape, "labels") // 2 if k.startswith("labels_out") else 0)   # + 8 a voxel written
            row["bytes"][k] = b
            row["bytes_per_s"][k] = b / (row["ms"][k]["median_ms"] * 1e-3)
            row["hbm_share"][k] = row["bytes_per_s"][k] / HBM_PEAK
        med = lambda k: row["ms"][k]["median_ms"]
        row["torch_over_hip"] = dict(matrix=med("torch") / med("matrix"), overlap=med("torch") / med("overlap"),
                                     **{"matrix_" + n: med("torch_" + n) / med("matrix_" + n) for n in logits},
                                     **{"overlap_" + n: med("torch_" + n) / med("overlap_" + n) for n in logits})
        row["surface_over_overlap"] = med("surface") / med("overlap")
        row["kernel_us"], row["pass_bytes_per_s"] = {}, {}
        for k in row["bytes"]:                               # in a run of its own: the profiler slows the host
            row["kernel_us"][k] = kernel_times(variants[k], args.iters)
            row["pass_bytes_per_s"][k] = row["bytes"][k] / (row["kernel_us"][k]["k_confusion"] * 1e-6)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del pred, target, x32, logits, want, variants
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "confusion_bench.json"), "w") as f:
            json.dump(rows, f, indent=1)
        with open(os.path.join(args.out, "summary.md"), "w") as f:
            f.write(summary(rows, args))


def summary(rows, args):
    out = ["# confusion_matrix / overlap_metrics: tools/confusion_bench.py", "",
           "One MI355X, device events around %d calls, median (min - max) of %d rounds, variants alternating inside a round; blob "
           "labels.  `torch` is argmax (logits only) and a per-entry `bincount(target * K + pred)`; `surface` is "
           "`surface_distance_metrics`.  GB/s: the bytes the algorithm needs over the median time of the whole call (clear, "
           "pass, finish); share of the 8 TB/s HBM peak beside it." % (args.iters, args.rounds), ""]
    for row in rows:
        out += ["## %s" % "x".join(map(str, row["shape"])), "", "| route | ms | GB/s | of HBM peak | torch / route |", "|---|---|---|---|---|"]
        for k, v in row["ms"].items():
            rate = row["bytes_per_s"].get(k)
            ratio = row["torch_over_hip"].get(k)
            out.append("| %s | %.4f (%.4f - %.4f) | %s | %s | %s |" % (
                k, v["median_ms"], v["min_ms"], v["max_ms"], "%.0f" % (rate / 1e9) if rate else "",
                "%.1f %%" % (100 * row["hbm_share"][k]) if rate else "", "%.2f" % ratio if ratio else ""))
        out += ["", "surface_distance_metrics / overlap_metrics: %.1f" % row["surface_over_overlap"], "",
                "Kernel times of a call (device activity records, us) and the needed bytes over the time of `k_confusion` alone:", "",
                "| route | clear | k_confusion | finish | pass GB/s | of HBM peak |", "|---|---|---|---|---|---|"]
        for k, us in row["kernel_us"].items():
            rate = row["pass_bytes_per_s"][k]
            out.append("| %s | %.1f | %.1f | %s | %.0f | %.1f %% |" % (
                k, us.get("k_confusion_clear", 0.0), us["k_confusion"],
                "%.1f" % us["k_overlap_finish"] if "k_overlap_finish" in us else "", rate / 1e9, 100 * rate / HBM_PEAK))
        out.append("")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    run(ap.parse_args())


if __name__ == "__main__":
    main()
