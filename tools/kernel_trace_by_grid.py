"""Per (kernel, grid size) of a rocprofv3 kernel-trace CSV: launches per solver call and mean / min / max duration, for the kernels
around the window scatter (the stats CSV averages k_zero_fill, k_det_absmax and k_det_convert over launches of different sizes).

    python tools/kernel_trace_by_grid.py <name>_kernel_trace.csv <solver calls in the traced process>"""
import csv, sys, collections
path, calls = sys.argv[1], float(sys.argv[2])
rows = list(csv.DictReader(open(path)))
keys = ("k_scatter_window2d", "k_det_absmax", "k_det_convert", "k_zero_fill", "k_window_merge2d")
g = collections.defaultdict(list)
for r in rows:
    n = r["Kernel_Name"]
    if not any(k in n for k in keys):
        continue
    short = n.replace("void advchain::", "").replace("advchain::", "").split("(")[0]
    grid = (r.get("Grid_Size_X") or r.get("Grid_Size"), r.get("Grid_Size_Y"), r.get("Grid_Size_Z"))
    g[(short, grid)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
for (short, grid), t in sorted(g.items()):
    print("%-52s grid %-22s %5.1f launches/call  mean %7.1f us  min %7.1f  max %7.1f  -> %6.1f us/call"
          % (short, "x".join(str(x) for x in grid), len(t) / calls, sum(t) / len(t), min(t), max(t), sum(t) / calls))
