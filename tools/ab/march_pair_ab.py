"""Parent library against this tree's, side by side in one process, through the same C entries: bits and time of the three
kernels whose text changed (k_adjoint_march, k_sample_march_flat, k_scatter_march3d_wide).

    python tools/ab/march_pair_ab.py <parent.so> <new.so> <outdir> [--no-time]

Writes <outdir>/ab_bits.json (N = 2 at the smallest shapes that reach each kernel) and <outdir>/ab_time.json (the timing shapes:
torch.equal, then device events, 20 iterations after 3 warm-up, the two libraries alternating over 3 rounds; gate: new median
<= parent median + (max - min of the parent's round medians)).  Exits 1 when an output differs or a backward took another route.
"""
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from advchain_amd import _lib as L   # noqa: E402  (prototypes only)

DEV = "cuda"
ROUTE_GATHER, ROUTE_MARCH = 3, 4


class Lib(object):
    def __init__(self, path):
        self.cdll = ctypes.CDLL(path)
        for name in ("advchain_grid_sample_fwd", "advchain_grid_sample_bwd", "advchain_compose_self_fwd", "advchain_compose_self_bwd",
                     "advchain_scatter_workspace", "advchain_last_bwd_route", "advchain_last_error"):
            res, args = L.PROTOTYPES[name]
            fn = getattr(self.cdll, name)
            fn.restype, fn.argtypes = res, args
            setattr(self, name, fn)

    def check(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s rc=%d: %s" % (what, rc, self.advchain_last_error()))


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dims_arr(dims):
    return (ctypes.c_int64 * len(dims))(*[int(v) for v in dims])


def identity(N, dims):
    D, H, W = dims
    ax = [torch.linspace(-1.0, 1.0, S, dtype=torch.float32) for S in (W, H, D)]
    gx = ax[0][None, None, :].expand(D, H, W)
    gy = ax[1][None, :, None].expand(D, H, W)
    gz = ax[2][:, None, None].expand(D, H, W)
    return torch.stack([gx, gy, gz])[None].repeat(N, 1, 1, 1, 1).contiguous()


def make_field(N, dims, bound, seed):
    """identity + a random displacement of at most 0.9 * bound voxels per axis; the bound is then checked in the kernels' own
    arithmetic: |((g + 1) * 0.5) * (S - 1) - s| < bound for every sample and axis."""
    g = torch.Generator().manual_seed(seed)
    D, H, W = dims
    disp = (torch.rand((N, 3) + tuple(dims), generator=g) * 2 - 1) * (0.9 * bound)
    scale = torch.tensor([2.0 / (W - 1), 2.0 / (H - 1), 2.0 / (D - 1)], dtype=torch.float32)[None, :, None, None, None]
    idn = identity(N, dims)
    f = (idn + disp * scale).contiguous()
    worst = 0.0
    for c, S in enumerate((W, H, D)):
        un = ((f[:, c] + 1.0) * 0.5) * float(S - 1)
        own = ((idn[:, c] + 1.0) * 0.5) * float(S - 1)
        worst = max(worst, float((un - own.round()).abs().max()))
    assert worst < bound, (worst, bound)
    return f.to(DEV), worst


def rnd(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(DEV)


def warp_fwd(lib, inp, grid, padding, clamp, hint):
    N, C = inp.shape[:2]
    out = torch.empty_like(inp)
    da = dims_arr(inp.shape[2:])
    lib.check(lib.advchain_grid_sample_fwd(ptr(inp), ptr(grid), ptr(out), N, C, 3, da, da, 0, padding, clamp | (hint << 8), stream()),
              "grid_sample_fwd")
    return (out,)


def warp_bwd(lib, gout, inp, grid, padding, clamp, halo, need_gg, ws):
    N, C = inp.shape[:2]
    gin = torch.empty_like(inp)
    gg = torch.empty_like(grid) if need_gg else None
    da = dims_arr(inp.shape[2:])
    lib.check(lib.advchain_grid_sample_bwd(ptr(gout), ptr(inp), ptr(grid), ptr(gin), ptr(gg), ptr(ws), N, C, 3, da, da, 0, padding,
                                           clamp, halo, stream()), "grid_sample_bwd")
    return (gin, gg) if need_gg else (gin,)


def self_fwd(lib, phi, phi0, final_mode, hint, want_disp):
    out = torch.empty_like(phi)
    disp = torch.zeros(4096, device=DEV) if want_disp else None
    lib.check(lib.advchain_compose_self_fwd(ptr(phi), ptr(out), ptr(phi0), phi.shape[0], 3, dims_arr(phi.shape[2:]),
                                            final_mode | (hint << 8), ptr(disp), stream()), "compose_self_fwd")
    return (out, disp) if want_disp else (out,)


def self_bwd(lib, gout, phi, halo, ws):
    gphi = torch.empty_like(phi)
    lib.check(lib.advchain_compose_self_bwd(ptr(gout), ptr(phi), ptr(gphi), ptr(ws), 0, halo, phi.shape[0], 3, dims_arr(phi.shape[2:]),
                                            stream()), "compose_self_bwd")
    return (gphi,)


def workspace(lib, N, dims):
    n = lib.advchain_scatter_workspace(N, 3, dims_arr(dims))
    assert n > 0
    return torch.empty(n, device=DEV, dtype=torch.int32)


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def bits_case(rows, old, new, name, fn, want_route=None):
    ro = fn(old)
    route_o = old.advchain_last_bwd_route()
    rn = fn(new)
    route_n = new.advchain_last_bwd_route()
    torch.cuda.synchronize()
    eq = same(ro, rn)
    finite = all(bool(torch.isfinite(x).all()) for x in rn)
    nonzero = all(bool((x != 0).any()) for x in rn)
    row = {"case": name, "equal": eq, "finite": finite, "nonzero": nonzero}
    if want_route is not None:
        row.update(route_parent=route_o, route_new=route_n, route_ok=(route_o == want_route and route_n == want_route))
    rows.append(row)
    print(json.dumps(row), flush=True)


def small_cases(old, new):
    rows = []
    N = 2
    shapes = [(5, 9, 16), (3, 10, 72), (4, 6, 100)]
    modes = [("zeros", 0, 0), ("zeros+clamp", 0, 1), ("border", 1, 0)]
    seed = 100
    for dims in shapes:
        ws_o, ws_n = workspace(old, N, dims), workspace(new, N, dims)
        pick = lambda lib: ws_o if lib is old else ws_n   # noqa: E731
        for C in (1, 4):
            inp = rnd((N, C) + dims, seed + 1)
            gout = rnd((N, C) + dims, seed + 2)
            for bound in (1, 2, 3, 4):
                if bound >= 2 and dims != shapes[0]:
                    continue
                grid, worst = make_field(N, dims, bound, seed + 10 * bound + C)
                for mname, pad, clamp in modes:
                    for gg in (True, False):
                        tag = "warp_bwd dims=%s C=%d bound=-%d %s gg=%d (|disp| <= %.3f)" % (dims, C, bound, mname, gg, worst)
                        bits_case(rows, old, new, tag,
                                  lambda lib: warp_bwd(lib, gout, inp, grid, pad, clamp, -bound, gg, pick(lib)),
                                  want_route=ROUTE_GATHER if bound == 1 else ROUTE_MARCH)
            grid1, worst = make_field(N, dims, 1, seed + 7 + C)
            for mname, pad, clamp in modes:
                bits_case(rows, old, new, "warp_fwd dims=%s C=%d hint=1 %s (|disp| <= %.3f)" % (dims, C, mname, worst),
                          lambda lib: warp_fwd(lib, inp, grid1, pad, clamp, 1))
        phi, worst = make_field(N, dims, 1, seed + 50)
        phi0, _ = make_field(N, dims, 1, seed + 51)
        gout = rnd((N, 3) + dims, seed + 52)
        bits_case(rows, old, new, "self_bwd dims=%s bound=-1 (|disp| <= %.3f)" % (dims, worst),
                  lambda lib: self_bwd(lib, gout, phi, -1, pick(lib)))
        for fm in (0, 1):
            bits_case(rows, old, new, "self_fwd dims=%s hint=1 final_mode=%d with disp_out" % (dims, fm),
                      lambda lib: self_fwd(lib, phi, phi0 if fm else None, fm, 1, True))
        seed += 1000
    return rows


def time_case(old, new, fn, rounds=3, iters=20, warm=3):
    med = {"parent": [], "new": []}
    for _ in range(rounds):
        for key, lib in (("parent", old), ("new", new)):
            for _ in range(warm):
                fn(lib)
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
            for a, b in ev:
                a.record()
                fn(lib)
                b.record()
            torch.cuda.synchronize()
            med[key].append(statistics.median([a.elapsed_time(b) * 1000.0 for a, b in ev]))
    pm, nm = statistics.median(med["parent"]), statistics.median(med["new"])
    spread = max(med["parent"]) - min(med["parent"])
    return {"parent_rounds_us": [round(v, 2) for v in med["parent"]], "new_rounds_us": [round(v, 2) for v in med["new"]],
            "parent_median_us": round(pm, 2), "parent_spread_us": round(spread, 2), "new_median_us": round(nm, 2),
            "gate": "pass" if nm <= pm + spread else "FAIL"}


def timing_cases(old, new, do_time):
    rows = []

    def run(name, kernel, fn, want_route=None):
        ro, rn = fn(old), fn(new)
        route = (old.advchain_last_bwd_route(), new.advchain_last_bwd_route())
        torch.cuda.synchronize()
        row = {"case": name, "kernel": kernel, "equal": same(ro, rn)}
        if want_route is not None:
            row["route_ok"] = route == (want_route, want_route)
        del ro, rn
        if do_time:
            row.update(time_case(old, new, fn))
        rows.append(row)
        print(json.dumps(row), flush=True)

    N, dims = 4, (128, 128, 64)
    ws_o, ws_n = workspace(old, N, dims), workspace(new, N, dims)
    pick = lambda lib: ws_o if lib is old else ws_n   # noqa: E731
    inp, gout = rnd((N, 1) + dims, 1), rnd((N, 1) + dims, 2)
    for bound in (1, 3):
        grid, _ = make_field(N, dims, bound, 10 + bound)
        run("4x1x128x128x64 warp forward, hint %d" % bound, "k_sample_march / k_sample_ring (parent's instructions)",
            lambda lib: warp_fwd(lib, inp, grid, 0, 0, bound))
        run("4x1x128x128x64 warp backward, bound -%d" % bound, "k_adjoint_march (a)" if bound == 1 else "k_scatter_march3d_wide (c)",
            lambda lib: warp_bwd(lib, gout, inp, grid, 0, 0, -bound, True, pick(lib)),
            want_route=ROUTE_GATHER if bound == 1 else ROUTE_MARCH)
    inp4, gout4 = rnd((N, 4) + dims, 3), rnd((N, 4) + dims, 4)
    grid, _ = make_field(N, dims, 1, 21)
    run("4x4x128x128x64 warp backward, bound -1", "k_adjoint_march (a)",
        lambda lib: warp_bwd(lib, gout4, inp4, grid, 0, 0, -1, True, pick(lib)), want_route=ROUTE_GATHER)
    del inp, gout, inp4, gout4, grid, ws_o, ws_n
    for N, dims in ((8, (128, 128, 64)), (2, (160, 160, 80))):
        ws_o, ws_n = workspace(old, N, dims), workspace(new, N, dims)
        phi, _ = make_field(N, dims, 1, 31)
        gout = rnd((N, 3) + dims, 32)
        label = "%dx3x%s" % (N, "x".join(str(v) for v in dims))
        run(label + " self-composition forward, sub-voxel", "k_sample_march_flat (b)" if dims[2] > 64 else "k_sample_march (parent's instructions)",
            lambda lib: self_fwd(lib, phi, None, 0, 1, True))
        run(label + " self-composition backward, bound -1", "k_adjoint_march (a)",
            lambda lib: self_bwd(lib, gout, phi, -1, pick(lib)))
        del phi, gout, ws_o, ws_n
    return rows


def main():
    parent, newp, outdir = sys.argv[1:4]
    do_time = "--no-time" not in sys.argv
    os.makedirs(outdir, exist_ok=True)
    old, new = Lib(parent), Lib(newp)
    small = small_cases(old, new)
    with open(os.path.join(outdir, "ab_bits.json"), "w") as f:
        json.dump(small, f, indent=1)
    big = timing_cases(old, new, do_time)
    with open(os.path.join(outdir, "ab_time.json"), "w") as f:
        json.dump(big, f, indent=1)
    bad = [r["case"] for r in small + big if not r["equal"] or r.get("route_ok") is False or r.get("finite") is False
           or r.get("nonzero") is False]
    fails = [r["case"] for r in big if r.get("gate") == "FAIL"]
    print("cases: %d small + %d timing; not equal / wrong route: %s; gate failures: %s" % (len(small), len(big), bad, fails))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
