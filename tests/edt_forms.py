"""Brute-force Euclidean distance transforms, signed distance maps and the closed form of the boundary loss of common.loss
(distance_transform_edt, signed_distance_maps, boundary_loss), written from their specification in plain torch (tests only).

    edt(v)     = min over the zero voxels u of the same entry of |S (v - u)|,  S = diag(sampling);  +inf without a zero voxel
    phi_nk(v)  = d(v, F_nk) - d(v, B_nk),  F_nk = {u: labels[n,u] == k},  B_nk its complement;  0 for a class absent from or filling n
    loss       = 1/(N V) sum_n sum_{v counted} sum_{k counted} omega_k p_k(v) phi_nk(v),   omega_k = w_k / sum of the counted w_j
    dL/dx_j(v) = 1/(N V) p_j (omega_j phi_j - sum_k omega_k phi_k p_k)  at a counted voxel, 0 elsewhere."""
import functools

import torch


def _coordinates(sp):
    axes = [torch.arange(s, dtype=torch.int64) for s in sp]
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, len(sp))


def edt_brute(mask, sampling=None, squared=False, dtype=torch.float64):
    """All-pairs distances per leading entry: (B, dims) float64 (squared: the squared distance, an exact integer with unit
    spacing).  `dtype` is the precision of the arithmetic with a sampling (float32: what an fp32 implementation can reach)."""
    mask = torch.as_tensor(mask).cpu()
    B, sp = mask.shape[0], tuple(mask.shape[1:])
    c = _coordinates(sp)
    out = torch.empty((B, c.shape[0]), dtype=torch.float64)
    for b in range(B):
        fg = (mask[b] != 0).reshape(-1)
        zeros = c[~fg]
        if zeros.shape[0] == 0:
            out[b] = float("inf")
            continue
        best = torch.zeros(c.shape[0], dtype=torch.float64)
        idx = torch.nonzero(fg).reshape(-1)
        for i0 in range(0, idx.numel(), 512):
            sel = idx[i0:i0 + 512]
            delta = c[sel][:, None, :] - zeros[None, :, :]
            if sampling is None:
                d2 = (delta * delta).sum(-1).min(1).values.to(torch.float64)
            else:
                s = torch.tensor([float(v) for v in sampling], dtype=dtype)
                sd = delta.to(dtype) * s
                d2 = ((sd * sd).sum(-1)).min(1).values
                if not squared:
                    d2 = d2.sqrt()
                d2 = d2.to(torch.float64)
            best[sel] = d2
        out[b] = best if (squared or sampling is not None) else best.sqrt()
    return out.reshape((B,) + sp)


def signed_maps_brute(labels, K, sampling=None, dtype=torch.float64):
    """(N, dims) labels -> (N, K, dims) float64 signed maps by two brute-force transforms per class."""
    labels = torch.as_tensor(labels).cpu()
    N = labels.shape[0]
    out = torch.zeros((N, K) + tuple(labels.shape[1:]), dtype=torch.float64)
    for k in range(K):
        member = labels == k
        to_member = edt_brute(~member, sampling, dtype=dtype)          # zero voxels of ~member are the members
        to_other = edt_brute(member, sampling, dtype=dtype)
        for n in range(N):
            if bool(member[n].any()) and not bool(member[n].all()):
                out[n, k] = to_member[n] - to_other[n]
    return out


def omega_of(K, weight, ignore_background, dtype):
    w = torch.ones(K, dtype=dtype) if weight is None else torch.as_tensor(weight).detach().cpu().to(dtype).reshape(-1).clone()
    if ignore_background:
        w[0] = 0.0
    return w / w.sum()


def gate_of(x, target):
    """(N,1,dims): 1 at a counted voxel, 0 at -100, NaN at any other label outside [0, K); all ones without labels."""
    if target is None:
        return torch.ones_like(x[:, :1])
    K = x.shape[1]
    g = torch.ones(target.shape, dtype=x.dtype)
    g[(target < 0) | (target >= K)] = float("nan")
    g[target == -100] = 0.0
    return g[:, None]


def _times_gate(v, gate):
    return torch.where(gate == 0, torch.zeros_like(v), v * gate)


def boundary_closed(x, target=None, weight=None, ignore_background=True, sampling=None, dist_maps=None):
    """Value of boundary_loss in x's dtype, on the CPU, differentiable w.r.t. x.  target: labels (gate, and the maps when
    dist_maps is None); dist_maps: the maps (with a target as well: the target only gates, so a test can reuse its maps)."""
    N, K = x.shape[:2]
    maps = signed_maps_brute(target, K, sampling) if dist_maps is None else dist_maps
    maps = maps.detach().to(x.dtype)
    omega = omega_of(K, weight, ignore_background, x.dtype).reshape((1, K) + (1,) * (x.dim() - 2))
    p = torch.softmax(x, 1)
    per_voxel = (p * maps * omega).sum(1, keepdim=True)
    return _times_gate(per_voxel, gate_of(x, target)).sum() / (x.numel() // K)


def boundary_scale(x, target=None, weight=None, ignore_background=True, dist_maps=None):
    """S = 1/(N V) sum omega_k p_k |phi_k| over the counted voxels: the size of the summands of the loss."""
    K = x.shape[1]
    omega = omega_of(K, weight, ignore_background, x.dtype).reshape((1, K) + (1,) * (x.dim() - 2))
    gate = torch.nan_to_num(gate_of(x, target), nan=1.0)
    return float(((torch.softmax(x, 1) * dist_maps.to(x.dtype).abs() * omega).sum(1, keepdim=True) * gate).sum() / (x.numel() // K))


def boundary_gradient(x, maps, gate, omega):
    """The stated gradient formula, for a unit upstream gradient."""
    K = x.shape[1]
    omega = omega.reshape((1, K) + (1,) * (x.dim() - 2))
    p = torch.softmax(x, 1)
    t = (omega * maps * p).sum(1, keepdim=True)
    return _times_gate(p * (omega * maps - t), gate) / (x.numel() // K)


def boundary_loop(x, maps, target=None, weight=None, ignore_background=True):
    """The same value by plain Python loops over entries, classes and voxels."""
    import math
    N, K = x.shape[:2]
    xs, ms = x.reshape(N, K, -1).tolist(), maps.reshape(N, K, -1).tolist()
    ys = None if target is None else target.reshape(N, -1).tolist()
    V = len(xs[0][0])
    w = [1.0] * K if weight is None else [float(a) for a in torch.as_tensor(weight).reshape(-1)]
    first = 1 if ignore_background else 0
    wsum = sum(w[first:])
    total = 0.0
    for n in range(N):
        for v in range(V):
            if ys is not None:
                if ys[n][v] == -100:
                    continue
                if ys[n][v] < 0 or ys[n][v] >= K:
                    return float("nan")
            mx = max(xs[n][k][v] for k in range(K))
            e = [math.exp(xs[n][k][v] - mx) for k in range(K)]
            z = sum(e)
            for k in range(first, K):
                total += w[k] / wsum * e[k] / z * ms[n][k][v]
    return total / (N * V)


# ---- the cases of tests/test_boundary_gpu.py (tests/test_boundary_cpu.py checks what fp32 can reach at the same cases) ----------

EDT_SHAPES = [(2, 5, 7),               # smaller than a wave
              (3, 36, 57),             # a tail in both axes
              (1, 70, 130),            # rows longer than a wave
              (1, 600, 9),             # a column longer than a 64-wide LDS tile of it
              (2, 6, 10, 70),          # 3D
              (1, 33, 9, 5)]           # the longest axis outermost
EDT_PATTERNS = ["fg05", "fg95", "corner", "half", "checker", "sparse", "full_entry"]
SAMPLING = {2: (1.5, 0.7), 3: (2.5, 1.0, 0.8)}
SAMPLING_TOL = 2e-6                       # relative (tests/test_boundary_cpu.py says why it is not 1e-6)

MAP_CASES = [(1, (3, 5, 7)), (3, (3, 36, 57)), (5, (2, 6, 10, 70)), (20, (2, 33, 31)), (70, (2, 9, 8))]     # (K, (N, dims))

LOSS_SHAPES = [(2, 3, 5, 7), (3, 4, 36, 57), (2, 5, 6, 10, 70), (2, 20, 33, 31), (1, 70, 8, 8), (2, 2, 8, 8)]


def mask_pattern(shape, name, seed=0):
    """A bool mask (B, dims); "full_entry" has one more entry in front, all foreground (+inf).  The structured patterns of the
    edge cases put their few zero voxels far from most of the others, so a lost carry or a scan cut short shows: random masks
    make every distance tiny."""
    g = torch.Generator().manual_seed(seed)
    B, sp = shape[0], tuple(shape[1:])
    W = sp[-1]
    if name in ("fg05", "fg95"):
        return torch.rand(shape, generator=g) < (0.05 if name == "fg05" else 0.95)
    if name in ("far_left", "far_right"):                  # the only zero voxel of every row is at x = 0 / x = W-1
        m = torch.ones(shape, dtype=torch.bool)
        m[..., 0 if name == "far_left" else W - 1] = False
        return m
    if name == "ends":                                     # the first and the last row only, and there only the first and the last
        m = torch.ones(shape, dtype=torch.bool)            # chunk of 64: x = 5 and x = W-3 (clamped to the row)
        rows = m.reshape(B, -1, W)
        for r in (0, rows.shape[1] - 1):
            rows[:, r, min(5, W - 1)] = False
            rows[:, r, max(W - 3, 0)] = False
        return m
    if name == "mid_chunk":                                # x = 37 (mod 320) of every row: chunks 0, 5, 10, ... hold a seed, so every
        m = torch.ones(shape, dtype=torch.bool)            # wave's second chunk takes its values from a carry over four empty ones
        m[..., 37::320] = False
        return m
    if name in ("corner", "one_corner"):
        m = torch.ones(shape, dtype=torch.bool)
        m.reshape(B, -1)[:, -1] = False
        return m
    if name == "half":
        m = torch.zeros(shape, dtype=torch.bool)
        m[..., sp[-1] // 2:] = True
        return m
    if name == "checker":
        return (_coordinates(sp).sum(-1) % 2 == 1).reshape(sp)[None].expand(shape).clone()
    if name == "sparse":                                   # two zero voxels: most rows and columns have none
        m = torch.ones(shape, dtype=torch.bool)
        flat = m.reshape(B, -1)
        flat[:, flat.shape[1] // 2] = False
        flat[:, flat.shape[1] // 7] = False
        return m
    if name == "full_entry":
        return torch.cat([torch.ones((1,) + sp, dtype=torch.bool), torch.rand(shape, generator=g) < 0.5])
    raise KeyError(name)


def label_case(K, shape, seed=0):
    """(N, dims) int64 labels: random blocks (4 voxels wide) of the classes 0 .. K-2 (class K-1 is absent), 10 % of the voxels at
    -100 and one voxel with the out-of-range label K + 3; the last entry is filled with class 0, and with K == 1 entry 1 is
    all -100 (the only class is absent there)."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, max(K - 1, 1), (shape[0],) + tuple((s + 3) // 4 for s in shape[1:]), generator=g)
    for a in range(1, len(shape)):
        y = y.repeat_interleave(4, dim=a).narrow(a, 0, shape[a])
    y = y.contiguous()
    y[torch.rand(shape, generator=g) < 0.1] = -100
    y.reshape(shape[0], -1)[0, 3] = K + 3
    y[-1] = 0
    if K == 1:
        y[1] = -100
    return y


def loss_case(shape, seed=0, ignored=True):
    """fp32 logits (N,K,dims) and labels of every class (from 4 classes on: of 0 .. K-2, class K-1 is absent), 10 % at -100 if
    `ignored`."""
    g = torch.Generator().manual_seed(seed)
    N, K = shape[:2]
    x = torch.randn(shape, generator=g) * 2
    y = torch.randint(0, K - 1 if K >= 4 else K, (N,) + tuple(shape[2:]), generator=g)
    if ignored:
        y[torch.rand(y.shape, generator=g) < 0.1] = -100
    return x, y


def loss_weights(K):
    w = [0.5 + 0.25 * (k % 5) for k in range(K)]
    if K >= 3:
        w[1] = 0.0
    return w


# ---- the edge cases of tests/test_edt_edges_gpu.py: the dispatch branches of csrc/edt.hip that the shapes above never reach ----

def edt_plan(W, K, L, I, NF):
    """(chunks, group, launches, TX, lds_bytes) of a call whose rows are W long, with K classes, for an axis pass over lines of
    length L and stride I with NF fields per entry.  A MIRROR of the three loops of edt_run / edt_axis as the header comment of
    csrc/edt.hip states them (64 voxels per ballot, 2048 ballots of a row in LDS at a time; TX halved from 64 until TX lines of
    every field fit in 64 KiB and TX / 2 < I, then down to 16 while the tile is above 16 KiB), written out in plain Python.  It
    tests no kernel: it keeps the case lists below honest about which branch a shape takes (tests/test_boundary_cpu.py)."""
    chunks = (W + 63) // 64
    group = 2048 // chunks
    launches = (K + group - 1) // group
    TX = 64
    while TX > 1 and (TX * L * NF * 4 > 65536 or TX // 2 >= I):
        TX //= 2
    while TX > 16 and TX * L * NF * 4 > 16384:
        TX //= 2
    return chunks, group, launches, TX, TX * L * NF * 4


def edt_axis_passes(dims):
    """[(L, I)] of the axis passes of a spatial shape, the finishing pass last: (H, W) in 2D; (H, W) per z, then (D, H W) in 3D."""
    if len(dims) == 2:
        return [(dims[0], dims[1])]
    return [(dims[1], dims[2]), (dims[0], dims[1] * dims[2])]


def edt_case_plan(K, dims, NF):
    """The plan of a whole call: dict(chunks, group, launches, TX (finishing pass), lds (finishing pass), plain_TX (the second
    pass of a 3D call, which runs one field at a time; None in 2D))."""
    passes = edt_axis_passes(dims)
    chunks, group, launches, TX, lds = edt_plan(dims[-1], K, passes[-1][0], passes[-1][1], NF)
    plain = edt_plan(dims[-1], K, passes[0][0], passes[0][1], 1)[3] if len(passes) == 2 else None
    return dict(chunks=chunks, group=group, launches=launches, TX=TX, lds=lds, plain_TX=plain)


ROW_PATTERNS = ["far_left", "far_right", "ends", "one_corner", "mid_chunk", "sparse", "full_entry"]
# (shape, patterns, what edt_case_plan must say, the branch it is there for).  A pattern is left out of a case where it has no
# zero voxel (mid_chunk on rows shorter than 38), where every voxel is one (far_left on 1-wide rows), or where the brute force
# would take a second or more (thousands of zero AND thousands of foreground voxels on the longest shapes: "fg95" stands in for
# the patterns with near seeds there).
EDGE_EDT_CASES = [
    ((2, 3, 64), ROW_PATTERNS, dict(chunks=1, TX=64), "a row of exactly one chunk: no tail, exist[] all ones"),
    ((1, 3, 256), ROW_PATTERNS, dict(chunks=4, TX=64), "an exact multiple of 64: every wave one full chunk"),
    ((1, 3, 257), ROW_PATTERNS, dict(chunks=5, TX=64), "wave 0 takes a second chunk, of one voxel"),
    ((1, 2, 600), ROW_PATTERNS, dict(chunks=10, TX=64), "every wave takes a second chunk, waves 0 and 1 a third"),
    ((1, 1100, 5), ["far_left", "ends", "one_corner", "sparse", "full_entry"], dict(TX=8, lds=35200), "AXIS_FINISH at TX 8"),
    ((1, 2100, 3), ["far_left", "ends", "one_corner", "sparse", "full_entry"], dict(TX=4, lds=33600), "AXIS_FINISH at TX 4"),
    ((1, 4200, 3), ["fg95", "ends", "one_corner", "sparse"], dict(TX=2, lds=33600), "AXIS_FINISH at TX 2"),
    ((1, 16384, 2), ["ends", "one_corner", "sparse"], dict(TX=1, lds=65536),
     "the longest leading axis accepted: TX 1 and all of the 64 KiB"),
    ((1, 2, 32767), ["far_left", "far_right", "ends", "one_corner", "mid_chunk", "sparse"], dict(chunks=512, TX=64),
     "the longest row accepted: every ballot word of LDS, squared distances of 32766^2 + 1 next to the sentinel"),
    ((2, 300, 1), ["ends", "one_corner", "sparse", "full_entry"], dict(chunks=1, TX=1), "W = 1: one live lane, I = 1"),
    ((2, 1, 300), ROW_PATTERNS, dict(chunks=5, TX=64, lds=256), "H = 1: reach 0, the pass only finishes"),
    ((1, 1, 1), ["one_corner", "full_entry"], dict(chunks=1, TX=1, lds=4), "one voxel"),
    ((1, 1, 9, 70), ["far_left", "ends", "one_corner", "sparse", "full_entry"], dict(TX=64, plain_TX=64, lds=256), "D = 1"),
    ((1, 9, 1, 70), ["far_left", "ends", "one_corner", "sparse", "full_entry"], dict(TX=64, plain_TX=64), "H = 1 in 3D"),
    ((1, 9, 70, 1), ["ends", "one_corner", "sparse", "full_entry"], dict(TX=64, plain_TX=1), "W = 1 in 3D: the second pass at I = 1"),
    ((1, 40, 1, 1), ["ends", "one_corner", "sparse", "full_entry"], dict(TX=1, plain_TX=1), "H = W = 1: I = 1 in both passes"),
    ((1, 3, 1100, 5), ["fg95", "ends", "one_corner", "sparse"], dict(TX=64, plain_TX=8), "the second pass with Oz > 1 at TX 8"),
    ((1, 1100, 3, 5), ["fg95", "ends", "one_corner", "sparse"], dict(TX=8, lds=35200), "the third pass at L = 1100, I = 15"),
]
EDGE_EDT_LIMITS = [(1, 16384, 2), (1, 2, 32767)]

# (K, (N, dims), what edt_case_plan must say with two fields, the branch)
EDGE_MAP_CASES = [
    (2, (1, 600, 9), dict(TX=8, lds=38400), "AXIS_FINISH_SIGNED at TX 8"),
    (2, (1, 2100, 3), dict(TX=2, lds=33600), "AXIS_FINISH_SIGNED at TX 2"),
    (2, (1, 4100, 2), dict(TX=1, lds=32800), "AXIS_FINISH_SIGNED at TX 1"),
    (2, (1, 8192, 2), dict(TX=1, lds=65536), "the longest leading axis accepted with two fields"),
    (70, (1, 3, 1900), dict(chunks=30, group=68, launches=2), "a second launch of k_edt_rows, of two classes"),
    (5, (1, 2, 32767), dict(chunks=512, group=4, launches=2), "the longest row: a second launch of one class"),
    (3, (2, 300, 1), dict(chunks=1, TX=1), "W = 1"),
    (3, (2, 1, 300), dict(chunks=5, TX=64), "H = 1"),
    (3, (1, 9, 1, 70), dict(TX=64, plain_TX=64), "H = 1 in 3D"),
]
EDGE_MAP_LIMITS = [(2, (1, 8192, 2)), (5, (1, 2, 32767))]

# (K, (N, dims), plan with one field, branch): surface_distance_metrics through edt_label_fields
EDGE_SURFACE_CASES = [
    (300, (1, 3, 400), dict(chunks=7, group=292, launches=2), "a second class group through edt_label_fields"),
    (4, (2, 300, 1), dict(chunks=1, TX=1), "W = 1"),
]


def edge_case_id(case):
    """"1x3x257" for a case of EDGE_EDT_CASES, "K70-1x3x1900" for one of the label cases."""
    if isinstance(case[0], int):
        return "K%d-%s" % (case[0], "x".join(map(str, case[1])))
    return "x".join(map(str, case[0]))


def _blocks(K, shape, g):
    """Random blocks (4 voxels wide) of ALL the classes 0 .. K-1."""
    y = torch.randint(0, K, (shape[0],) + tuple((s + 3) // 4 for s in shape[1:]), generator=g)
    for a in range(1, len(shape)):
        y = y.repeat_interleave(4, dim=a).narrow(a, 0, shape[a])
    return y.contiguous()


def plant_second_group(y, first, K):
    """Classes first .. K-1 (the ones a second launch of k_edt_rows writes) as runs of 9 voxels in the middle chunks of the rows of
    entry 0, one class after the other over the rows, 100 voxels apart and away from both ends of the row: present, compact, and
    with distances that reach across many chunks, so that a field of theirs that was not written, or written for another class,
    cannot pass."""
    W = y.shape[-1]
    rows = y[0].reshape(-1, W)
    R = rows.shape[0]
    per_row = (K - first + R - 1) // R
    for i, k in enumerate(range(first, K)):
        x = W // 2 - 4 - 50 * (per_row - 1) + 100 * (i // R)
        assert 64 <= x and x + 9 <= W - 64
        rows[i % R, x:x + 9] = k
    return y


def edge_label_case(K, shape, seed=0):
    """(N, dims) int64 labels of a case of EDGE_MAP_CASES, with voxels at -100 and one out-of-range label (K + 3) in each.
      leading axis above 512: class 0 but for a band of class 1 (rows L/8 .. L/8 + L/32), one voxel of it three rows from the
                      bottom and 20 more at random: distances of 7/8 of the axis outside the class and inside its complement;
      row of 32767:   no class (-100) but for one run of 9 voxels per class: class 0 at the left end of row 0, class 1 at the
                      right end of row 1, classes 2 and 3 across a chunk border, the second group in the middle (all-pairs cost
                      is members times voxels, so the classes have to be small here);
      K = 70:         random blocks of every class but the last two, which plant_second_group() adds;
      otherwise:      random blocks of all the classes."""
    g = torch.Generator().manual_seed(seed)
    N, sp = shape[0], tuple(shape[1:])
    W, V = sp[-1], 1
    for s in sp:
        V *= s
    if W == 32767:
        y = torch.full(shape, -100, dtype=torch.int64)
        y[0, 0, 0:9], y[0, 1, W - 9:W], y[0, 0, 60:69], y[0, 1, 8188:8197] = 0, 1, 2, 3
        plant_second_group(y, 2048 // ((W + 63) // 64), K)
        y[0, 1, 700] = K + 3
        return y
    if sp[0] > 512:
        L = sp[0]
        y = torch.zeros(shape, dtype=torch.int64)
        y[:, L // 8:L // 8 + L // 32] = 1
        y[:, L - 3, W - 1] = 1
        flat = y.reshape(N, -1)
        flat[:, torch.randint(V // 2, V, (20,), generator=g)] = 1
        flat[:, torch.randint(0, V, (40,), generator=g)] = -100
        flat[0, 3] = K + 3
        return y
    group = 2048 // ((W + 63) // 64)
    y = _blocks(min(K, group), shape, g)
    y[torch.rand(shape, generator=g) < 0.1] = -100
    if K > group:
        plant_second_group(y, group, K)
    y.reshape(N, -1)[0, 3] = K + 3
    return y


def edge_surface_pair(K, shape, seed=0):
    """(pred, target) of a case of EDGE_SURFACE_CASES: surface_forms.label_pair, and where K needs a second class group those
    classes planted in both maps, three voxels apart."""
    from tests.surface_forms import label_pair
    p, y = label_pair(K, shape, seed=seed)
    group = 2048 // ((shape[-1] + 63) // 64)
    if K > group:
        plant_second_group(y, group, K)
        q = torch.full_like(p, -1)
        plant_second_group(q, group, K)
        q = torch.roll(q, 3, dims=-1)
        p = torch.where(q >= 0, q, p)
    return p, y


# The references of the edge cases, computed once per process and shared (read-only) by the tests that use them.

@functools.lru_cache(maxsize=None)
def edge_edt_reference(shape, name):
    """(mask, squared distances with unit spacing, distances with SAMPLING), float64."""
    m = mask_pattern(shape, name, seed=len(shape))
    return m, edt_brute(m, squared=True), edt_brute(m, SAMPLING[len(shape) - 1])


@functools.lru_cache(maxsize=None)
def edge_map_reference(K, shape):
    """(labels, maps with unit spacing, maps with SAMPLING), float64."""
    y = edge_label_case(K, shape, seed=K)
    return y, signed_maps_brute(y, K), signed_maps_brute(y, K, SAMPLING[len(shape) - 1])
