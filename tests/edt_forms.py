"""Brute-force Euclidean distance transforms, signed distance maps and the closed form of the boundary loss of common.loss
(distance_transform_edt, signed_distance_maps, boundary_loss), written from their specification in plain torch (tests only).

    edt(v)     = min over the zero voxels u of the same entry of |S (v - u)|,  S = diag(sampling);  +inf without a zero voxel
    phi_nk(v)  = d(v, F_nk) - d(v, B_nk),  F_nk = {u: labels[n,u] == k},  B_nk its complement;  0 for a class absent from or filling n
    loss       = 1/(N V) sum_n sum_{v counted} sum_{k counted} omega_k p_k(v) phi_nk(v),   omega_k = w_k / sum of the counted w_j
    dL/dx_j(v) = 1/(N V) p_j (omega_j phi_j - sum_k omega_k phi_k p_k)  at a counted voxel, 0 elsewhere."""
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
    """A bool mask (B, dims); "full_entry" has one more entry in front, all foreground (+inf)."""
    g = torch.Generator().manual_seed(seed)
    B, sp = shape[0], tuple(shape[1:])
    if name in ("fg05", "fg95"):
        return torch.rand(shape, generator=g) < (0.05 if name == "fg05" else 0.95)
    if name == "corner":
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
