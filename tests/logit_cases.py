"""Deterministic logits (N, K, dims) and int64 labels (N, dims) by regime, for the softmax-family losses (plain torch on the CPU,
tests only).  tests/test_logit_cases_cpu.py checks what each regime promises; tests/test_logit_range_gpu.py feeds them to every
kernel that takes a softmax.

    base        randn * 3                                             the control: the range every other loss test stays in
    offset+/-   base + 1000 / base - 1000                             shift invariance; lse of magnitude 1000
    saturated   randn * 60                                            fp32 probabilities of exactly 1 and exactly 0; a fifth of the
                                                                      labels is moved off the argmax (confident and wrong)
    mixed       randn * 2^u, u uniform in [-30, 6] per voxel          all-equal probabilities next to saturated ones in one wave
    huge        base, +1e30 in one class and -1e30 in another at      exp(x - max) is exactly 0 for every other class; the label sits on
                min(8, V) voxels of entry 0                           the +1e30 class, so the value stays finite in fp32
    masked      base with -inf by voxel index v % 4: 0 class 0;       a masked class in front, two in front, in the middle, at the end;
                1 classes 0 and 1 (K >= 3, else class 0); 2 class     labels that pointed at a masked class are moved to the argmax
                K // 2; 3 class K - 1 -- every fourth lane-group
                (v // 4) % 4 == 3 left untouched
    poison      base with one NaN (class 0) and one +inf (class       non-finite propagation
                K - 1) at two voxels of entry 1

The masked patterns interleave by voxel (a lane of the supervised kernels owns 4 consecutive voxels, so every lane that holds
masked voxels holds all four patterns) and leave whole 4-voxel groups untouched beside them.  With bf16=True the values are
rounded to bf16 first (returned as fp32 that bf16 holds exactly) and everything derived -- argmax, moved labels -- is taken
from the rounded values, so a float64 reference built from the returned tensor starts from exactly what a kernel reads."""
import torch

REGIMES = ("base", "offset+", "offset-", "saturated", "mixed", "huge", "masked", "poison")
FINITE = tuple(r for r in REGIMES if r not in ("masked", "poison"))      # every logit finite
HUGE = 1e30
# exponent range of `mixed`.  Probabilities that agree to one fp32 ulp need logits within 2^-24 of each other, so the lower end
# lies below -24: at 2^-20 the probabilities of a voxel still differ by 16 ulp.
MIXED_U = (-30.0, 6.0)


def _generator(regime, seed):
    return torch.Generator().manual_seed(1000 * seed + REGIMES.index(regime))


def masked_pattern(V):
    """(V,) int: 0..3 the pattern of tests/logit_cases.py's table at that voxel, -1 untouched."""
    v = torch.arange(V)
    return torch.where((v // 4) % 4 == 3, torch.full_like(v, -1), v % 4)


def masked_classes(pattern, K):
    """The classes that pattern 0..3 sets to -inf."""
    return {0: [0], 1: [0, 1] if K >= 3 else [0], 2: [K // 2], 3: [K - 1]}[pattern]


def huge_voxels(V):
    """The voxels of entry 0 that carry +-1e30, spread over the entry."""
    n = min(8, V)
    return [(2 * i + 1) * V // (2 * n) for i in range(n)]


def poison_voxels(V):
    """(the voxel of entry 1 with the NaN, the one with +inf)."""
    return V // 3, (2 * V) // 3


def logits(regime, N, K, dims, seed=0, bf16=False):
    """(x, y): fp32 logits (N, K) + dims and int64 labels (N,) + dims of one regime; another seed is another draw."""
    assert regime in REGIMES, regime
    g = _generator(regime, seed)
    shape = (N, K) + tuple(dims)
    V = 1
    for s in dims:
        V *= s
    base = torch.randn(shape, generator=g)
    y = torch.randint(0, K, (N, V), generator=g)
    if regime == "saturated":
        x = base * 60
    elif regime == "mixed":
        # one u per voxel: the N V equally spaced points of the range, both ends included, in random order -- a 7-voxel entry
        # still meets both ends
        strata = torch.randperm(N * V, generator=g).float() / max(N * V - 1, 1)
        u = (strata * (MIXED_U[1] - MIXED_U[0]) + MIXED_U[0]).reshape((N, 1) + tuple(dims))
        x = base * torch.pow(2.0, u)
    elif regime.startswith("offset"):
        x = base * 3 + (1000.0 if regime == "offset+" else -1000.0)
    else:
        x = base * 3
    x = x.reshape(N, K, V)
    if regime == "huge":
        for i, v in enumerate(huge_voxels(V)):
            x[0, i % K, v] = HUGE
            if K > 1:
                x[0, (i + 1) % K, v] = -HUGE
            y[0, v] = i % K
    elif regime == "masked":
        pat = masked_pattern(V)
        for p in range(4):
            for c in masked_classes(p, K):
                x[:, c, pat == p] = float("-inf")
    elif regime == "poison":
        nan_v, inf_v = poison_voxels(V)
        x[1, 0, nan_v] = float("nan")
        x[1, K - 1, inf_v] = float("inf")
    if bf16:
        x = x.bfloat16().float()
    if regime == "saturated":
        top = x.argmax(1)
        wrong = torch.arange(V) % 5 == 0
        y = torch.where(wrong[None], (top + 1) % K, top)
    elif regime == "masked":
        at_label = x.gather(1, y[:, None])[:, 0]
        y = torch.where(torch.isinf(at_label), x.argmax(1), y)
    return x.reshape(shape).contiguous(), y.reshape((N,) + tuple(dims)).contiguous()


def soft_target(N, K, dims, seed=0):
    """A soft target (N, K) + dims, fp32, rows of probabilities (every entry positive)."""
    g = torch.Generator().manual_seed(7000 + seed)
    return torch.softmax(torch.randn((N, K) + tuple(dims), generator=g) * 2, 1).contiguous()


def binary_mask(N, K, dims, seed=0):
    """A 0/1 mask (N, K) + dims with about a fifth of zeros, channels distinct."""
    g = torch.Generator().manual_seed(8000 + seed)
    return (torch.rand((N, K) + tuple(dims), generator=g) > 0.2).float().contiguous()


# ---- the shapes of tests/test_logit_range_gpu.py (N = 2 throughout) -----------------------------------------------------------
N = 2
# supervised losses: the scalar path with partial tiles, the 16-byte path, 3D odd and 3D aligned; K = 18 crosses the 16-class
# chunk of the Dice sums
SUPERVISED = (((11, 20), 3), ((12, 64), 4), ((3, 5, 7), 5), ((5, 6, 64), 4), ((11, 20), 18))
# consistency loss, dims and K of tests/test_ops_gpu.py::test_kl_term_in_every_kernel_variant, one per variant: fused 2D rows
# (K = 2, 4), 16-byte three-kernel form and marching edges (K = 5), generic per-voxel kernels (K = 6; odd V), fused z-march and
# marching 3D (K = 4, 5), generic 3D; then the last register K, and the run-time-K kernels on single-row volumes
CONSISTENCY = (((12, 64), 2), ((12, 64), 4), ((12, 64), 5), ((11, 20), 6), ((9, 11), 4), ((5, 6, 64), 4), ((5, 6, 64), 5),
               ((3, 5, 7), 2), ((11, 20), 16), ((1, 7), 17), ((1, 7), 20))
