"""Brute-force surface Dice at a tolerance (common.metrics.surface_dice), from its definition on the all-pairs squared distances
of tests/surface_forms.directed_squares (tests only).

    within[n,k,0] = #{a in dA : d(a, dB)^2 <= T},  within[n,k,1] = #{b in dB : d(b, dA)^2 <= T}
    unit spacing: int64 squares against T = min(floor(tau * tau), 2^30 - 1), taken in float64; with a sampling: float64 squares
                  against tau * tau in float64
    surface_dice  = (c0 + c1) / (m0 + m1) in float64; NaN when m0 + m1 == 0; 0 when exactly one border is empty (every distance
                  is +inf: nothing is within)"""
import collections
import math

import torch

Reference = collections.namedtuple("Reference", ["surface_dice", "within", "surface_voxels"])


def threshold(tau, unit):
    """What a squared distance is compared with: an int (unit spacing) or a float."""
    t2 = float(tau) * float(tau)
    if unit:
        return 2 ** 30 - 1 if t2 >= 2 ** 30 - 1 else int(math.floor(t2))
    return t2


def tolerances_of(tolerance, K):
    return [float(tolerance)] * K if not isinstance(tolerance, (list, tuple)) else [float(t) for t in tolerance]


def dice_of(squares, N, K, tolerance, unit):
    """The Reference (float64 / int64, CPU) from directed_squares()."""
    tol = tolerances_of(tolerance, K)
    r = Reference(torch.zeros(N, K, dtype=torch.float64), torch.zeros(N, K, 2, dtype=torch.int64),
                  torch.zeros(N, K, 2, dtype=torch.int64))
    for (n, k), v in squares.items():
        d0, d1, m0, m1 = v[:4]
        r.surface_voxels[n, k] = torch.tensor([m0, m1])
        T = threshold(tol[k], unit)
        if m0 and m1:
            for d, sq in enumerate((d0, d1)):
                sq = sq.long() if unit else sq.double()
                r.within[n, k, d] = int((sq <= T).sum())
        r.surface_dice[n, k] = float(r.within[n, k].sum()) / (m0 + m1) if m0 + m1 else float("nan")
    return r


def smallest_gap(squares, K, tolerance):
    """The smallest relative distance |sq - tau^2| / tau^2 between a (float64) squared distance and its class's threshold."""
    tol = tolerances_of(tolerance, K)
    gap = float("inf")
    for (n, k), v in squares.items():
        if not (v[2] and v[3]):
            continue
        t2 = tol[k] * tol[k]
        for sq in v[:2]:
            gap = min(gap, float(((sq.double() - t2).abs() / t2).min()))
    return gap


def surface_dice_brute(pred, target, K, tolerance, sampling=None):
    from tests.surface_forms import directed_squares
    pred = torch.as_tensor(pred)
    return dice_of(directed_squares(pred, target, K, sampling), pred.shape[0], K, tolerance, sampling is None)
