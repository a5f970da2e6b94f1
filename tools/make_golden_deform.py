"""Writes tests/golden/g13_deform.npz by RUNNING THE UPSTREAM REFERENCE's deformation helpers (advchain/augmentor/adv_morph.py:
57-202, 377-452; adv_bias.py:12-48; adv_affine.py:275-287) on CPU in fp32.

TEST INFRASTRUCTURE, build container only (the reference never travels).  The fixture holds seeded inputs, values, the
gradients the reference's own autograd gives under seeded upstream gradients, the final step count of the 3D cases, and the
reference's inspect.signature strings.  Composition and exponentiation gradient cases are drawn so that no sample of any
squaring / composition lies within 1e-3 px of a grid node (a kink of the bilinear weights), like g8_kinks.

    python tools/make_golden_deform.py
"""
import inspect
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle._import_reference import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g13_deform.npz")
CPU = torch.device("cpu")
MARGIN = 1e-3


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(shape, seed, lo=-1.0, hi=1.0):
    return torch.rand(*shape, generator=gen(seed)) * (hi - lo) + lo


def kink_distance(pos):
    """Smallest distance (px) of an unnormalised sampling coordinate to a grid node; pos (N,d,...) normalised, channel 0 ->
    the last axis."""
    d = pos.shape[1]
    best = np.inf
    for c in range(d):
        S = pos.shape[pos.dim() - 1 - c]
        x = ((pos[:, c].double() + 1) * 0.5 * (S - 1)).clamp(0, S - 1)
        inside = (x > 0) & (x < S - 1)
        if inside.any():
            f = x[inside] - torch.floor(x[inside])
            best = min(best, float(torch.minimum(f, 1 - f).min()))
    return best


DIFF = [("d_5x4_c3", (2, 3, 5, 4)), ("d_2x7", (1, 2, 2, 7)), ("d_6x3", (2, 1, 6, 3)), ("d_3x2", (1, 1, 3, 2)),
        ("d_4x4", (2, 2, 4, 4)), ("d_9x70", (1, 2, 9, 70))]
JAC = [("j_5x4", (2, 5, 4), 0.3), ("j_2x3", (1, 2, 3), 0.3), ("j_3x2", (2, 3, 2), 0.3), ("j_4x4", (1, 4, 4), 0.3),
       ("j_fold_8x7", (2, 8, 7), 3.0), ("j_7x66", (1, 7, 66), 0.5)]
# (name, flow1 shape, flow2 shape, spread of the positions)
COMP = [("c2_c3", (2, 3, 6, 5), (2, 2, 4, 7), 1.3), ("c2_c1", (1, 1, 5, 5), (1, 2, 5, 5), 1.0),
        ("c3_c2", (1, 2, 4, 5, 3), (1, 3, 3, 4, 5), 1.25), ("c3_c3", (2, 3, 3, 4, 4), (2, 3, 3, 4, 4), 1.0)]
# (name, shape, amplitude, nb_steps, type)
EXP2 = [("e2_n8", (2, 2, 8, 9), 3.0, 8, "ss"), ("e2_n3", (1, 2, 7, 6), 2.0, 3, "ss"), ("e2_n0", (1, 2, 5, 5), 1.0, 0, "ss"),
        ("e2_euler3", (2, 2, 6, 7), 2.0, 3, "euler")]
EXP3 = [("e3_nogrow", (1, 3, 4, 5, 6), 0.05, 3), ("e3_grow", (2, 3, 4, 4, 5), 1.5, 2), ("e3_n0", (1, 3, 3, 4, 4), 0.02, 0)]
BSPLINE2 = [[1, 1], [2, 3], [4, 4], [3, 2]]
BSPLINE3 = [[1, 1, 1], [2, 2, 3], [3, 2, 2]]
# (name, spatial dims, shape, sigma, iter, kernel_size)
GAUSS = [("g2_s1", 2, (2, 2, 12, 11), 1.0, 1, 5), ("g2_s2_it2", 2, (1, 3, 16, 14), 2.0, 2, 41),
         ("g2_s8", 2, (1, 2, 20, 18), 8.0, 1, 41), ("g3_s1_it2", 3, (1, 3, 8, 7, 9), 1.0, 2, 5),
         ("g3_s2", 3, (1, 2, 9, 8, 7), 2.0, 1, 5), ("g3_s8", 3, (1, 1, 6, 7, 5), 8.0, 1, 41)]


def main():
    import_reference()
    M = sys.modules["advchain.augmentor.adv_morph"]
    B = sys.modules["advchain.augmentor.adv_bias"]
    A = sys.modules["advchain.augmentor.adv_affine"]
    S = sys.modules["advchain.augmentor.adv_compose_solver"]
    assert M.__file__.startswith(os.environ.get("ADVCHAIN_REFERENCE_ROOT", "/root/reference")), M.__file__
    torch.set_grad_enabled(True)
    arrays, meta = {}, {"diff": [], "jac": [], "comp": [], "exp2": [], "exp3": [], "bspline": [], "gauss": []}
    sigs = {}
    for name in ("calculate_image_diff", "calculate_jacobian_determinant", "integrate_by_add", "vectorFieldExponentiation2D",
                 "vectorFieldExponentiation3D", "applyComposition2D", "applyComposition3D"):
        sigs[name] = str(inspect.signature(getattr(M, name)))
    for name in ("bspline_kernel_2d", "bspline_kernel_3d"):
        sigs[name] = str(inspect.signature(getattr(B, name)))
    sigs["calc_segmentation_consistency"] = str(inspect.signature(S.calc_segmentation_consistency))
    sigs["AdvMorph.gaussian_smooth"] = str(inspect.signature(M.AdvMorph.gaussian_smooth))
    sigs["AdvMorph.get_gaussian_kernel"] = str(inspect.signature(M.AdvMorph.get_gaussian_kernel))
    sigs["AdvBias.get_bspline_kernel"] = str(inspect.signature(B.AdvBias.get_bspline_kernel))
    sigs["AdvAffine.make_batch_eye_matrix"] = str(inspect.signature(A.AdvAffine.make_batch_eye_matrix))
    meta["signatures"] = sigs

    for i, (name, shape) in enumerate(DIFF):
        x = rnd(shape, 1000 + i).requires_grad_(True)
        dx, dy = M.calculate_image_diff(x)
        gx, gy = rnd(shape, 1100 + i), rnd(shape, 1200 + i)
        torch.autograd.backward([dx, dy], [gx, gy])
        arrays.update({name + "__x": x.detach().numpy(), name + "__dx": dx.detach().numpy(), name + "__dy": dy.detach().numpy(),
                       name + "__gdx": gx.numpy(), name + "__gdy": gy.numpy(), name + "__grad": x.grad.numpy()})
        meta["diff"].append(dict(name=name))
    for i, (name, (N, H, W), amp) in enumerate(JAC):
        x = (rnd((N, 2, H, W), 2000 + i) * amp).requires_grad_(True)
        det = M.calculate_jacobian_determinant(x)
        g = rnd(det.shape, 2100 + i)
        det.backward(g)
        arrays.update({name + "__x": x.detach().numpy(), name + "__det": det.detach().numpy(), name + "__g": g.numpy(),
                       name + "__grad": x.grad.numpy()})
        meta["jac"].append(dict(name=name, negative=int((det < 0).sum())))
    assert meta["jac"][4]["negative"] > 0
    for i, (name, s1, s2, spread) in enumerate(COMP):
        for k in range(200):
            seed = 3000 + 100 * i + k
            pos = rnd(s2, seed) * spread
            if kink_distance(pos) > MARGIN:
                break
        else:
            raise RuntimeError("no kink-free draw for " + name)
        f1 = rnd(s1, seed + 50).requires_grad_(True)
        pos = pos.requires_grad_(True)
        fn = M.applyComposition2D if len(s1) == 4 else M.applyComposition3D
        out = fn(f1, pos)
        g = rnd(out.shape, seed + 60)
        out.backward(g)
        arrays.update({name + "__flow1": f1.detach().numpy(), name + "__flow2": pos.detach().numpy(), name + "__out": out.detach().numpy(),
                       name + "__g": g.numpy(), name + "__grad1": f1.grad.numpy(), name + "__grad2": pos.grad.numpy()})
        meta["comp"].append(dict(name=name, seed=seed))
    for i, (name, shape, amp, n, typ) in enumerate(EXP2):
        for k in range(400):
            seed = 4000 + 100 * i + k
            r = rnd(shape, seed)      # |v| bounded away from 0: phi_0 = id + v / 2^n must not sit on the nodes
            v = torch.sign(r) * (0.4 + 0.6 * r.abs()) * amp * (2.0 / (shape[2] - 1))
            # the start grid and every squaring's input must stay clear of the kinks
            phi = M.get_base_grid(shape[0], shape[2], shape[3], device=CPU) + v / (2.0 ** n)
            phi0, ok = phi, kink_distance(phi) > MARGIN
            for _ in range(max(n, 0)):
                if not ok:
                    break
                phi = M.applyComposition2D(phi if typ == "ss" else phi0, phi)
                ok = kink_distance(phi) > MARGIN
            if ok:
                break
        else:
            raise RuntimeError("no kink-free draw for " + name)
        v = v.requires_grad_(True)
        out = M.vectorFieldExponentiation2D(v, nb_steps=n, type=typ, device=CPU)
        g = rnd(out.shape, seed + 70)
        out.backward(g)
        arrays.update({name + "__duv": v.detach().numpy(), name + "__out": out.detach().numpy(), name + "__g": g.numpy(),
                       name + "__grad": v.grad.numpy()})
        meta["exp2"].append(dict(name=name, nb_steps=n, type=typ, seed=seed))
    for i, (name, shape, amp, n) in enumerate(EXP3):
        v = rnd(shape, 5000 + i) * amp
        nfin, nrm = n, float(torch.norm(v))
        while float(torch.norm(v / (2.0 ** nfin))) > 0.5:
            nfin += 1
        for m in range(-3, 12):       # no norm within 1e-4 of the threshold
            assert abs(nrm / 2.0 ** m - 0.5) > 1e-4, (name, m)
        out = M.vectorFieldExponentiation3D(v, nb_steps=n, device=CPU)
        arrays.update({name + "__duv": v.numpy(), name + "__out": out.numpy()})
        meta["exp3"].append(dict(name=name, nb_steps=n, n_final=nfin, grows=nfin > n))
    assert meta["exp3"][1]["grows"] and not meta["exp3"][0]["grows"]
    for sp in BSPLINE2 + BSPLINE3:
        for order in (1, 2, 3):
            fn = B.bspline_kernel_2d if len(sp) == 2 else B.bspline_kernel_3d
            name = "b%dd_%s_o%d" % (len(sp), "x".join(map(str, sp)), order)
            arrays[name] = fn(sp, order=order, asTensor=False)
            meta["bspline"].append(dict(name=name, spacing=sp, order=order))

    class Holder(object):
        use_gpu = False
        get_gaussian_kernel = M.AdvMorph.get_gaussian_kernel
        gaussian_smooth = M.AdvMorph.gaussian_smooth

    for i, (name, nd, shape, sigma, it, ks) in enumerate(GAUSS):
        h = Holder()
        h.spatial_dims = nd
        x = rnd(shape, 6000 + i)
        with torch.no_grad():
            y = h.gaussian_smooth(x, iter=it, kernel_size=ks, sigma=sigma)
        arrays.update({name + "__x": x.numpy(), name + "__y": y.numpy()})
        k = h.get_gaussian_kernel(kernel_size=ks, sigma=sigma, channels=shape[1]).weight
        if k.numel() <= 20000:
            arrays[name + "__weight"] = k.detach().numpy()
        meta["gauss"].append(dict(name=name, nd=nd, sigma=sigma, iter=it, kernel_size=ks, taps=int(k.shape[-1]),
                                  weight=k.numel() <= 20000))
    for nd in (2, 3):
        h = Holder()
        h.spatial_dims = nd
        arrays["eye%d" % nd] = A.AdvAffine.make_batch_eye_matrix(h, 3, CPU).numpy()
    arrays["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
