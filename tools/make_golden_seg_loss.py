"""Writes tests/golden/g12_seg_loss.npz by RUNNING THE UPSTREAM REFERENCE's contour_loss / One_Hot / cross_entropy_2D
(advchain/common/loss.py:102-220, 252-326) on CPU in fp32.

TEST INFRASTRUCTURE, build container only (the reference never travels).  The fixture holds seeded inputs, the values and
the gradients the reference's own autograd gives w.r.t. `input` (and a soft target), and the One_Hot outputs.

    python tools/make_golden_seg_loss.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle._import_reference import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g12_seg_loss.npz")
CPU = torch.device("cpu")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def logits(shape, seed, scale=2.0):
    return torch.randn(*shape, generator=gen(seed)) * scale


def labels(shape, K, seed):
    return torch.randint(0, K, shape, generator=gen(seed))


# (name, ndim, N, K, dims, label shape ('nd' | 'n1d' | None = soft target), ignore_background, mask ('none' | '1' | 'K' | int))
CONTOUR = [
    ("c2_lab_nd", 2, 2, 4, (12, 10), "nd", True, "none"),
    ("c2_lab_n1d_mask1", 2, 2, 4, (12, 10), "n1d", False, "1"),
    ("c2_soft_maskK", 2, 2, 4, (12, 10), None, True, "K"),
    ("c2_soft_noign_mask1", 2, 2, 3, (9, 11), None, False, "1"),
    ("c2_lab_noign_softmax", 2, 2, 4, (12, 10), "nd", False, "none"),
    ("c2_lab_K2_maskK", 2, 3, 2, (8, 8), "nd", True, "K"),
    ("c3_lab_nd", 3, 2, 4, (6, 5, 7), "nd", True, "none"),
    ("c3_lab_n1d_mask1", 3, 2, 4, (6, 5, 7), "n1d", False, "1"),
    ("c3_soft_maskK", 3, 2, 4, (5, 6, 4), None, True, "K"),
    ("c3_lab_mask2", 3, 2, 4, (5, 6, 4), "nd", True, 2),
    ("c3_soft_noign_none", 3, 1, 3, (4, 5, 6), None, False, "none"),
]

# (name, N, K, H, W, target 'lab' | 'lab_ign' | 'soft', weight None | 'tensor' | 'list', size_average)
CE = [
    ("ce_lab_K4", 2, 4, 8, 12, "lab", None, True),
    ("ce_lab_w_K4", 2, 4, 8, 12, "lab", "tensor", True),
    ("ce_lab_ign_w_K5", 2, 5, 7, 9, "lab_ign", "tensor", True),
    ("ce_lab_ign_K4_nosa", 2, 4, 8, 8, "lab_ign", None, False),
    ("ce_soft_wlist_K4", 2, 4, 8, 12, "soft", "list", True),
    ("ce_soft_K2_nosa", 2, 2, 6, 10, "soft", None, False),
    ("ce_soft_K5", 1, 5, 9, 7, "soft", None, True),
    ("ce_lab_K2", 3, 2, 5, 6, "lab", None, True),
]

ONE_HOT = [("oh_nd", (2, 6, 5), 4), ("oh_n1d", (2, 1, 6, 5), 4), ("oh_3d", (2, 3, 4, 5), 3)]


def main():
    import_reference()
    L = sys.modules["advchain.common.loss"]
    assert L.__file__.startswith(os.environ.get("ADVCHAIN_REFERENCE_ROOT", "/root/reference")), L.__file__
    torch.set_grad_enabled(True)
    arrays, meta = {}, {"contour": [], "ce": [], "one_hot": []}
    for i, (name, nd, N, K, dims, lab, ign, mk) in enumerate(CONTOUR):
        seed = 100 + 10 * i
        # with every class in S, a softmax input and a normalised target make u pure rounding: only the case named
        # *_softmax keeps that (an absolute bound in the tests); the others draw per-class maps in [0, 1)
        prob = ign or name.endswith("_softmax")
        draw = (lambda s: torch.softmax(logits((N, K) + dims, s), dim=1)) if prob else \
            (lambda s: torch.rand((N, K) + dims, generator=gen(s)))
        x = draw(seed).detach().requires_grad_(True)
        if lab is None:
            t = draw(seed + 1).detach().requires_grad_(True)
            target = t
        else:
            y = labels((N,) + dims, K, seed + 1)
            target = y if lab == "nd" else y[:, None]
        if mk == "none":
            m = None
        else:
            mc = 1 if mk == "1" else (K if mk == "K" else int(mk))
            m = torch.rand((N, mc) + dims, generator=gen(seed + 2))
            if mk == "1":
                m = (m > 0.3).float()
        v = L.contour_loss(x, target, use_gpu=False, ignore_background=ign, one_hot_target=lab is not None, mask=m,
                           device=CPU)
        v.backward()
        arrays[name + "__input"] = x.detach().numpy()
        arrays[name + "__target"] = target.detach().numpy()
        if m is not None:
            arrays[name + "__mask"] = m.numpy()
        arrays[name + "__value"] = np.float32(v.item())
        arrays[name + "__grad_input"] = x.grad.numpy()
        if lab is None:
            arrays[name + "__grad_target"] = t.grad.numpy()
        meta["contour"].append(dict(name=name, ignore_background=ign, one_hot_target=lab is not None, mask=m is not None))
    for i, (name, N, K, H, W, tk, wk, sa) in enumerate(CE):
        seed = 500 + 10 * i
        x = logits((N, K, H, W), seed).requires_grad_(True)
        t = None
        if tk == "soft":
            t = torch.softmax(logits((N, K, H, W), seed + 1), dim=1).detach().requires_grad_(True)
            target = t
        else:
            target = labels((N, H, W), K, seed + 1)
            if tk == "lab_ign":
                target[torch.rand((N, H, W), generator=gen(seed + 3)) < 0.2] = -100
        w = None
        if wk is not None:
            wv = (torch.rand(K, generator=gen(seed + 2)) * 2 + 0.25)
            w = wv if wk == "tensor" else [float(a) for a in wv]
            arrays[name + "__weight"] = wv.numpy()
        v = L.cross_entropy_2D(x, target, weight=w, size_average=sa)
        v.backward()
        arrays[name + "__input"] = x.detach().numpy()
        arrays[name + "__target"] = target.detach().numpy()
        arrays[name + "__value"] = np.float32(v.item())
        arrays[name + "__grad_input"] = x.grad.numpy()
        if t is not None:
            arrays[name + "__grad_target"] = t.grad.numpy()
        meta["ce"].append(dict(name=name, weight=wk, size_average=sa))
    for i, (name, shape, depth) in enumerate(ONE_HOT):
        y = labels(shape, depth, 900 + i)
        arrays[name + "__labels"] = y.numpy()
        arrays[name + "__out"] = L.One_Hot(depth, use_gpu=False)(y).numpy()
        meta["one_hot"].append(dict(name=name, depth=depth))
    arrays["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
