"""Host-side answers about the x+y Gaussian launch (no GPU): advchain_gauss_xy_plan, and advchain_gauss_xy_takes unchanged."""
import ctypes
import re

import pytest

from advchain_amd import _lib

TILES = [(16, 256), (16, 512), (32, 256), (32, 512), (64, 1024)]
LDS_PER_CU = 160 * 1024        # gfx950


def _plan(dims, planes):
    lib = _lib.load()
    form, ty, nt = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.advchain_gauss_xy_plan(len(dims), _lib.dims_array(dims), planes, ctypes.byref(form), ctypes.byref(ty), ctypes.byref(nt))
    return rc, form.value, ty.value, nt.value


def _takes_before(dims, planes):
    """advchain_gauss_xy_takes as it was before the lane form existed (2D: a leading axis of 1)."""
    s0, s1, s2 = ([1] + list(dims))[-3:]
    if s2 % 4 or s2 < 8 or s2 > 512 or s1 < 8 or planes > 65535 or s0 > 65535:
        return False
    ty = 32
    while ty > 8 and (ty + 8) * (2 * s2 + 8) * 4 > 53248:
        ty //= 2
    if ty > s1:
        ty = (s1 + 7) // 8 * 8
    return (ty + 8) * (2 * s2 + 8) * 4 <= 65536


def _lane_rule(dims):
    """rows of 256 voxels: one row a wave (the shape class at which the lane form was measured to win)"""
    return dims[-1] == 256 and dims[-2] >= 8


@pytest.mark.parametrize("dims,planes,form", [
    ((8, 8), 3, 1), ((20, 16), 2, 1), ((40, 64), 2, 1), ((33, 256), 1, 2), ((24, 128), 2, 1), ((5, 12, 32), 2, 1),
    ((16, 80), 2, 1), ((16, 512), 1, 0), ((64, 512), 1, 0), ((64, 508), 1, 1), ((64, 64), 8, 1), ((8, 256), 1, 2),
    ((3, 40, 256), 6, 2),
    ((256, 256), 128, 2),            # cfg-2: the paired field of 32 x 2 -- rows of 256 voxels: the lane form
    ((128, 128, 64), 24, 1),         # cfg-3: 4 x 3, paired -- rows of 64 voxels lost to the staged kernel when measured
    ((160, 160, 80), 24, 1),         # cfg-5: rows of 80 voxels stay with the staged kernel
    ((7, 256), 2, 0), ((64, 6), 2, 0), ((64, 258), 2, 0),
])
def test_plan(dims, planes, form):
    rc, f, ty, nt = _plan(dims, planes)
    assert rc == 0 and f == form
    s1, W = dims[-2], dims[-1]
    if f == 0:
        assert (ty, nt) == (0, 0)
    elif f == 1:
        assert nt == 256 and ty in (8, 16, 24, 32) and (ty + 8) * (2 * W + 8) * 4 <= 65536
    else:
        assert (ty, nt) == (min(32, (s1 + 7) // 8 * 8), 512) and (32, 512) in TILES
        assert (ty + 8) * W * 4 <= LDS_PER_CU // 2                       # two workgroups a CU at the least
        assert (ty + 8) * (W // 4) <= {256: 10, 512: 5, 1024: 5}[nt] * nt   # the rounds the kernels are built for


def test_plan_rejects_bad_arguments():
    lib = _lib.load()
    i = ctypes.c_int(0)
    assert lib.advchain_gauss_xy_plan(2, _lib.dims_array((16, 16)), 2, None, ctypes.byref(i), ctypes.byref(i)) == -1
    assert lib.advchain_gauss_xy_plan(4, _lib.dims_array((16, 16, 16, 16)), 2, ctypes.byref(i), ctypes.byref(i), ctypes.byref(i)) == -1
    assert lib.advchain_gauss_xy_plan(2, _lib.dims_array((16, 16)), -1, ctypes.byref(i), ctypes.byref(i), ctypes.byref(i)) == -1


def test_takes_keeps_its_answers_and_the_plan_follows_it():
    """advchain_gauss_xy_takes (a C++ symbol the composite entries link to) on a grid of shapes against the rule as it stood;
    the plan takes exactly those shapes, and the lane form's are a subset."""
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    takes = getattr(cdll, "_Z23advchain_gauss_xy_takesiPKll")
    takes.restype, takes.argtypes = ctypes.c_bool, [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64]
    n = lanes = 0
    for W in (4, 6, 8, 12, 16, 32, 40, 64, 80, 96, 128, 192, 256, 260, 384, 512, 516):
        for s1 in (1, 7, 8, 9, 16, 31, 64, 256):
            for lead in ((), (1,), (5,), (65536,)):
                for planes in (1, 24, 65535, 65536):
                    dims = lead + (s1, W)
                    want = _takes_before(dims, planes)
                    assert bool(takes(len(dims), _lib.dims_array(dims), planes)) == want, (dims, planes)
                    rc, form, _, _ = _plan(dims, planes)
                    assert rc == 0 and (form != 0) == want, (dims, planes)
                    assert (form == 2) == (want and _lane_rule(dims)), (dims, planes)
                    n += 1
                    lanes += form == 2
    assert n > 2000 and lanes > 50


def test_header_declares_the_new_entries():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "advchain_hip.h")).read()
    for name in ("advchain_gauss_xy_staged", "advchain_gauss_xy_lanes", "advchain_gauss_xy_plan"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in _lib.PROTOTYPES
        assert hasattr(_lib.load(), name)
