"""The C ABI of the reference-side gradient of the consistency loss (csrc/loss_ref.hip) without a GPU: the header declares
advchain_consistency_ref_bwd, the ctypes table binds it, and its argument checks run on the host before any launch."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib_built():
    from advchain_amd import _lib
    from advchain_amd.build import build_library
    build_library()
    return _lib.load()


def test_header_declares_the_entry():
    text = open(os.path.join(ROOT, "include", "advchain_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+advchain_consistency_ref_bwd\s*\(", text)


def test_prototype_table_holds_the_entry():
    from advchain_amd import _lib
    res, args = _lib.PROTOTYPES["advchain_consistency_ref_bwd"]
    assert res is ctypes.c_int and len(args) == 18        # one pointer (stats) more than the fused / three-kernel backward


def test_argument_checks_run_on_the_host():
    from advchain_amd import _lib
    lib = _lib_built()
    assert lib.advchain_version() >= 140
    dims = _lib.dims_array((8, 8))
    rc = lib.advchain_consistency_ref_bwd(None, None, None, None, None, None, None, 1.0, 0.5, 0.5, 1.0, 0, 1, 4, 2, dims, 1, None)
    assert rc < 0 and b"consistency_ref_bwd" in lib.advchain_last_error()
    one = ctypes.c_void_p(16)                              # (never dereferenced: every check below fails before a launch)
    rc = lib.advchain_consistency_ref_bwd(one, one, None, None, None, None, one, 1.0, 0.5, 0.5, 1.0, 0, 1, 70000, 2, dims, 1, None)
    assert rc < 0 and b"consistency_ref_bwd: bad N/K" in lib.advchain_last_error()
    rc = lib.advchain_consistency_ref_bwd(one, one, None, None, one, None, one, 1.0, 0.5, 0.5, 1.0, 0, 1, 4, 2, dims, 3, None)
    assert rc < 0 and b"consistency_ref_bwd: mask" in lib.advchain_last_error()
    rc = lib.advchain_consistency_ref_bwd(one, one, None, None, None, None, one, 1.0, 0.5, 0.5, 1.0, 0, 1, 4, 4, dims, 1, None)
    assert rc < 0 and b"consistency_ref_bwd: bad dims" in lib.advchain_last_error()
    # an empty batch is fine and launches nothing
    assert lib.advchain_consistency_ref_bwd(one, one, None, None, None, None, one, 1.0, 0.5, 0.5, 1.0, 0, 0, 4, 2, dims, 1, None) == 0


def test_register_form_knob_is_clamped():
    from advchain_amd import ops
    lib = _lib_built()
    assert ops.REF_GRAD_REG_MAX_K == 4
    try:
        for k, want in ((0, 0), (3, 3), (9, 4), (-2, 0)):
            lib.advchain_set_ref_grad_reg_max_k(k)
            assert lib.advchain_get_ref_grad_reg_max_k() == want
    finally:
        lib.advchain_set_ref_grad_reg_max_k(4)
