"""The warm start's C-ABI boundary, without a device: mspmv_set_initial_guess, mspmv_dresidual and mspmv_dresidual_dev
are declared, exported and bound; a null handle is MSPMV_ERR_INVALID; an unknown mode is rejected before the handle
is looked at, and *old is written only by a call that succeeds.  (The sticky round trip on a live handle:
test_gpu_warm_start.py, test_sticky_mode.)"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mspmv_set_initial_guess", "mspmv_dresidual", "mspmv_dresidual_dev")
INVALID = 1


def test_declared_exported_and_bound(mspmv):
    header = open(os.path.join(ROOT, "include", "mspmv.h")).read()
    lib = ctypes.CDLL(mspmv.LIB_PATH)
    for name in NAMES:
        assert re.search(r"MSPMV_API\s+mspmv_status\s+" + name + r"\s*\(", header), name
        assert hasattr(lib, name) and name in mspmv._SIGS, name
    assert re.search(r"MSPMV_X0_ZERO\s*=\s*0\s*,\s*MSPMV_X0_CALLER\s*=\s*1", header)
    assert (mspmv.X0_ZERO, mspmv.X0_CALLER) == (0, 1)
    # the sharded CG's exclusion is written where its caller reads
    assert "x0 = 0" in open(os.path.join(ROOT, "include", "mspmv_dist.h")).read()
    for method in ("set_initial_guess", "residual", "residual_dev"):
        assert callable(getattr(mspmv.GpuCsr, method))


@pytest.mark.parametrize("mode", [0, 1])
def test_null_handle_is_invalid(mspmv, mode):
    old = ctypes.c_int(77)
    assert mspmv.lib.mspmv_set_initial_guess(None, mode, ctypes.byref(old)) == INVALID
    assert b"null handle" in mspmv.lib.mspmv_last_error()
    assert old.value == 77


def test_residual_null_handle_is_invalid(mspmv):
    v = np.zeros(4)
    p = v.ctypes.data_as(ctypes.c_void_p)
    for fn in (mspmv.lib.mspmv_dresidual, mspmv.lib.mspmv_dresidual_dev):
        assert fn(None, p, p, p, 1, p) == INVALID
        assert b"null handle" in mspmv.lib.mspmv_last_error()


@pytest.mark.parametrize("mode", [-1, 2, 7])
def test_bad_mode_is_rejected(mspmv, mode):
    old = ctypes.c_int(77)
    assert mspmv.lib.mspmv_set_initial_guess(None, mode, ctypes.byref(old)) == INVALID
    assert b"unknown mode" in mspmv.lib.mspmv_last_error()
    assert old.value == 77


def test_host_solvers_take_an_initial_guess(mspmv):
    """Every host solver of the binding has the x0 keyword, every *_dev one the warm flag."""
    import inspect

    g = mspmv.GpuCsr
    for fn in (g.cg_single, g.cg_multi, g.bicgstab, g.block_cg, g.pcg_spai, mspmv.pcg_ic0, mspmv.pbicgstab_ilu0):
        assert inspect.signature(fn).parameters["x0"].default is None, fn.__name__
    for fn in (g.cg_dev, g.bicgstab_dev, g.block_cg_dev, g.pcg_spai_dev, mspmv.pbicgstab_ilu0_dev):
        assert inspect.signature(fn).parameters["warm"].default is None, fn.__name__
