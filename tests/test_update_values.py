"""mspmv_csr_update_values / _dev / mspmv_update_ms at the C-ABI boundary, as far as it goes without a device
(test_abi.py's ground): the symbols are declared and exported, their ctypes signatures load, a null handle is
MSPMV_ERR_INVALID with a message, and GpuCsr.update_values refuses a wrong length or dtype before the library is
called.  What an update computes is test_gpu_update_values.py's."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mspmv_csr_update_values", "mspmv_csr_update_values_dev", "mspmv_update_ms")
INVALID = 1


def test_declared_and_exported(mspmv):
    header = open(os.path.join(ROOT, "include", "mspmv.h")).read()
    declared = set(re.findall(r"MSPMV_API\s+[\w\s\*]*?\b(mspmv_\w+)\s*\(", header))
    assert set(NAMES) <= declared
    lib = ctypes.CDLL(mspmv.LIB_PATH)
    assert all(hasattr(lib, n) for n in NAMES)
    # the header no longer calls the matrix immutable, and says what an update leaves alone
    assert "the matrix is immutable" not in header
    assert "mspmv_ic0 / mspmv_ilu0 factors" in header


def test_signatures_load(mspmv):
    P, D, I = ctypes.c_void_p, ctypes.c_double, ctypes.c_int
    assert mspmv._SIGS["mspmv_csr_update_values"] == (I, [P, P])
    assert mspmv._SIGS["mspmv_csr_update_values_dev"] == (I, [P, P])
    assert mspmv._SIGS["mspmv_update_ms"] == (D, [P])
    for n in NAMES:
        f = getattr(mspmv.lib, n)
        assert f.restype is mspmv._SIGS[n][0] and list(f.argtypes) == mspmv._SIGS[n][1]


@pytest.mark.parametrize("name", NAMES[:2])
def test_null_handle_is_invalid(mspmv, name):
    v = np.ones(4)
    assert mspmv.STATUS[INVALID] and getattr(mspmv.lib, name)(None, v.ctypes.data) == INVALID
    assert b"null handle" in mspmv.lib.mspmv_last_error()


def test_update_ms_of_no_handle(mspmv):
    assert mspmv.lib.mspmv_update_ms(None) == 0.0


class _Unreachable:
    """Stands where the library handle would: the binding must raise before it reads it."""

    def __getattr__(self, name):
        raise AssertionError("update_values reached the library")


@pytest.mark.parametrize("values", [np.ones(6), np.ones(8), np.ones((7, 1)), np.ones(7, np.float32), np.ones(7, np.int64),
                                    [1.0] * 7, None], ids=["short", "long", "2d", "float32", "int64", "list", "none"])
def test_wrong_values_are_refused_before_the_call(mspmv, monkeypatch, values):
    g = mspmv.GpuCsr.__new__(mspmv.GpuCsr)   # no device: a handle-less object of the right shape
    g.h, g.num_rows, g.num_cols, g.num_nonzeros = None, 3, 3, 7
    monkeypatch.setattr(mspmv, "lib", _Unreachable())
    with pytest.raises(ValueError):
        g.update_values(values)
