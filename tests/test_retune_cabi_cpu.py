"""CPU-only checks of the retune entry points (include/fmd.h, fmd_batch_retune_channels): they are exported,
bound in the package, and refuse null arguments with FMD_ERR_ARG before anything touches the HIP runtime."""
import ctypes as C

import numpy as np
import pytest

from __graft_entry__ import load_package

FMD_ERR_ARG = -1


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def test_retune_symbols_are_exported(pkg):
    lib = pkg.lib()
    for name in ("fmd_batch_enable_retune", "fmd_batch_retune_channels"):
        assert hasattr(lib, name), name
        assert name in pkg.EXPORTS
    assert hasattr(pkg.Batch, "enable_retune") and hasattr(pkg.Batch, "retune")


def test_null_arguments_are_refused(pkg):
    lib = pkg.lib()
    ch = np.array([0], dtype=np.uint32)
    sh = np.array([3], dtype=np.int32)
    assert lib.fmd_batch_enable_retune(None) == FMD_ERR_ARG
    assert b"null" in lib.fmd_last_error()
    assert lib.fmd_batch_retune_channels(None, ch.ctypes.data, sh.ctypes.data, 1) == FMD_ERR_ARG
    assert b"null" in lib.fmd_last_error()
    # a list pointer that is null is refused whatever n says (also n == 0), before the batch is looked at
    fake = C.c_void_p(1)
    assert lib.fmd_batch_retune_channels(fake, None, sh.ctypes.data, 1) == FMD_ERR_ARG
    assert lib.fmd_batch_retune_channels(fake, ch.ctypes.data, None, 1) == FMD_ERR_ARG
    assert lib.fmd_batch_retune_channels(fake, None, None, 0) == FMD_ERR_ARG
    assert b"null" in lib.fmd_last_error()
