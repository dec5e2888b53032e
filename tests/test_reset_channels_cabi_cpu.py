"""CPU-only checks of the single-channel reset (include/fmd.h, fmd_batch_reset_channels): it is exported, bound in
the package, and refuses null arguments with FMD_ERR_ARG before anything touches the HIP runtime."""
import ctypes as C

import numpy as np
import pytest

from __graft_entry__ import load_package

FMD_ERR_ARG = -1


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def test_reset_channels_symbol_is_exported(pkg):
    lib = pkg.lib()
    assert hasattr(lib, "fmd_batch_reset_channels")
    assert "fmd_batch_reset_channels" in pkg.EXPORTS
    assert hasattr(pkg.Batch, "reset_channels")
    # the reference's per-decoder Reset keeps its own surface
    assert hasattr(pkg.FmDecoder, "Reset")


def test_reset_channels_null_arguments_are_refused(pkg):
    lib = pkg.lib()
    ch = np.array([0], dtype=np.uint32)
    assert lib.fmd_batch_reset_channels(None, ch.ctypes.data, 1) == FMD_ERR_ARG
    assert b"null" in lib.fmd_last_error()
    # a null list is refused whatever n says (also n == 0), before the batch is looked at
    fake = C.c_void_p(1)
    assert lib.fmd_batch_reset_channels(fake, None, 1) == FMD_ERR_ARG
    assert b"null" in lib.fmd_last_error()
    assert lib.fmd_batch_reset_channels(fake, None, 0) == FMD_ERR_ARG
    assert lib.fmd_batch_reset_channels(None, None, 0) == FMD_ERR_ARG
    assert b"fmd_batch_reset_channels" in lib.fmd_last_error()
