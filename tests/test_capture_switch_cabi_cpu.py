"""CPU-only checks of the capture map entry points (include/fmd.h, fmd_batch_set_capture_map and its kin): they are
exported, bound in the package, and refuse null arguments with FMD_ERR_ARG before anything touches the HIP runtime."""
import ctypes as C

import numpy as np
import pytest

from __graft_entry__ import load_package

FMD_ERR_ARG = -1
NAMES = ("fmd_batch_set_capture_map", "fmd_batch_switch_captures", "fmd_batch_retune_channels_to",
         "fmd_batch_get_capture_map")


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def test_capture_map_symbols_are_exported(pkg):
    lib = pkg.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in pkg.EXPORTS
    for meth in ("set_capture_map", "switch_captures", "capture_map", "retune"):
        assert hasattr(pkg.Batch, meth), meth


def test_null_batch_is_refused(pkg):
    lib = pkg.lib()
    m = np.zeros(4, dtype=np.uint32)
    ch = np.array([0], dtype=np.uint32)
    sh = np.array([3], dtype=np.int32)
    cp = np.array([1], dtype=np.uint32)
    out = np.zeros(4, dtype=np.uint32)
    for rc in (lib.fmd_batch_set_capture_map(None, m.ctypes.data, 2),
               lib.fmd_batch_set_capture_map(None, None, 0),
               lib.fmd_batch_switch_captures(None, ch.ctypes.data, cp.ctypes.data, 1),
               lib.fmd_batch_retune_channels_to(None, ch.ctypes.data, sh.ctypes.data, cp.ctypes.data, 1),
               lib.fmd_batch_get_capture_map(None, out.ctypes.data, 4)):
        assert rc == FMD_ERR_ARG
        assert b"null" in lib.fmd_last_error()


def test_null_lists_are_refused_before_the_batch_is_looked_at(pkg):
    """A list pointer that is null is refused whatever n says (also n == 0): the batch pointer here is not a batch,
    so anything that read it or called into the HIP runtime would not come back with FMD_ERR_ARG."""
    lib = pkg.lib()
    fake = C.c_void_p(1)
    ch = np.array([0], dtype=np.uint32)
    sh = np.array([3], dtype=np.int32)
    cp = np.array([1], dtype=np.uint32)
    for rc in (lib.fmd_batch_switch_captures(fake, None, cp.ctypes.data, 1),
               lib.fmd_batch_switch_captures(fake, ch.ctypes.data, None, 1),
               lib.fmd_batch_switch_captures(fake, None, None, 0),
               lib.fmd_batch_retune_channels_to(fake, None, sh.ctypes.data, cp.ctypes.data, 1),
               lib.fmd_batch_retune_channels_to(fake, ch.ctypes.data, None, cp.ctypes.data, 1),
               lib.fmd_batch_retune_channels_to(fake, ch.ctypes.data, sh.ctypes.data, None, 1),
               lib.fmd_batch_get_capture_map(fake, None, 4)):
        assert rc == FMD_ERR_ARG
        assert b"null" in lib.fmd_last_error()
