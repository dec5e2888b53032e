"""CPU-only checks of the state entry points (include/fmd.h, fmd_batch_save_state and its kin): they are exported,
bound in the package, and refuse null arguments and sizes below a blob's header with FMD_ERR_ARG and a sentence
before anything touches the HIP runtime (a fake non-null handle is never dereferenced)."""
import ctypes as C

import numpy as np
import pytest

from __graft_entry__ import load_package

FMD_ERR_ARG = -1
NAMES = ["fmd_batch_state_size", "fmd_batch_save_state", "fmd_batch_load_state", "fmd_batch_export_channels",
         "fmd_batch_import_channels", "fmd_save_state", "fmd_load_state", "fmd_batch_debug_state_skip"]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def test_state_symbols_are_exported(pkg):
    lib = pkg.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in pkg.EXPORTS
    for name in ("save_state", "load_state", "export_channels", "import_channels", "debug_state_skip"):
        assert hasattr(pkg.Batch, name), name
    assert hasattr(pkg.FmDecoder, "SaveState") and hasattr(pkg.FmDecoder, "LoadState")


def _refused(lib, rc, word):
    assert rc == FMD_ERR_ARG
    msg = lib.fmd_last_error()
    assert word in msg, msg
    return msg


def test_state_null_arguments_are_refused(pkg):
    lib = pkg.lib()
    fake = C.c_void_p(1)
    buf = np.zeros(4096, np.uint8)
    ch = np.array([0], dtype=np.uint32)
    n = C.c_size_t()
    assert lib.fmd_batch_state_size(None, 1) == 0
    # save / export: a null batch, a null blob, a null list
    assert b"fmd_batch_save_state" in _refused(lib, lib.fmd_batch_save_state(None, buf.ctypes.data, buf.size, C.byref(n)), b"null")
    _refused(lib, lib.fmd_batch_save_state(fake, None, buf.size, C.byref(n)), b"null")
    assert b"fmd_batch_export_channels" in _refused(
        lib, lib.fmd_batch_export_channels(None, ch.ctypes.data, 1, buf.ctypes.data, buf.size, C.byref(n)), b"null")
    _refused(lib, lib.fmd_batch_export_channels(fake, None, 1, buf.ctypes.data, buf.size, C.byref(n)), b"null")
    _refused(lib, lib.fmd_batch_export_channels(fake, ch.ctypes.data, 1, None, buf.size, C.byref(n)), b"null")
    # load / import
    assert b"fmd_batch_load_state" in _refused(lib, lib.fmd_batch_load_state(None, buf.ctypes.data, buf.size), b"null")
    _refused(lib, lib.fmd_batch_load_state(fake, None, buf.size), b"null")
    assert b"fmd_batch_import_channels" in _refused(
        lib, lib.fmd_batch_import_channels(None, ch.ctypes.data, 1, buf.ctypes.data, buf.size), b"null")
    _refused(lib, lib.fmd_batch_import_channels(fake, None, 1, buf.ctypes.data, buf.size), b"null")
    _refused(lib, lib.fmd_batch_import_channels(fake, ch.ctypes.data, 1, None, buf.size), b"null")
    # the single decoder's pair and the test aid
    assert b"fmd_save_state" in _refused(lib, lib.fmd_save_state(None, buf.ctypes.data, buf.size, C.byref(n)), b"null")
    _refused(lib, lib.fmd_save_state(fake, None, buf.size, C.byref(n)), b"null")
    assert b"fmd_load_state" in _refused(lib, lib.fmd_load_state(None, buf.ctypes.data, buf.size), b"null")
    _refused(lib, lib.fmd_load_state(fake, None, buf.size), b"null")
    assert b"fmd_batch_debug_state_skip" in _refused(lib, lib.fmd_batch_debug_state_skip(None, 0), b"null")


def test_state_sizes_below_the_header_are_refused(pkg):
    lib = pkg.lib()
    fake = C.c_void_p(1)
    buf = np.zeros(64, np.uint8)
    ch = np.array([0], dtype=np.uint32)
    n = C.c_size_t()
    for size in (0, 1, 64):
        _refused(lib, lib.fmd_batch_load_state(fake, buf.ctypes.data, size), b"header")
        _refused(lib, lib.fmd_batch_import_channels(fake, ch.ctypes.data, 1, buf.ctypes.data, size), b"header")
        _refused(lib, lib.fmd_batch_save_state(fake, buf.ctypes.data, size, C.byref(n)), b"header")
        _refused(lib, lib.fmd_batch_export_channels(fake, ch.ctypes.data, 1, buf.ctypes.data, size, C.byref(n)),
                 b"header")
