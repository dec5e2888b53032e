"""CPU-only checks of the band scan's C ABI (include/fmd.h, fmd_scan_*): the entry points are exported and bound, bad
arguments are refused with FMD_ERR_ARG and a sentence before the HIP runtime is touched, and without a GPU
fmd_scan_create fails loudly (no CPU fallback)."""
import ctypes as C

import numpy as np
import pytest

from __graft_entry__ import load_package

FMD_ERR_ARG, FMD_ERR_DEVICE = -1, -2
SYMBOLS = ("fmd_scan_create", "fmd_scan_destroy", "fmd_scan_reset", "fmd_scan_slots", "fmd_scan_accumulate_device",
           "fmd_scan_accumulate_device_u8", "fmd_scan_accumulate_host", "fmd_scan_finish_device",
           "fmd_scan_finish_host")


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def _params(pkg, **kw):
    p = pkg.FmdScanParams(2.4e6, 24, 1024, 100e3, 150e3, 10.0, 0.2)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _create(pkg, p, n=1):
    h = C.c_void_p()
    return pkg.lib().fmd_scan_create(C.byref(p), n, 0, C.byref(h))


def test_scan_symbols_are_exported_and_bound(pkg):
    lib = pkg.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in pkg.EXPORTS
    from importlib import import_module
    scan = import_module(pkg.__name__ + ".scan")
    assert hasattr(scan, "Scan") and hasattr(scan, "scan_stations")
    assert C.sizeof(pkg.FmdScanCandidate) == 16


def test_null_arguments_are_refused(pkg):
    lib = pkg.lib()
    h = C.c_void_p()
    assert lib.fmd_scan_create(None, 1, 0, C.byref(h)) == FMD_ERR_ARG
    assert b"null" in lib.fmd_last_error()
    assert lib.fmd_scan_create(C.byref(_params(pkg)), 1, 0, None) == FMD_ERR_ARG
    assert b"null" in lib.fmd_last_error()
    buf = np.zeros(4096, np.float32)
    for rc in (lib.fmd_scan_reset(None, None), lib.fmd_scan_slots(None, None),
               lib.fmd_scan_accumulate_device(None, buf.ctypes.data, 0, 1024, None),
               lib.fmd_scan_accumulate_device_u8(None, buf.ctypes.data, 0, 1024, None),
               lib.fmd_scan_accumulate_host(None, buf.ctypes.data, 0, 1024),
               lib.fmd_scan_finish_device(None, None, None, None, None, 0, None, None),
               lib.fmd_scan_finish_host(None, None, None, None, None, 0, None)):
        assert rc == FMD_ERR_ARG
        assert b"null" in lib.fmd_last_error()
    lib.fmd_scan_destroy(None)  # a no-op


@pytest.mark.parametrize("field,value,word", [
    ("nfft", 3000, b"nfft"), ("nfft", 128, b"nfft"), ("nfft", 8192, b"nfft"),
    ("floor_quantile", 1.0, b"floor_quantile"), ("floor_quantile", -0.1, b"floor_quantile"),
    ("half_width_hz", -50e3, b"half_width_hz"), ("min_separation_hz", -1.0, b"min_separation_hz"),
    ("table_size", 5000, b"table_size"), ("sample_rate_if", -1.0, b"sample_rate_if")])
def test_invalid_parameters_are_refused_with_a_sentence(pkg, field, value, word):
    assert _create(pkg, _params(pkg, **{field: value})) == FMD_ERR_ARG
    msg = pkg.lib().fmd_last_error()
    assert word in msg and len(msg.split()) >= 5, msg


def test_python_layer_refuses_explicit_zero_quantile_and_bad_widths(pkg):
    from importlib import import_module
    scan = import_module(pkg.__name__ + ".scan")
    for kw in ({"floor_quantile": 0.0}, {"floor_quantile": 1.0}, {"half_width_hz": -1.0}, {"nfft": 3000}):
        with pytest.raises(pkg.FmdError, match="fmd error -1"):
            scan.Scan(2.4e6, 1, **kw)


def test_create_without_a_gpu_fails_loudly(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the no-GPU path cannot be observed here")
    assert _create(pkg, _params(pkg)) == FMD_ERR_DEVICE
    assert b"no HIP device" in pkg.lib().fmd_last_error()
