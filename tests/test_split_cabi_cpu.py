"""CPU-only checks of the band splitter's C ABI (include/fmd.h, fmd_split_*): the entry points are exported and bound,
bad arguments are refused with FMD_ERR_ARG and a sentence naming the field before the HIP runtime is touched, and
without a GPU fmd_split_create fails loudly (no CPU fallback)."""
import ctypes as C

import numpy as np
import pytest

from __graft_entry__ import load_package

FMD_ERR_ARG, FMD_ERR_DEVICE = -1, -2
SYMBOLS = ("fmd_split_create", "fmd_split_destroy", "fmd_split_reset", "fmd_split_set_shifts", "fmd_split_rows",
           "fmd_split_out_rate", "fmd_split_max_out_samples", "fmd_split_get_taps", "fmd_split_tile_samples",
           "fmd_split_debug_table_versions", "fmd_split_process_device", "fmd_split_process_host")


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def _params(pkg, **kw):
    p = pkg.FmdSplitParams(9.6e6, 4, 0, 0.0, 0, 0.0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _create(pkg, p, n_captures=1, n_bands=2, shifts=(1, -1)):
    h = C.c_void_p()
    sh = np.asarray(shifts, np.int32)
    return pkg.lib().fmd_split_create(C.byref(p), n_captures, n_bands, sh.ctypes.data, 0, C.byref(h))


def test_split_symbols_are_exported_and_bound(pkg):
    lib = pkg.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in pkg.EXPORTS
    from importlib import import_module
    split = import_module(pkg.__name__ + ".split")
    assert hasattr(split, "Splitter") and hasattr(split, "plan_bands")
    assert C.sizeof(pkg.FmdSplitParams) == 32


def test_null_arguments_are_refused(pkg):
    lib = pkg.lib()
    h = C.c_void_p()
    sh = np.zeros(2, np.int32)
    assert lib.fmd_split_create(None, 1, 2, sh.ctypes.data, 0, C.byref(h)) == FMD_ERR_ARG
    assert b"null" in lib.fmd_last_error()
    assert lib.fmd_split_create(C.byref(_params(pkg)), 1, 2, None, 0, C.byref(h)) == FMD_ERR_ARG
    assert b"null" in lib.fmd_last_error()
    assert lib.fmd_split_create(C.byref(_params(pkg)), 1, 2, sh.ctypes.data, 0, None) == FMD_ERR_ARG
    assert b"null" in lib.fmd_last_error()
    buf = np.zeros(4096, np.float32)
    n = C.c_uint()
    for rc in (lib.fmd_split_reset(None, None), lib.fmd_split_set_shifts(None, sh.ctypes.data, 2),
               lib.fmd_split_rows(None), lib.fmd_split_debug_table_versions(None), lib.fmd_split_get_taps(None, buf.ctypes.data, 16),
               lib.fmd_split_process_device(None, buf.ctypes.data, 0, 0, 1024, buf.ctypes.data, 512, C.byref(n), None),
               lib.fmd_split_process_host(None, buf.ctypes.data, 0, 0, 1024, buf.ctypes.data, 512, C.byref(n))):
        assert rc == FMD_ERR_ARG
        assert b"null" in lib.fmd_last_error()
    assert lib.fmd_split_out_rate(None) == 0.0 and b"null" in lib.fmd_last_error()
    assert lib.fmd_split_max_out_samples(None, 16) == 0 and b"null" in lib.fmd_last_error()
    assert lib.fmd_split_tile_samples(None) == 0 and b"null" in lib.fmd_last_error()
    lib.fmd_split_destroy(None)  # a no-op


def test_a_format_outside_fmd_iq_is_refused_before_anything_else(pkg):
    lib = pkg.lib()
    buf = np.zeros(64, np.float32)
    for fmt in (-1, 4, 99):
        assert lib.fmd_split_process_device(None, buf.ctypes.data, fmt, 0, 16, buf.ctypes.data, 8, None,
                                            None) == FMD_ERR_ARG
        assert b"iq_format" in lib.fmd_last_error()
        assert lib.fmd_split_process_host(None, buf.ctypes.data, fmt, 0, 16, buf.ctypes.data, 8, None) == FMD_ERR_ARG
        assert b"iq_format" in lib.fmd_last_error()


@pytest.mark.parametrize("field,value,word", [
    ("sample_rate_in", 0.0, b"sample_rate_in"), ("sample_rate_in", -1.0, b"sample_rate_in"),
    ("sample_rate_in", float("nan"), b"sample_rate_in"),
    ("decimation", 0, b"decimation"), ("decimation", 1, b"decimation"), ("decimation", 65, b"decimation"),
    ("filter_order", 1, b"filter_order"), ("filter_order", 1025, b"filter_order"),
    ("cutoff", -0.1, b"cutoff"), ("cutoff", 0.51, b"cutoff"), ("cutoff", float("nan"), b"cutoff"),
    ("table_size", 1025, b"table_size"),
    ("out_scale", float("inf"), b"out_scale"), ("out_scale", float("nan"), b"out_scale")])
def test_invalid_parameters_are_refused_with_a_sentence(pkg, field, value, word):
    assert _create(pkg, _params(pkg, **{field: value})) == FMD_ERR_ARG
    msg = pkg.lib().fmd_last_error()
    assert word in msg and len(msg.split()) >= 5, msg


def test_invalid_geometry_is_refused_with_a_sentence(pkg):
    lib = pkg.lib()
    assert _create(pkg, _params(pkg), n_captures=0) == FMD_ERR_ARG
    assert b"n_captures" in lib.fmd_last_error()
    assert _create(pkg, _params(pkg), n_bands=0) == FMD_ERR_ARG
    assert b"n_bands" in lib.fmd_last_error()


def test_python_layer_refuses_shifts_that_do_not_fill_the_rows(pkg):
    from importlib import import_module
    split = import_module(pkg.__name__ + ".split")
    with pytest.raises(pkg.FmdError, match="fmd error -1"):
        split.Splitter(9.6e6, 4, 2, [1, 2, 3])
    with pytest.raises(pkg.FmdError, match="decimation"):
        split.Splitter(9.6e6, 1, 1, [1, 2])


def test_create_without_a_gpu_fails_loudly(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the no-GPU path cannot be observed here")
    assert _create(pkg, _params(pkg)) == FMD_ERR_DEVICE
    assert b"no HIP device" in pkg.lib().fmd_last_error()
