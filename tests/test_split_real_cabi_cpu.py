"""CPU-only checks of the real band splitter's C ABI (include/fmd.h, fmd_split_create_real and FMD_REAL_*): the
symbol is exported and bound, 16 / 18 / 19 get past the splitter's format check and nowhere else, 15 / 17 / 20 are no
formats, and fmd_split_create_real refuses what fmd_split_create refuses -- all before the HIP runtime is touched."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

from __graft_entry__ import load_package

FMD_ERR_ARG, FMD_ERR_DEVICE = -1, -2
REAL_FORMATS = (16, 18, 19)


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def _params(pkg, **kw):
    p = pkg.FmdSplitParams(19.2e6, 8, 0, 0.0, 0, 0.0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _create_real(pkg, p, n_captures=1, n_bands=2, shifts=(1, -1)):
    h = C.c_void_p()
    sh = np.asarray(shifts, np.int32)
    return pkg.lib().fmd_split_create_real(C.byref(p), n_captures, n_bands, sh.ctypes.data, 0, C.byref(h))


def test_the_symbol_and_the_constants_are_exported_and_bound(pkg):
    lib = pkg.lib()
    assert hasattr(lib, "fmd_split_create_real") and "fmd_split_create_real" in pkg.EXPORTS
    assert lib.fmd_split_create_real.argtypes is not None
    assert (pkg.FMD_REAL_F32, pkg.FMD_REAL_S8, pkg.FMD_REAL_S16) == REAL_FORMATS
    assert (pkg.FMD_REAL_F32, pkg.FMD_REAL_S8, pkg.FMD_REAL_S16) == (16 | pkg.FMD_IQ_F32, 16 | pkg.FMD_IQ_S8,
                                                                     16 | pkg.FMD_IQ_S16)
    split = import_module(pkg.__name__ + ".split")
    assert hasattr(split, "plan_bands_real")
    assert C.sizeof(pkg.FmdSplitParams) == 32   # the parameters did not grow


@pytest.mark.parametrize("fmt", REAL_FORMATS)
def test_real_formats_get_past_the_splitters_format_check(pkg, fmt):
    """with a null splitter the refusal names the null pointer, not the format"""
    lib = pkg.lib()
    buf = np.zeros(64, np.float32)
    for rc in (lib.fmd_split_process_device(None, buf.ctypes.data, fmt, 0, 16, buf.ctypes.data, 8, None, None),
               lib.fmd_split_process_host(None, buf.ctypes.data, fmt, 0, 16, buf.ctypes.data, 8, None)):
        assert rc == FMD_ERR_ARG
        msg = lib.fmd_last_error()
        assert b"null" in msg and b"iq_format" not in msg, msg


@pytest.mark.parametrize("fmt", [17, 20, 15])
def test_neighbours_of_the_real_formats_are_no_formats(pkg, fmt):
    lib = pkg.lib()
    buf = np.zeros(64, np.float32)
    assert lib.fmd_split_process_device(None, buf.ctypes.data, fmt, 0, 16, buf.ctypes.data, 8, None,
                                        None) == FMD_ERR_ARG
    msg = lib.fmd_last_error()
    assert b"fmd_split_process_device" in msg and b"iq_format" in msg and b"null" not in msg, msg
    assert lib.fmd_split_process_host(None, buf.ctypes.data, fmt, 0, 16, buf.ctypes.data, 8, None) == FMD_ERR_ARG
    msg = lib.fmd_last_error()
    assert b"fmd_split_process_host" in msg and b"iq_format" in msg and b"null" not in msg, msg


def _other_entry_points(lib, fmt):
    """every other entry point that takes an iq_format, with a null object and otherwise valid arguments"""
    buf = np.zeros(4096, np.float32)
    out = np.zeros(4096, np.float32)
    nf = C.c_uint()
    p, o = buf.ctypes.data, out.ctypes.data
    return {
        "fmd_batch_process_device_fmt": lambda: lib.fmd_batch_process_device_fmt(None, p, fmt, 0, 1024, o, 0,
                                                                                 C.byref(nf), None),
        "fmd_batch_process_host_fmt": lambda: lib.fmd_batch_process_host_fmt(None, p, fmt, 0, 1024, o, 0,
                                                                             C.byref(nf)),
        "fmd_process_stream_fmt": lambda: lib.fmd_process_stream_fmt(None, p, fmt, 1024, o),
        "fmd_receiver_write_fmt": lambda: lib.fmd_receiver_write_fmt(None, p, fmt, 1024),
        "fmd_scan_accumulate_device_fmt": lambda: lib.fmd_scan_accumulate_device_fmt(None, p, fmt, 0, 1024, None),
        "fmd_scan_accumulate_host_fmt": lambda: lib.fmd_scan_accumulate_host_fmt(None, p, fmt, 0, 1024),
    }


@pytest.mark.parametrize("fmt", REAL_FORMATS)
@pytest.mark.parametrize("name", ["fmd_batch_process_device_fmt", "fmd_batch_process_host_fmt",
                                  "fmd_process_stream_fmt", "fmd_receiver_write_fmt",
                                  "fmd_scan_accumulate_device_fmt", "fmd_scan_accumulate_host_fmt"])
def test_every_other_entry_point_refuses_the_real_formats_with_its_present_sentence(pkg, name, fmt):
    """the sentence is the one the entry point has for 4, a value that never was a format"""
    lib = pkg.lib()
    assert _other_entry_points(lib, 4)[name]() == FMD_ERR_ARG
    present = lib.fmd_last_error()
    assert name.encode() in present and b"format" in present
    assert _other_entry_points(lib, 0)[name]() == FMD_ERR_ARG   # (another refusal in between: a null object)
    assert lib.fmd_last_error() != present
    assert _other_entry_points(lib, fmt)[name]() == FMD_ERR_ARG
    assert lib.fmd_last_error() == present


def test_null_arguments_are_refused(pkg):
    lib = pkg.lib()
    h = C.c_void_p()
    sh = np.zeros(2, np.int32)
    for rc in (lib.fmd_split_create_real(None, 1, 2, sh.ctypes.data, 0, C.byref(h)),
               lib.fmd_split_create_real(C.byref(_params(pkg)), 1, 2, None, 0, C.byref(h))):
        assert rc == FMD_ERR_ARG
        msg = lib.fmd_last_error()
        assert b"fmd_split_create_real" in msg and b"null" in msg, msg
    assert lib.fmd_split_create_real(C.byref(_params(pkg)), 1, 2, sh.ctypes.data, 0, None) == FMD_ERR_ARG
    assert b"null" in lib.fmd_last_error()


@pytest.mark.parametrize("field,value,word", [
    ("sample_rate_in", 0.0, b"sample_rate_in"), ("sample_rate_in", -1.0, b"sample_rate_in"),
    ("sample_rate_in", float("nan"), b"sample_rate_in"),
    ("decimation", 0, b"decimation"), ("decimation", 1, b"decimation"), ("decimation", 65, b"decimation"),
    ("filter_order", 1, b"filter_order"), ("filter_order", 1025, b"filter_order"),
    ("cutoff", -0.1, b"cutoff"), ("cutoff", 0.51, b"cutoff"), ("cutoff", float("nan"), b"cutoff"),
    ("table_size", 1025, b"table_size"),
    ("out_scale", float("inf"), b"out_scale"), ("out_scale", float("nan"), b"out_scale")])
def test_create_real_refuses_what_create_refuses_with_a_sentence(pkg, field, value, word):
    assert _create_real(pkg, _params(pkg, **{field: value})) == FMD_ERR_ARG
    msg = pkg.lib().fmd_last_error()
    assert b"fmd_split_create_real" in msg and word in msg and len(msg.split()) >= 5, msg


def test_create_real_refuses_an_invalid_geometry(pkg):
    lib = pkg.lib()
    assert _create_real(pkg, _params(pkg), n_captures=0) == FMD_ERR_ARG
    assert b"n_captures" in lib.fmd_last_error()
    assert _create_real(pkg, _params(pkg), n_captures=65536) == FMD_ERR_ARG
    assert b"n_captures" in lib.fmd_last_error()
    assert _create_real(pkg, _params(pkg), n_bands=0) == FMD_ERR_ARG
    assert b"n_bands" in lib.fmd_last_error()


def test_python_layer_creates_the_kind_it_is_asked_for(pkg):
    split = import_module(pkg.__name__ + ".split")
    with pytest.raises(pkg.FmdError, match="fmd_split_create_real: decimation"):
        split.Splitter(19.2e6, 1, 1, [1, 2], real=True)
    with pytest.raises(pkg.FmdError, match="fmd_split_create: decimation"):
        split.Splitter(19.2e6, 1, 1, [1, 2])


def test_create_real_without_a_gpu_fails_loudly(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the no-GPU path cannot be observed here")
    assert _create_real(pkg, _params(pkg)) == FMD_ERR_DEVICE
    assert b"no HIP device" in pkg.lib().fmd_last_error()
