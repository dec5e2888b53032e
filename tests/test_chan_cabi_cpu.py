"""CPU-only checks of the polyphase channeliser's C ABI (include/fmd.h, fmd_chan_*): the entry points are exported,
declared and bound; bad arguments are refused with FMD_ERR_ARG and a sentence naming the field before the HIP runtime
is touched (FMD_REAL_* and FMD_IN_CIQ_* input with a sentence of their own, a geometry that does not fit LDS at
create); the zero-means-default rules are the header's; and without a GPU fmd_chan_create fails loudly (no CPU
fallback)."""
import ctypes as C
import os
import re
from importlib import import_module

import numpy as np
import pytest

from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMD_ERR_ARG, FMD_ERR_DEVICE = -1, -2
SYMBOLS = ("fmd_chan_create", "fmd_chan_destroy", "fmd_chan_reset", "fmd_chan_set_shifts", "fmd_chan_rows",
           "fmd_chan_out_rate", "fmd_chan_max_out_samples", "fmd_chan_get_taps", "fmd_chan_tile_samples",
           "fmd_chan_process_device", "fmd_chan_process_host")


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def _params(pkg, **kw):
    p = pkg.FmdChanParams(9.6e6, 96, 44, 0, 0.0, 0.0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _create(pkg, p, n_captures=1, n_rows=2, shifts=(1, -1)):
    h = C.c_void_p()
    sh = np.asarray(shifts, np.int32)
    return pkg.lib().fmd_chan_create(C.byref(p), n_captures, n_rows, sh.ctypes.data, 0, C.byref(h))


def test_chan_symbols_are_exported_declared_and_bound(pkg):
    lib = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "fmd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in pkg.EXPORTS
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared in include/fmd.h"
    assert re.search(r"#define\s+FMD_CHAN_MAX_SAMPLES\s+16777216u", code)
    chan = import_module(pkg.__name__ + ".chan")
    assert hasattr(chan, "Channeliser") and hasattr(chan, "plan_bins")
    for m in ("process", "process_host", "set_shifts", "reset", "taps", "max_out_samples", "out_stride", "close"):
        assert callable(getattr(chan.Channeliser, m)), m
    assert C.sizeof(pkg.FmdChanParams) == 40


def test_the_header_says_what_is_not_offered():
    hdr = open(os.path.join(ROOT, "include", "fmd.h")).read()
    sect = hdr[hdr.index("polyphase channeliser: a wideband"):hdr.index("host-only pieces")]
    line = sect[sect.index("Not offered"):]
    for word in ("real-sampled input", "int16 rows", "saving a channeliser's state", "N above 256"):
        assert word in line, word


def test_null_arguments_are_refused(pkg):
    lib = pkg.lib()
    h = C.c_void_p()
    sh = np.zeros(2, np.int32)
    assert lib.fmd_chan_create(None, 1, 2, sh.ctypes.data, 0, C.byref(h)) == FMD_ERR_ARG
    assert b"null" in lib.fmd_last_error()
    assert lib.fmd_chan_create(C.byref(_params(pkg)), 1, 2, None, 0, C.byref(h)) == FMD_ERR_ARG
    assert b"null" in lib.fmd_last_error()
    assert lib.fmd_chan_create(C.byref(_params(pkg)), 1, 2, sh.ctypes.data, 0, None) == FMD_ERR_ARG
    assert b"null" in lib.fmd_last_error()
    buf = np.zeros(4096, np.float32)
    n = C.c_uint()
    for rc in (lib.fmd_chan_reset(None, None), lib.fmd_chan_set_shifts(None, sh.ctypes.data, 2),
               lib.fmd_chan_rows(None), lib.fmd_chan_get_taps(None, buf.ctypes.data, 16),
               lib.fmd_chan_process_device(None, buf.ctypes.data, 0, 0, 1024, buf.ctypes.data, 512, C.byref(n), None),
               lib.fmd_chan_process_host(None, buf.ctypes.data, 0, 0, 1024, buf.ctypes.data, 512, C.byref(n))):
        assert rc == FMD_ERR_ARG
        assert b"null" in lib.fmd_last_error()
    assert lib.fmd_chan_out_rate(None) == 0.0 and b"null" in lib.fmd_last_error()
    assert lib.fmd_chan_max_out_samples(None, 16) == 0 and b"null" in lib.fmd_last_error()
    assert lib.fmd_chan_tile_samples(None) == 0 and b"null" in lib.fmd_last_error()
    lib.fmd_chan_destroy(None)  # a no-op


@pytest.mark.parametrize("fmt,word", [(-1, b"iq_format"), (4, b"iq_format"), (99, b"iq_format"),
                                      (16, b"FMD_REAL"), (18, b"FMD_REAL"), (19, b"FMD_REAL"),
                                      (32, b"FMD_IN_CIQ"), (33, b"FMD_IN_CIQ")])
def test_a_format_outside_fmd_iq_is_refused_before_anything_else(pkg, fmt, word):
    lib = pkg.lib()
    buf = np.zeros(64, np.float32)
    for rc in (lib.fmd_chan_process_device(None, buf.ctypes.data, fmt, 0, 16, buf.ctypes.data, 8, None, None),
               lib.fmd_chan_process_host(None, buf.ctypes.data, fmt, 0, 16, buf.ctypes.data, 8, None)):
        assert rc == FMD_ERR_ARG
        msg = lib.fmd_last_error()
        assert word in msg and b"iq_format must be one of FMD_IQ_F32" in msg and len(msg.split()) >= 5, msg


@pytest.mark.parametrize("field,value,word", [
    ("sample_rate_in", 0.0, b"sample_rate_in"), ("sample_rate_in", -1.0, b"sample_rate_in"),
    ("sample_rate_in", float("nan"), b"sample_rate_in"),
    ("n_bins", 0, b"n_bins"), ("n_bins", 1, b"n_bins"), ("n_bins", 257, b"n_bins"),
    ("decimation", 0, b"decimation"), ("decimation", 1, b"decimation"), ("decimation", 257, b"decimation"),
    ("filter_order", 1, b"filter_order"), ("filter_order", 4097, b"filter_order"),
    ("cutoff", -0.1, b"cutoff"), ("cutoff", 0.51, b"cutoff"), ("cutoff", float("nan"), b"cutoff"),
    ("out_scale", float("inf"), b"out_scale"), ("out_scale", float("nan"), b"out_scale")])
def test_invalid_parameters_are_refused_with_a_sentence(pkg, field, value, word):
    assert _create(pkg, _params(pkg, **{field: value})) == FMD_ERR_ARG
    msg = pkg.lib().fmd_last_error()
    assert word in msg and len(msg.split()) >= 5, msg


def test_invalid_geometry_is_refused_with_a_sentence(pkg):
    lib = pkg.lib()
    assert _create(pkg, _params(pkg), n_captures=0) == FMD_ERR_ARG
    assert b"n_captures" in lib.fmd_last_error()
    assert _create(pkg, _params(pkg), n_rows=0) == FMD_ERR_ARG
    assert b"n_rows_per_capture" in lib.fmd_last_error()


def test_a_window_that_does_not_fit_lds_is_refused_at_create(pkg):
    """31 D + K window samples and N x 32 branch sums above a workgroup's LDS: a sentence, before any device call"""
    assert _create(pkg, _params(pkg, n_bins=256, decimation=256, filter_order=4096)) == FMD_ERR_ARG
    msg = pkg.lib().fmd_last_error()
    assert b"LDS" in msg and b"filter_order" in msg and b"n_bins" in msg, msg


def test_defaults_reach_past_the_parameter_checks(pkg):
    """filter_order 0 = 8 D must pass where 8 D is in range and be refused where it is not (D 256 gives 2048: fine;
    there is no D whose default order is out of range), cutoff 0 = 0.6 / D, out_scale 0 = 1.0: all zeros get as far as
    the device question."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the defaults are checked on the device (tests/test_gpu_chan.py)")
    for D in (2, 44, 256):
        assert _create(pkg, _params(pkg, n_bins=16, decimation=D)) == FMD_ERR_DEVICE


def test_python_layer_refuses_shifts_that_do_not_fill_the_rows(pkg):
    chan = import_module(pkg.__name__ + ".chan")
    with pytest.raises(pkg.FmdError, match="fmd error -1"):
        chan.Channeliser(9.6e6, 96, 44, 2, [1, 2, 3])
    with pytest.raises(pkg.FmdError, match="decimation"):
        chan.Channeliser(9.6e6, 96, 1, 1, [1, 2])
    with pytest.raises(pkg.FmdError, match="n_bins"):
        chan.Channeliser(9.6e6, 300, 44, 1, [1, 2])


def test_create_without_a_gpu_fails_loudly(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the no-GPU path cannot be observed here")
    assert _create(pkg, _params(pkg)) == FMD_ERR_DEVICE
    assert b"no HIP device" in pkg.lib().fmd_last_error()
