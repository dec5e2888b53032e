"""CPU-only checks of the real-sampled channeliser's and the int16 rows' C ABI (include/fmd.h: fmd_chan_create_real,
fmd_chan_process_device_fmt, fmd_chan_process_host_fmt): exported, declared and bound; null arguments, parameters out
of range (n_bins up to 512 for a real channeliser) and an out_format outside FMD_CIQ_* are refused with FMD_ERR_ARG and
a sentence before the HIP runtime is touched; without a GPU the create fails loudly."""
import ctypes as C
import os
import re
from importlib import import_module

import numpy as np
import pytest

from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMD_ERR_ARG, FMD_ERR_DEVICE = -1, -2
SYMBOLS = ("fmd_chan_create_real", "fmd_chan_process_device_fmt", "fmd_chan_process_host_fmt")


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def _params(pkg, **kw):
    p = pkg.FmdChanParams(51.2e6, 512, 235, 0, 0.0, 0.0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _create_real(pkg, p, n_captures=1, n_rows=2, shifts=(1, -1)):
    h = C.c_void_p()
    sh = np.asarray(shifts, np.int32)
    rc = pkg.lib().fmd_chan_create_real(C.byref(p), n_captures, n_rows, sh.ctypes.data, 0, C.byref(h))
    assert rc != 0 or h.value
    if rc == 0:
        pkg.lib().fmd_chan_destroy(h)
    return rc


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_symbols_are_exported_declared_and_bound(pkg):
    lib = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "fmd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in pkg.EXPORTS
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared in include/fmd.h"
    assert C.sizeof(pkg.FmdChanParams) == 40
    chan = import_module(pkg.__name__ + ".chan")
    assert callable(chan.plan_bins_real)
    assert chan.rows_format_of(None) == 0 == chan.rows_format_of(np.complex64) and chan.rows_format_of(np.int16) == 1
    with pytest.raises(pkg.FmdError, match="row format"):
        chan.rows_format_of(np.float32)


def test_the_header_states_the_contract_and_what_is_still_not_offered():
    hdr = open(os.path.join(ROOT, "include", "fmd.h")).read()
    sect = hdr[hdr.index("polyphase channeliser: a wideband"):hdr.index("host-only pieces")]
    new = sect[sect.index("Real-sampled captures (fmd_chan_create_real)"):]
    for word in ("bit for bit", "compare zeros with ==", "257..512", "fmd_f32_to_mpx16", "multiple of 4"):
        assert word in new, word
    last = new[new.index("Still not offered"):].split("*/")[0]
    for word in ("unsigned real samples", "saving a channeliser's state", "N above 256 for complex input",
                 "N above 512"):
        assert word in last, word


def test_null_arguments_are_refused(pkg):
    lib = pkg.lib()
    h = C.c_void_p()
    sh = np.zeros(2, np.int32)
    assert lib.fmd_chan_create_real(None, 1, 2, sh.ctypes.data, 0, C.byref(h)) == FMD_ERR_ARG
    assert b"null" in lib.fmd_last_error() and b"fmd_chan_create_real" in lib.fmd_last_error()
    assert lib.fmd_chan_create_real(C.byref(_params(pkg)), 1, 2, None, 0, C.byref(h)) == FMD_ERR_ARG
    assert b"null" in lib.fmd_last_error()
    assert lib.fmd_chan_create_real(C.byref(_params(pkg)), 1, 2, sh.ctypes.data, 0, None) == FMD_ERR_ARG
    assert b"null" in lib.fmd_last_error()
    buf = np.zeros(4096, np.float32)
    n = C.c_uint(77)
    for fmt in (0, 3):
        for ofmt in (0, 1):
            for rc in (lib.fmd_chan_process_device_fmt(None, buf.ctypes.data, fmt, 0, 1024, buf.ctypes.data, ofmt, 512,
                                                       C.byref(n), None),
                       lib.fmd_chan_process_host_fmt(None, buf.ctypes.data, fmt, 0, 1024, buf.ctypes.data, ofmt, 512,
                                                     C.byref(n))):
                assert rc == FMD_ERR_ARG
                assert b"null" in lib.fmd_last_error()
    assert n.value == 77


@pytest.mark.parametrize("fmt,word", [(-1, b"iq_format"), (4, b"iq_format"), (17, b"iq_format"), (99, b"iq_format"),
                                      (16, b"FMD_REAL"), (18, b"FMD_REAL"), (19, b"FMD_REAL"),
                                      (32, b"FMD_IN_CIQ"), (33, b"FMD_IN_CIQ")])
def test_the_fmt_entry_points_refuse_formats_like_the_old_ones_with_a_null_handle(pkg, fmt, word):
    """no channeliser, so no kind: FMD_REAL_* is refused with the old entry points' sentence"""
    lib = pkg.lib()
    buf = np.zeros(64, np.float32)
    for rc in (lib.fmd_chan_process_device_fmt(None, buf.ctypes.data, fmt, 0, 16, buf.ctypes.data, 0, 8, None, None),
               lib.fmd_chan_process_host_fmt(None, buf.ctypes.data, fmt, 0, 16, buf.ctypes.data, 1, 8, None)):
        assert rc == FMD_ERR_ARG
        msg = lib.fmd_last_error()
        assert word in msg and b"iq_format must be one of FMD_IQ_F32" in msg and len(msg.split()) >= 5, msg


@pytest.mark.parametrize("ofmt", [-1, 2, 16, 32, 33, 99])
def test_an_out_format_outside_fmd_ciq_gets_a_sentence(pkg, ofmt):
    lib = pkg.lib()
    buf = np.zeros(64, np.float32)
    for rc in (lib.fmd_chan_process_device_fmt(None, buf.ctypes.data, 0, 0, 16, buf.ctypes.data, ofmt, 8, None, None),
               lib.fmd_chan_process_host_fmt(None, buf.ctypes.data, 0, 0, 16, buf.ctypes.data, ofmt, 8, None)):
        assert rc == FMD_ERR_ARG
        msg = lib.fmd_last_error()
        assert b"out_format must be FMD_CIQ_F32 or FMD_CIQ_S16" in msg and len(msg.split()) >= 5, msg


@pytest.mark.parametrize("field,value,word", [
    ("sample_rate_in", 0.0, b"sample_rate_in"), ("sample_rate_in", float("nan"), b"sample_rate_in"),
    ("n_bins", 0, b"n_bins"), ("n_bins", 1, b"n_bins"), ("n_bins", 513, b"n_bins"), ("n_bins", 1024, b"n_bins"),
    ("decimation", 1, b"decimation"), ("decimation", 257, b"decimation"),
    ("filter_order", 1, b"filter_order"), ("filter_order", 4097, b"filter_order"),
    ("cutoff", 0.51, b"cutoff"), ("out_scale", float("inf"), b"out_scale")])
def test_invalid_parameters_are_refused_with_a_sentence(pkg, field, value, word):
    assert _create_real(pkg, _params(pkg, **{field: value})) == FMD_ERR_ARG
    msg = pkg.lib().fmd_last_error()
    assert word in msg and b"fmd_chan_create_real" in msg and len(msg.split()) >= 5, msg
    if field == "n_bins":
        assert b"512" in msg


def test_invalid_geometry_is_refused_with_a_sentence(pkg):
    lib = pkg.lib()
    assert _create_real(pkg, _params(pkg), n_captures=0) == FMD_ERR_ARG
    assert b"n_captures" in lib.fmd_last_error()
    assert _create_real(pkg, _params(pkg), n_rows=0) == FMD_ERR_ARG
    assert b"n_rows_per_capture" in lib.fmd_last_error()


@pytest.mark.parametrize("n_bins", [257, 500, 512])
def test_n_bins_above_256_passes_the_parameter_checks_of_a_real_channeliser_only(pkg, n_bins):
    """257 .. 512 are not refused for n_bins -- nor for anything else in front of the device question --, while
    fmd_chan_create still refuses them"""
    rc = _create_real(pkg, _params(pkg, n_bins=n_bins))
    msg = pkg.lib().fmd_last_error()
    if _no_gpu():
        assert rc == FMD_ERR_DEVICE and b"no HIP device" in msg, msg
    else:
        assert rc == 0, msg
    h = C.c_void_p()
    sh = np.zeros(2, np.int32)
    p = _params(pkg, n_bins=n_bins)
    assert pkg.lib().fmd_chan_create(C.byref(p), 1, 2, sh.ctypes.data, 0, C.byref(h)) == FMD_ERR_ARG
    assert b"n_bins must be 2 .. 256" in pkg.lib().fmd_last_error()


def test_the_lds_check_of_a_real_geometry(pkg):
    """A real tile holds one float a window sample and one plane of branch sums: the largest geometry the parameter
    ranges admit -- N 512, D 256, K 4096: 48 KB of window, 16 KB of taps, 68 KB of branch sums -- fits the 160 KB of a
    workgroup, so no real geometry is refused for LDS, while the same D and K are refused for a complex channeliser
    already at N 256.  (The check and its sentence are shared by both kinds.)"""
    rc = _create_real(pkg, _params(pkg, n_bins=512, decimation=256, filter_order=4096))
    msg = pkg.lib().fmd_last_error()
    if _no_gpu():
        assert rc == FMD_ERR_DEVICE and b"no HIP device" in msg, msg
    else:
        assert rc == 0, msg
    h = C.c_void_p()
    sh = np.zeros(2, np.int32)
    p = _params(pkg, n_bins=256, decimation=256, filter_order=4096)
    assert pkg.lib().fmd_chan_create(C.byref(p), 1, 2, sh.ctypes.data, 0, C.byref(h)) == FMD_ERR_ARG
    msg = pkg.lib().fmd_last_error()
    assert b"LDS" in msg and b"filter_order" in msg and b"n_bins" in msg, msg


def test_python_layer_of_a_real_channeliser(pkg):
    chan = import_module(pkg.__name__ + ".chan")
    with pytest.raises(pkg.FmdError, match="n_bins must be 2 .. 512"):
        chan.Channeliser(51.2e6, 513, 235, 1, [1, 2], real=True)
    with pytest.raises(pkg.FmdError, match="n_bins must be 2 .. 256"):
        chan.Channeliser(51.2e6, 512, 235, 1, [1, 2])
    with pytest.raises(pkg.FmdError, match="fmd error -1"):
        chan.Channeliser(9.6e6, 96, 44, 2, [1, 2, 3], real=True)


def test_create_real_without_a_gpu_fails_loudly(pkg):
    rc = _create_real(pkg, _params(pkg))
    if _no_gpu():
        assert rc == FMD_ERR_DEVICE
        assert b"no HIP device" in pkg.lib().fmd_last_error()
    else:
        assert rc == 0, pkg.lib().fmd_last_error()
