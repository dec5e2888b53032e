"""CPU-only checks of channel IQ rows as a call's input (include/fmd.h, FMD_IN_CIQ_*): the exports and constants
exist, are declared and bound; formats 32 / 33 are refused with a sentence by every entry point that is not one of the
three _call entry points -- positional batch and decoder calls, receiver, scan, splitter -- before the HIP runtime is
touched (this file runs without a GPU); the _call entry points take them past the format check and refuse a null
object and a row stride below the call's length; FMD_IN_CIQ_S16's conversion equals numpy's over all 65 536 values;
the Python layer picks the format by dtype and refuses everything else.  What needs a device is in
tests/test_gpu_ciq_in.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package

FMD_OK, FMD_ERR_ARG = 0, -1
IN_FORMATS = (32, 33)
SYMBOLS = ("fmd_batch_baseband_limits", "fmd_batch_debug_ciq_in_skip_tile", "fmd_debug_ciq16_to_f32",
           "fmd_batch_process_device_call", "fmd_batch_process_host_call", "fmd_process_stream_call")


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def _positional(lib, fmt):
    """every entry point that takes an input format and is not a _call entry point, with a null object and otherwise
    valid arguments: name -> () -> return code"""
    buf = np.zeros(8192, np.float32)
    out = np.zeros(16384, np.float32)
    nf, nm, nfeed = C.c_uint(), C.c_uint(), C.c_uint()
    p, o = buf.ctypes.data, out.ctypes.data
    return {
        "fmd_batch_process_device_fmt": lambda: lib.fmd_batch_process_device_fmt(None, p, fmt, 0, 1024, o, 0,
                                                                                 C.byref(nf), None),
        "fmd_batch_process_device_pcm": lambda: lib.fmd_batch_process_device_pcm(None, p, fmt, 0, 1024, o, 0, 0,
                                                                                 C.byref(nf), None),
        "fmd_batch_process_device_mpx": lambda: lib.fmd_batch_process_device_mpx(
            None, p, fmt, 0, 1024, o, 0, 0, C.byref(nf), None, 0, 0, C.byref(nm), None),
        "fmd_batch_process_device_feed": lambda: lib.fmd_batch_process_device_feed(
            None, p, fmt, 0, 1024, o, 0, 0, C.byref(nf), None, 0, 0, C.byref(nm), None, 0, 0, C.byref(nfeed), None),
        "fmd_batch_process_host_fmt": lambda: lib.fmd_batch_process_host_fmt(None, p, fmt, 0, 1024, o, 0, C.byref(nf)),
        "fmd_batch_process_host_pcm": lambda: lib.fmd_batch_process_host_pcm(None, p, fmt, 0, 1024, o, 0, 0,
                                                                             C.byref(nf)),
        "fmd_batch_process_host_mpx": lambda: lib.fmd_batch_process_host_mpx(
            None, p, fmt, 0, 1024, o, 0, 0, C.byref(nf), None, 0, 0, C.byref(nm)),
        "fmd_batch_process_host_feed": lambda: lib.fmd_batch_process_host_feed(
            None, p, fmt, 0, 1024, o, 0, 0, C.byref(nf), None, 0, 0, C.byref(nm), None, 0, 0, C.byref(nfeed)),
        "fmd_process_stream_fmt": lambda: lib.fmd_process_stream_fmt(None, p, fmt, 1024, o),
        "fmd_process_stream_pcm": lambda: lib.fmd_process_stream_pcm(None, p, fmt, 1024, o, 0),
        "fmd_process_stream_mpx": lambda: lib.fmd_process_stream_mpx(None, p, fmt, 1024, o, 0, None, 0, C.byref(nm)),
        "fmd_process_stream_feed": lambda: lib.fmd_process_stream_feed(None, p, fmt, 1024, o, 0, None, 0,
                                                                       C.byref(nfeed)),
        "fmd_receiver_write_fmt": lambda: lib.fmd_receiver_write_fmt(None, p, fmt, 1024),
        "fmd_scan_accumulate_device_fmt": lambda: lib.fmd_scan_accumulate_device_fmt(None, p, fmt, 0, 1024, None),
        "fmd_scan_accumulate_host_fmt": lambda: lib.fmd_scan_accumulate_host_fmt(None, p, fmt, 0, 1024),
        "fmd_split_process_device": lambda: lib.fmd_split_process_device(None, p, fmt, 0, 1024, o, 0, C.byref(nf), None),
        "fmd_split_process_host": lambda: lib.fmd_split_process_host(None, p, fmt, 0, 1024, o, 0, C.byref(nf)),
    }


POSITIONAL = sorted(_positional(None, 0))


def _record(pkg, fmt, rows=None, stride=0, m=1024, audio=None):
    rows = np.zeros(4096, np.float32) if rows is None else rows
    audio = np.zeros(16384, np.float32) if audio is None else audio
    return (rows, audio), pkg.make_call(rows.ctypes.data, fmt, stride, m, audio=pkg.make_rows(audio.ctypes.data, 0, 0))


def test_symbols_and_constants_are_exported_declared_and_bound(pkg):
    lib = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "fmd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in pkg.EXPORTS
        assert getattr(lib, name).argtypes is not None, name
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared in include/fmd.h"
    assert re.search(r"#define\s+FMD_IN_CIQ_F32\s+32\b", code) and re.search(r"#define\s+FMD_IN_CIQ_S16\s+33\b", code)
    assert (pkg.FMD_IN_CIQ_F32, pkg.FMD_IN_CIQ_S16) == (32, 33)
    assert pkg.IN_CIQ_BYTES == {32: 8, 33: 4}
    for name in ("baseband_limits", "process_call", "process_host_ciq_in"):
        assert hasattr(pkg.Batch, name)
    assert hasattr(pkg.FmDecoder, "ProcessChannelIq")
    cpp = open(os.path.join(ROOT, "include", "fm_decoder.hpp")).read()
    assert "ProcessChannelIq(const float* ciq, unsigned int m, float* audio)" in cpp
    assert "ProcessChannelIqWithMpx" in cpp and "ProcessChannelIqToPcm16" in cpp
    # the call record did not change: the formats are two more values of its iq_format
    assert C.sizeof(pkg.FmdCall) == 8 + 8 + 8 + 8 + 8 + 4 * 32 + 8
    # the header says what such a call leaves alone
    assert "interface_level" in hdr and "keeps the\n * value the last IQ call left" in hdr


@pytest.mark.parametrize("fmt", IN_FORMATS)
@pytest.mark.parametrize("name", POSITIONAL)
def test_every_other_entry_point_refuses_the_formats_with_a_sentence(pkg, name, fmt):
    """a null object everywhere: the format is looked at first, so the sentence is the format's -- and no device is
    needed to get it"""
    lib = pkg.lib()
    assert _positional(lib, fmt)[name]() == FMD_ERR_ARG
    msg = lib.fmd_last_error()
    assert b"format" in msg.lower() or b"FMD_IN_CIQ" in msg, msg
    assert b"null" not in msg, msg
    if name.startswith(("fmd_batch_process", "fmd_process_stream")) and not name.endswith("_fmt"):
        assert b"FMD_IN_CIQ" in msg and b"_call entry points only" in msg and name.encode() in msg, msg


@pytest.mark.parametrize("fmt", IN_FORMATS)
def test_call_entry_points_take_the_formats_up_to_the_object(pkg, fmt):
    """past the format check: what refuses these calls is the null batch / decoder"""
    lib = pkg.lib()
    keep, call = _record(pkg, fmt)
    for fn in (lib.fmd_batch_process_device_call, lib.fmd_batch_process_host_call, lib.fmd_process_stream_call):
        assert fn(None, C.byref(call)) == FMD_ERR_ARG
        msg = lib.fmd_last_error()
        assert b"null" in msg and b"format" not in msg, msg
    # a value that is neither kind of format names both in its refusal
    for bad in (4, 31, 34, 16, -1):
        keep, call = _record(pkg, bad)
        assert lib.fmd_batch_process_host_call(None, C.byref(call)) == FMD_ERR_ARG
        msg = lib.fmd_last_error()
        assert b"FMD_IQ_F32" in msg and b"FMD_IN_CIQ_F32" in msg, msg


@pytest.mark.parametrize("fmt,offset,stride", [(32, 8, 1024), (32, 4, 1024), (33, 4, 1024), (33, 8, 1024),
                                               (32, 0, 1025), (33, 0, 1026), (33, 0, 1025), (33, 0, 1027)])
def test_device_rows_have_to_be_aligned(pkg, fmt, offset, stride):
    """a pointer off a 16-byte boundary, or a stride that is no multiple of 2 (float pairs) / 4 (int16 pairs) complex
    samples: refused by the device entry point before it looks at the batch -- the rule of the ciq output's rows"""
    lib = pkg.lib()
    raw = np.zeros(8192 + 64, np.uint8)
    ptr = (raw.ctypes.data + 15) // 16 * 16 + offset
    audio = np.zeros(64, np.float32)
    call = pkg.make_call(ptr, fmt, stride, 1024, audio=pkg.make_rows(audio.ctypes.data, 0, 0))
    assert lib.fmd_batch_process_device_call(None, C.byref(call)) == FMD_ERR_ARG
    msg = lib.fmd_last_error()
    assert b"16-byte aligned" in msg and b"iq_channel_stride" in msg and b"fmd_batch_process_device_call" in msg, msg
    # the host call and the decoder take any alignment and stride: what refuses them here is the null object
    for fn in (lib.fmd_batch_process_host_call, lib.fmd_process_stream_call):
        assert fn(None, C.byref(call)) == FMD_ERR_ARG
        assert b"null" in lib.fmd_last_error()


def test_getters_of_no_batch(pkg):
    lib = pkg.lib()
    lo = C.c_uint(7)
    assert lib.fmd_batch_baseband_limits(None, C.byref(lo), None, None) == FMD_ERR_ARG
    assert b"null" in lib.fmd_last_error() and lo.value == 7
    assert lib.fmd_batch_debug_ciq_in_skip_tile(None, 1) == FMD_ERR_ARG
    assert lib.fmd_debug_ciq16_to_f32(None, 4, None) == FMD_ERR_ARG


def test_s16_conversion_over_all_values_is_numpys(pkg):
    """(float)v * 2^-13 of every int16: exact, and the inverse scale of FMD_CIQ_S16 -- converting back gives v"""
    from test_mpx_cabi_cpu import mpx16
    v = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    out = np.full(v.size, np.nan, np.float32)
    assert pkg.lib().fmd_debug_ciq16_to_f32(v.ctypes.data, v.size, out.ctypes.data) == FMD_OK
    want = v.astype(np.float32) * np.float32(2.0 ** -13)
    assert out.tobytes() == want.tobytes()
    assert np.array_equal(want.astype(np.float64) * 8192.0, v.astype(np.float64))  # exact in float
    assert np.array_equal(mpx16(out), v)  # FMD_CIQ_S16 of the converted row is the row


def test_python_layer_picks_the_format_by_dtype(pkg):
    f32 = np.zeros((3, 40), np.complex64)
    s16 = np.zeros((3, 44, 2), np.int16)
    assert pkg.ciq_in_of(f32) == (f32.ctypes.data, pkg.FMD_IN_CIQ_F32, 40, 40)
    assert pkg.ciq_in_of(s16) == (s16.ctypes.data, pkg.FMD_IN_CIQ_S16, 44, 44)
    assert pkg.ciq_in_of(f32[:, :33]) == (f32.ctypes.data, pkg.FMD_IN_CIQ_F32, 40, 33)  # a stride of its own
    assert pkg.ciq_in_of(s16[1, :9]) == (s16[1].ctypes.data, pkg.FMD_IN_CIQ_S16, 0, 9)  # one row
    call = pkg.make_call(ciq_in=s16[:, :21])
    assert (call.iq, call.iq_format, call.iq_channel_stride, call.samples) == (s16.ctypes.data, 33, 44, 21)
    assert call.size == C.sizeof(pkg.FmdCall)
    for bad in (np.zeros((3, 40), np.complex128), np.zeros((3, 40), np.float32), np.zeros((3, 40), np.int16),
                np.zeros((3, 40, 2), np.int8), f32[:, ::2], np.zeros((2, 3, 40), np.complex64)):
        with pytest.raises(pkg.FmdError):
            pkg.ciq_in_of(bad)
    with pytest.raises(pkg.FmdError, match="not both"):
        pkg.make_call(f32.ctypes.data, 0, 0, 40, ciq_in=f32)
    try:
        import torch
    except ImportError:
        return
    t = torch.zeros((2, 24), dtype=torch.complex64)
    assert pkg.ciq_in_of(t) == (t.data_ptr(), pkg.FMD_IN_CIQ_F32, 24, 24)
    t = torch.zeros((2, 24, 2), dtype=torch.int16)
    assert pkg.ciq_in_of(t) == (t.data_ptr(), pkg.FMD_IN_CIQ_S16, 24, 24)
    with pytest.raises(pkg.FmdError):
        pkg.ciq_in_of(torch.zeros((2, 24), dtype=torch.float32))
