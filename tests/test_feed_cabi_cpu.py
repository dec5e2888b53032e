"""CPU-only checks of the mono feed of the C ABI (include/fmd.h, FMD_FEED_* and the _feed entry points): the exports
exist, are declared and bound; and every refusal that needs no batch -- feed format, divisor, alignment, stride
multiple, null object -- returns its code and a sentence before the HIP runtime is touched (this file runs without a
GPU).  The refusals that need a live batch (a feed pointer while the feed is off, a stride below the call's count) are
in tests/test_gpu_feed.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package

FMD_ERR_ARG = -1
SYMBOLS = ("fmd_batch_set_feed", "fmd_batch_get_feed", "fmd_batch_feed_rate", "fmd_batch_max_feed_samples",
           "fmd_batch_get_feed_taps", "fmd_batch_process_device_feed", "fmd_batch_process_host_feed",
           "fmd_process_stream_feed", "fmd_batch_select_feed", "fmd_batch_get_feed_selection",
           "fmd_batch_debug_feed_skip_roll")
PROCESS = ("fmd_batch_process_device_feed", "fmd_batch_process_host_feed", "fmd_process_stream_feed")


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def _aligned(nbytes, offset=0):
    """(keep-alive, address): a host buffer whose address is 16-byte aligned plus `offset`"""
    raw = np.zeros(nbytes + 64, np.uint8)
    base = (raw.ctypes.data + 15) // 16 * 16
    return raw, base + offset


def _calls(lib, handle, iq_fmt, pcm_fmt, mpx_fmt, feed_fmt, feed_ptr, feed_stride=1024):
    """every _feed entry point with `handle` as its object; the other arguments are valid"""
    buf = np.zeros(4096, np.float32)
    out = np.zeros(8192, np.float32)
    nf, nm, nfeed = C.c_uint(), C.c_uint(), C.c_uint(77)
    p, o = buf.ctypes.data, out.ctypes.data
    return {
        "fmd_batch_process_device_feed": lambda: (lib.fmd_batch_process_device_feed(
            handle, p, iq_fmt, 0, 1024, o, pcm_fmt, 0, C.byref(nf), None, mpx_fmt, 0, C.byref(nm), feed_ptr, feed_fmt,
            feed_stride, C.byref(nfeed), None), nfeed.value),
        "fmd_batch_process_host_feed": lambda: (lib.fmd_batch_process_host_feed(
            handle, p, iq_fmt, 0, 1024, o, pcm_fmt, 0, C.byref(nf), None, mpx_fmt, 0, C.byref(nm), feed_ptr, feed_fmt,
            feed_stride, C.byref(nfeed)), nfeed.value),
        "fmd_process_stream_feed": lambda: (lib.fmd_process_stream_feed(
            handle, p, iq_fmt, 1024, o, pcm_fmt, feed_ptr, feed_fmt, C.byref(nfeed)), nfeed.value),
    }


def test_feed_symbols_are_exported_declared_and_bound(pkg):
    lib = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "fmd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in pkg.EXPORTS
        assert getattr(lib, name).argtypes is not None, name
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared in include/fmd.h"
    assert re.search(r"#define\s+FMD_FEED_F32\s+0\b", code) and re.search(r"#define\s+FMD_FEED_S16\s+1\b", code)
    assert (pkg.FMD_FEED_F32, pkg.FMD_FEED_S16) == (0, 1)
    assert pkg.FEED_BYTES == {0: 4, 1: 2}
    for name in ("set_feed", "select_feed", "feed_selection", "max_feed_samples", "feed_rate", "feed_taps"):
        assert hasattr(pkg.Batch, name)
    for name in ("SetFeed", "ProcessStreamWithFeed"):
        assert hasattr(pkg.FmDecoder, name)
        assert name in open(os.path.join(ROOT, "include", "fm_decoder.hpp")).read()
    # the header says what a call without the feed is, and that the setup call waits
    assert "SPLICE" in hdr and "WAITS for the calls in flight" in hdr


@pytest.mark.parametrize("iq,pcm,mpx", [(0, 0, 0), (-1, 0, 0), (4, 2, 5), (0, -1, 2)])
@pytest.mark.parametrize("feed", [-1, 2])
@pytest.mark.parametrize("name", PROCESS)
def test_feed_format_outside_the_enum_is_refused_first(pkg, name, feed, iq, pcm, mpx):
    lib = pkg.lib()
    keep, ptr = _aligned(4096)
    for fp in (ptr, None):
        rc, _ = _calls(lib, None, iq, pcm, mpx, feed, fp)[name]()
        assert rc == FMD_ERR_ARG
        msg = lib.fmd_last_error()
        assert name.encode() in msg and b"format" in msg and b"FMD_FEED" in msg, msg


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("name", PROCESS)
def test_null_object_is_refused(pkg, name, fmt):
    lib = pkg.lib()
    keep, ptr = _aligned(4096)
    for fp in (ptr, None):
        rc, nfeed = _calls(lib, None, 0, 0, 0, fmt, fp)[name]()
        assert rc == FMD_ERR_ARG
        assert b"null" in lib.fmd_last_error()
        assert nfeed == 0  # (the count is cleared even for a refused call)


@pytest.mark.parametrize("fmt,offset,stride", [(0, 4, 1024), (1, 2, 1024), (0, 8, 1024), (1, 8, 1024), (0, 0, 1022),
                                               (1, 0, 1028), (1, 0, 1022), (0, 0, 1023)])
def test_device_rows_have_to_be_aligned(pkg, fmt, offset, stride):
    """pointer off a 16-byte boundary, or a stride that is no multiple of 4 (float) / 8 (int16) elements: refused by
    the device entry point before it looks at the batch"""
    lib = pkg.lib()
    keep, ptr = _aligned(4096, offset)
    rc, nfeed = _calls(lib, None, 0, 0, 0, fmt, ptr, stride)["fmd_batch_process_device_feed"]()
    assert rc == FMD_ERR_ARG and nfeed == 0
    msg = lib.fmd_last_error()
    assert b"16-byte aligned" in msg and b"feed_channel_stride" in msg, msg


@pytest.mark.parametrize("divisor", [-1, 1, 4, 5, 6, 48])
def test_other_divisors_are_refused(pkg, divisor):
    lib = pkg.lib()
    assert lib.fmd_batch_set_feed(None, divisor) == FMD_ERR_ARG
    msg = lib.fmd_last_error()
    assert b"divisor" in msg and b"2 or 3" in msg, msg


def test_setup_and_getters_of_no_batch(pkg):
    lib = pkg.lib()
    for d in (0, 2, 3):
        assert lib.fmd_batch_set_feed(None, d) == FMD_ERR_ARG
        assert b"null" in lib.fmd_last_error()
    assert lib.fmd_batch_get_feed(None) == FMD_ERR_ARG
    assert lib.fmd_batch_feed_rate(None) == 0.0
    assert lib.fmd_batch_max_feed_samples(None, 65536) == 0
    assert lib.fmd_batch_get_feed_taps(None, None, 0) == FMD_ERR_ARG
    assert lib.fmd_batch_select_feed(None, None, 0) == FMD_ERR_ARG
    assert lib.fmd_batch_get_feed_selection(None, None, 0) == FMD_ERR_ARG
    assert lib.fmd_batch_debug_feed_skip_roll(None, 1) == FMD_ERR_ARG


def test_python_layer_refuses_other_feed_dtypes(pkg):
    assert pkg.feed_format_of(np.float32) == pkg.FMD_FEED_F32
    assert pkg.feed_format_of(np.int16) == pkg.FMD_FEED_S16
    assert pkg.feed_format_of(pkg.FMD_FEED_S16) == pkg.FMD_FEED_S16
    for dt in (np.float64, np.uint8, np.int32, 2, -1, True, "pcm"):
        with pytest.raises(pkg.FmdError):
            pkg.feed_format_of(dt)
