"""CPU-only checks of the input formats of the C ABI (include/fmd.h, FMD_IQ_* and the _fmt entry points): the six
entry points are exported and bound, a null batch / decoder / receiver / scan and a format outside 0..3 are refused
with FMD_ERR_ARG and a sentence before the HIP runtime is touched, and the two signed integer conversions of
csrc/fmd_math.h (host build of the source the GPU executes) give numpy's v.astype(float32) * 2**-15 | 2**-7, bit
for bit, over all 65 536 + 256 values."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from __graft_entry__ import PKG_DIR, ROOT, load_package

FMD_ERR_ARG = -1
SYMBOLS = ("fmd_batch_process_device_fmt", "fmd_batch_process_host_fmt", "fmd_process_stream_fmt",
           "fmd_receiver_write_fmt", "fmd_scan_accumulate_device_fmt", "fmd_scan_accumulate_host_fmt")


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def _calls(lib, handle, fmt):
    """every _fmt entry point with `handle` as its object and `fmt` as its format; the other arguments are valid"""
    buf = np.zeros(4096, np.float32)
    out = np.zeros(4096, np.float32)
    nf = C.c_uint()
    p, o = buf.ctypes.data, out.ctypes.data
    return {
        "fmd_batch_process_device_fmt": lambda: lib.fmd_batch_process_device_fmt(handle, p, fmt, 0, 1024, o, 0,
                                                                                 C.byref(nf), None),
        "fmd_batch_process_host_fmt": lambda: lib.fmd_batch_process_host_fmt(handle, p, fmt, 0, 1024, o, 0,
                                                                             C.byref(nf)),
        "fmd_process_stream_fmt": lambda: lib.fmd_process_stream_fmt(handle, p, fmt, 1024, o),
        "fmd_receiver_write_fmt": lambda: lib.fmd_receiver_write_fmt(handle, p, fmt, 1024),
        "fmd_scan_accumulate_device_fmt": lambda: lib.fmd_scan_accumulate_device_fmt(handle, p, fmt, 0, 1024, None),
        "fmd_scan_accumulate_host_fmt": lambda: lib.fmd_scan_accumulate_host_fmt(handle, p, fmt, 0, 1024),
    }


def test_fmt_symbols_are_exported_and_bound(pkg):
    lib = pkg.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in pkg.EXPORTS
        assert getattr(lib, name).argtypes is not None, name
    assert (pkg.FMD_IQ_F32, pkg.FMD_IQ_U8, pkg.FMD_IQ_S8, pkg.FMD_IQ_S16) == (0, 1, 2, 3)
    assert pkg.IQ_BYTES == {0: 8, 1: 2, 2: 2, 3: 4}
    for name in ("process_host_fmt",):
        assert hasattr(pkg.Batch, name)
    for name in ("ProcessStreamS8", "ProcessStreamS16"):
        assert hasattr(pkg.FmDecoder, name)
    assert hasattr(pkg.Receiver, "write")


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
@pytest.mark.parametrize("name", SYMBOLS)
def test_null_object_is_refused_for_every_format(pkg, name, fmt):
    lib = pkg.lib()
    assert _calls(lib, None, fmt)[name]() == FMD_ERR_ARG
    msg = lib.fmd_last_error()
    assert b"null" in msg and len(msg.split()) >= 2, msg


@pytest.mark.parametrize("fmt", [-1, 4])
@pytest.mark.parametrize("name", SYMBOLS)
def test_format_outside_the_enum_is_refused_with_a_sentence(pkg, name, fmt):
    """The format is the first thing every entry point looks at: the sentence names it even when the object is null,
    and the call returns before any HIP call (this test runs without a GPU)."""
    lib = pkg.lib()
    assert _calls(lib, None, fmt)[name]() == FMD_ERR_ARG
    msg = lib.fmd_last_error()
    assert name.encode() in msg and b"format" in msg and len(msg.split()) >= 5, msg


def test_python_layer_picks_the_format_from_the_dtype(pkg):
    a, fmt, per = pkg.iq_format_of(np.zeros(8, np.complex64))
    assert (fmt, per) == (pkg.FMD_IQ_F32, 1)
    for dt, want in ((np.float32, pkg.FMD_IQ_F32), (np.uint8, pkg.FMD_IQ_U8), (np.int8, pkg.FMD_IQ_S8),
                     (np.int16, pkg.FMD_IQ_S16)):
        a, fmt, per = pkg.iq_format_of(np.zeros(8, dt))
        assert (fmt, per, a.dtype) == (want, 2, np.dtype(dt))
    for dt in (np.float64, np.int32, np.uint16, np.complex128):
        with pytest.raises(pkg.FmdError, match="fmd error -1"):
            pkg.iq_format_of(np.zeros(8, dt))


def test_signed_conversions_are_exact_for_every_value(tmp_path):
    exe = str(tmp_path / "iq_convert_check")
    src = os.path.join(ROOT, "tests", "cpp", "iq_convert_check.c")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-I", os.path.join(PKG_DIR, "csrc"), src, "-lm",
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {"s16": {}, "s8": {}}
    for line in out:
        if line:
            kind, v, bits = line.split()
            got[kind][int(v)] = int(bits, 16)
    v16 = np.arange(-32768, 32768).astype(np.int16)
    v8 = np.arange(-128, 128).astype(np.int8)
    want16 = (v16.astype(np.float32) * np.float32(2.0 ** -15)).view(np.uint32)
    want8 = (v8.astype(np.float32) * np.float32(2.0 ** -7)).view(np.uint32)
    assert len(got["s16"]) == 65536 and len(got["s8"]) == 256
    assert np.array_equal(np.array([got["s16"][int(v)] for v in v16], dtype=np.uint32), want16)
    assert np.array_equal(np.array([got["s8"][int(v)] for v in v8], dtype=np.uint32), want8)
    minus_one = int(np.float32(-1.0).view(np.uint32))
    assert got["s16"][-32768] == minus_one and got["s8"][-128] == minus_one
    # exactness: the float product is the real number v / 2^15 (v / 2^7)
    assert np.array_equal(want16.view(np.float32).astype(np.float64) * 32768.0, v16.astype(np.float64))
    assert np.array_equal(want8.view(np.float32).astype(np.float64) * 128.0, v8.astype(np.float64))
