"""CPU-only checks of the demodulated multiplex output of the C ABI (include/fmd.h, FMD_MPX_* and the _mpx entry
points): the five entry points are exported, declared and bound; without a batch or decoder every one of them fails
loudly (FMD_ERR_ARG and a sentence, the two getters 0) before the HIP runtime is touched; a multiplex format outside
its enum is refused before anything else is looked at; and the conversion of csrc/fmd_math.h (host build of the
source the GPU executes) equals the contract's numpy function mpx16() on every tie, every integer and the edge
values."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from __graft_entry__ import PKG_DIR, ROOT, load_package
from feed_spec import mpx16

FMD_ERR_ARG = -1
SYMBOLS = ("fmd_batch_process_device_mpx", "fmd_batch_process_host_mpx", "fmd_process_stream_mpx",
           "fmd_batch_max_mpx_samples", "fmd_batch_mpx_rate")
PROCESS = SYMBOLS[:3]


def value_sets():
    """every tie (k + 0.5) / 8192 and every integer k / 8192, k = -32769 ... 32768; +-0, the smallest denormal,
    +-inf, NaN, +-3.4e38 and the scale's landmarks (+-75 kHz = +-2.5, full scale +-4.0)"""
    k = np.arange(-32769, 32769, dtype=np.float64)
    ties = ((k + 0.5) / 8192.0).astype(np.float32)
    ints = (k / 8192.0).astype(np.float32)
    assert np.array_equal(ties.astype(np.float64) * 8192.0, k + 0.5)  # exact in float32
    edges = np.array([0.0, -0.0, np.float32(1e-45), -np.float32(1e-45), np.inf, -np.inf, np.nan, -np.nan, 3.4e38,
                      -3.4e38, 2.5, -2.5, 4.0, -4.0, 0.5 / 8192, 1.5 / 8192, 2.5 / 8192, 32767.5 / 8192,
                      -32768.5 / 8192, 1e-38, -1e-38], dtype=np.float32)
    return {"ties": ties, "integers": ints, "edges": edges}


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def _calls(lib, handle, iq_fmt, pcm_fmt, mpx_fmt, with_mpx=True):
    """every _mpx entry point with `handle` as its object and the three formats; the other arguments are valid"""
    buf = np.zeros(4096, np.float32)
    out = np.zeros(4096, np.float32)
    mpx = np.zeros(4096, np.float32)
    nf, nm = C.c_uint(), C.c_uint()
    p, o, m = buf.ctypes.data, out.ctypes.data, mpx.ctypes.data if with_mpx else None
    return {
        "fmd_batch_process_device_mpx": lambda: lib.fmd_batch_process_device_mpx(
            handle, p, iq_fmt, 0, 1024, o, pcm_fmt, 0, C.byref(nf), m, mpx_fmt, 1024, C.byref(nm), None),
        "fmd_batch_process_host_mpx": lambda: lib.fmd_batch_process_host_mpx(
            handle, p, iq_fmt, 0, 1024, o, pcm_fmt, 0, C.byref(nf), m, mpx_fmt, 1024, C.byref(nm)),
        "fmd_process_stream_mpx": lambda: lib.fmd_process_stream_mpx(handle, p, iq_fmt, 1024, o, pcm_fmt, m, mpx_fmt,
                                                                     C.byref(nm)),
    }


def test_mpx_symbols_are_exported_declared_and_bound(pkg):
    lib = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "fmd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in pkg.EXPORTS
        assert getattr(lib, name).argtypes is not None, name
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared in include/fmd.h"
    assert re.search(r"#define\s+FMD_MPX_F32\s+0\b", code) and re.search(r"#define\s+FMD_MPX_S16\s+1\b", code)
    assert (pkg.FMD_MPX_F32, pkg.FMD_MPX_S16) == (0, 1)
    assert pkg.MPX_BYTES == {0: 4, 1: 2}
    for name in ("process_host_fmt", "process_device", "max_mpx_samples", "mpx_rate"):
        assert hasattr(pkg.Batch, name)
    assert hasattr(pkg.FmDecoder, "ProcessStreamWithMpx")
    assert "ProcessStreamWithMpx" in open(os.path.join(ROOT, "include", "fm_decoder.hpp")).read()
    # the header says who counts saturated samples, and what the scale is
    assert "no clip counter" in hdr and "30 000" in hdr


@pytest.mark.parametrize("with_mpx", [True, False], ids=["mpx", "null-mpx"])
@pytest.mark.parametrize("mpx", [0, 1])
@pytest.mark.parametrize("name", PROCESS)
def test_null_object_is_refused_for_every_format(pkg, name, mpx, with_mpx):
    """no batch, no decoder: FMD_ERR_ARG and a sentence, with and without multiplex rows"""
    lib = pkg.lib()
    assert _calls(lib, None, 0, 0, mpx, with_mpx)[name]() == FMD_ERR_ARG
    msg = lib.fmd_last_error()
    assert b"null" in msg and len(msg.split()) >= 2, msg


def test_getters_of_no_batch_return_zero(pkg):
    lib = pkg.lib()
    assert lib.fmd_batch_max_mpx_samples(None, 65536) == 0
    assert lib.fmd_batch_mpx_rate(None) == 0.0


@pytest.mark.parametrize("iq,pcm", [(0, 0), (-1, 0), (4, 2), (0, -1)])
@pytest.mark.parametrize("mpx", [-1, 2])
@pytest.mark.parametrize("name", PROCESS)
def test_mpx_format_outside_the_enum_is_refused_first(pkg, name, mpx, iq, pcm):
    """The multiplex format is the first thing every entry point looks at: the sentence names the function and
    FMD_MPX whatever the object and the other two formats are, and the call returns before any HIP call (this test
    runs without a GPU)."""
    lib = pkg.lib()
    for with_mpx in (True, False):
        assert _calls(lib, None, iq, pcm, mpx, with_mpx)[name]() == FMD_ERR_ARG
        msg = lib.fmd_last_error()
        assert name.encode() in msg and b"format" in msg and b"FMD_MPX" in msg and len(msg.split()) >= 5, msg


@pytest.mark.parametrize("name", PROCESS)
def test_the_other_formats_are_still_refused_with_their_sentences(pkg, name):
    lib = pkg.lib()
    assert _calls(lib, None, 4, 0, 1)[name]() == FMD_ERR_ARG
    msg = lib.fmd_last_error()
    assert name.encode() in msg and b"FMD_IQ" in msg, msg
    assert _calls(lib, None, 0, 2, 1)[name]() == FMD_ERR_ARG
    msg = lib.fmd_last_error()
    assert name.encode() in msg and b"FMD_PCM" in msg, msg


def test_python_layer_refuses_other_multiplex_dtypes(pkg):
    assert pkg.mpx_format_of(np.float32) == pkg.FMD_MPX_F32
    assert pkg.mpx_format_of(np.int16) == pkg.FMD_MPX_S16
    assert pkg.mpx_format_of(pkg.FMD_MPX_S16) == pkg.FMD_MPX_S16
    for dt in (None, np.int8, np.int32, np.float64, 2, -1, True):
        with pytest.raises(pkg.FmdError, match="fmd error -1"):
            pkg.mpx_format_of(dt)


def test_the_specification_on_its_own_examples():
    x = np.array([2.5, -2.5, 4.0, -4.0, 0.5 / 8192, 1.5 / 8192, 2.5 / 8192, 32767.5 / 8192, np.inf, -np.inf, np.nan],
                 np.float32)
    assert mpx16(x).tolist() == [20480, -20480, 32767, -32768, 0, 2, 2, 32767, 32767, -32768, 0]


def test_host_build_of_the_conversion_equals_mpx16(tmp_path):
    exe = str(tmp_path / "mpx_convert_check")
    src = os.path.join(ROOT, "tests", "cpp", "mpx_convert_check.c")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-I", os.path.join(PKG_DIR, "csrc"), src, "-lm",
                           "-o", exe])
    for name, x in value_sets().items():
        fin, fout = str(tmp_path / (name + ".f32")), str(tmp_path / (name + ".s16"))
        x.tofile(fin)
        subprocess.run([exe, fin, fout], check=True)
        got = np.fromfile(fout, dtype=np.int16)
        want = mpx16(x)
        bad = np.flatnonzero(got != want) if got.size == want.size else None
        assert bad is not None and bad.size == 0, (name, [(float(x[i]), int(got[i]), int(want[i])) for i in bad[:8]])
    v = value_sets()
    assert (np.abs(mpx16(v["ties"]).astype(np.int32)) == 32768).any() and (mpx16(v["integers"]) == 32767).any()
