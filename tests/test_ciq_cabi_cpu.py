"""CPU-only checks of the public call record and the channel IQ output of the C ABI (include/fmd.h: fmd_call,
fmd_rows, FMD_CIQ_*, the _call entry points and fmd_batch_select_ciq): the symbols are exported, declared and bound and
the ctypes structures have the header's layout; a record of another size, a null record, batch or decoder give
FMD_ERR_ARG and a sentence before the HIP runtime is touched; a ciq.format outside its enum is refused before any other
format; include/fmd.h compiles as C; and the host build of the conversion (tests/cpp/ciq_convert_check.c over
csrc/fmd_math.h, the source the GPU executes) equals mpx16() of both parts on every tie, every integer and the edge
values -- the value sets are those of tests/test_mpx_cabi_cpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from __graft_entry__ import PKG_DIR, ROOT, load_package
from test_mpx_cabi_cpu import mpx16, value_sets

FMD_ERR_ARG = -1
CALLS = ("fmd_batch_process_device_call", "fmd_batch_process_host_call", "fmd_process_stream_call")
SYMBOLS = CALLS + ("fmd_batch_select_ciq", "fmd_batch_get_ciq_selection")


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def _record(pkg, iq_fmt=0, pcm_fmt=0, mpx_fmt=0, feed_fmt=0, ciq_fmt=0, with_ciq=True, keep=[]):
    """a record whose pointers are valid host arrays (nothing reads them: every call here is refused)"""
    buf, out, rows = np.zeros(4096, np.float32), np.zeros(4096, np.float32), np.zeros(4096, np.float32)
    nf, nq = C.c_uint(7), C.c_uint(7)
    keep[:] = [buf, out, rows, nf, nq]
    call = pkg.make_call(buf.ctypes.data, iq_fmt, 0, 1024,
                         audio=pkg.make_rows(out.ctypes.data, pcm_fmt, 0, nf),
                         mpx=pkg.make_rows(None, mpx_fmt), feed=pkg.make_rows(None, feed_fmt),
                         ciq=pkg.make_rows(rows.ctypes.data if with_ciq else None, ciq_fmt, 1024, nq))
    return call, nq


def test_symbols_are_exported_declared_and_bound(pkg):
    lib = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "fmd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in pkg.EXPORTS
        assert getattr(lib, name).argtypes is not None, name
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared in include/fmd.h"
    assert re.search(r"#define\s+FMD_CIQ_F32\s+0\b", code) and re.search(r"#define\s+FMD_CIQ_S16\s+1\b", code)
    assert (pkg.FMD_CIQ_F32, pkg.FMD_CIQ_S16) == (0, 1)
    assert pkg.CIQ_BYTES == {0: 8, 1: 4}
    for name in ("select_ciq", "ciq_selection", "process_call", "process_host_fmt", "process_device"):
        assert hasattr(pkg.Batch, name)
    assert hasattr(pkg.FmDecoder, "ProcessStreamWithChannelIq")
    assert "ProcessStreamWithChannelIq" in open(os.path.join(ROOT, "include", "fm_decoder.hpp")).read()
    # the header says what the units are, that nobody counts saturated samples, and where the conversion is tested
    assert "COMPLEX SAMPLES" in hdr and "what = 9" in hdr


def test_ctypes_structures_have_the_headers_layout(pkg, tmp_path):
    """sizeof and every offsetof, from a C program that includes the header"""
    fields = ["size", "iq", "iq_format", "iq_channel_stride", "samples", "audio", "mpx", "feed", "ciq", "stream"]
    rows = ["p", "format", "stride", "count"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fmd.h"\nint main(void)\n{\n'
                   '  printf("%zu %zu", sizeof(fmd_call), sizeof(fmd_rows));\n'
                   + "".join('  printf(" %%zu", offsetof(fmd_call, %s));\n' % f for f in fields)
                   + "".join('  printf(" %%zu", offsetof(fmd_rows, %s));\n' % f for f in rows)
                   + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    want = ([C.sizeof(pkg.FmdCall), C.sizeof(pkg.FmdRows)] + [getattr(pkg.FmdCall, f).offset for f in fields]
            + [getattr(pkg.FmdRows, f).offset for f in rows])
    assert got == want
    assert pkg.make_call(None, 0, 0, 0).size == got[0]


def test_header_still_compiles_as_c(tmp_path):
    src = tmp_path / "hdr.c"
    src.write_text('#include "fmd.h"\nint main(void)\n{\n  fmd_call c = {sizeof(fmd_call)};\n'
                   "  c.ciq.format = FMD_CIQ_S16;\n  return fmd_batch_process_device_call(0, &c) == FMD_OK;\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "include"), str(src)])


@pytest.mark.parametrize("name", CALLS)
def test_null_record_and_wrong_size_are_refused(pkg, name):
    lib = pkg.lib()
    fn = getattr(lib, name)
    assert fn(None, None) == FMD_ERR_ARG
    msg = lib.fmd_last_error()
    assert name.encode() in msg and b"null call record" in msg, msg
    for delta in (-8, 8, -pkg.make_call(None, 0, 0, 0).size):
        call, nq = _record(pkg)
        call.size += delta
        assert fn(None, C.byref(call)) == FMD_ERR_ARG
        msg = lib.fmd_last_error()
        assert name.encode() in msg and b"sizeof(fmd_call)" in msg, msg
        assert nq.value == 7  # a record that is not understood is not written through


@pytest.mark.parametrize("with_ciq", [True, False], ids=["ciq", "null-ciq"])
@pytest.mark.parametrize("ciq", [0, 1])
@pytest.mark.parametrize("name", CALLS)
def test_null_object_is_refused(pkg, name, ciq, with_ciq):
    """no batch, no decoder: FMD_ERR_ARG and a sentence (this test runs without a GPU: no HIP call comes first)"""
    lib = pkg.lib()
    call, nq = _record(pkg, ciq_fmt=ciq, with_ciq=with_ciq)
    assert getattr(lib, name)(None, C.byref(call)) == FMD_ERR_ARG
    msg = lib.fmd_last_error()
    assert b"null" in msg and len(msg.split()) >= 2, msg
    assert nq.value == 0  # the count a refused call would leave behind is cleared


@pytest.mark.parametrize("iq,pcm,mpx,feed", [(0, 0, 0, 0), (-1, 0, 0, 0), (4, 2, 2, 2), (0, -1, -1, -1), (0, 0, 0, 2)])
@pytest.mark.parametrize("ciq", [-1, 2])
@pytest.mark.parametrize("name", CALLS)
def test_ciq_format_outside_the_enum_is_refused_first(pkg, name, ciq, iq, pcm, mpx, feed):
    """whatever the object and the other four formats are, the sentence names the entry point and FMD_CIQ"""
    lib = pkg.lib()
    for with_ciq in (True, False):
        call, _ = _record(pkg, iq, pcm, mpx, feed, ciq, with_ciq)
        assert getattr(lib, name)(None, C.byref(call)) == FMD_ERR_ARG
        msg = lib.fmd_last_error()
        assert name.encode() in msg and b"format" in msg and b"FMD_CIQ" in msg and len(msg.split()) >= 5, msg


@pytest.mark.parametrize("name", CALLS)
def test_the_other_formats_keep_their_sentences_and_their_order(pkg, name):
    """behind the ciq format: feed, multiplex, IQ, audio -- the _feed entry points' order -- under the _call name"""
    lib = pkg.lib()
    for fmts, word in (((4, 2, 2, 2), b"FMD_FEED"), ((4, 2, 2, 0), b"FMD_MPX"), ((4, 2, 0, 0), b"FMD_IQ"),
                       ((0, 2, 0, 0), b"FMD_PCM")):
        call, _ = _record(pkg, *fmts, ciq_fmt=1)
        assert getattr(lib, name)(None, C.byref(call)) == FMD_ERR_ARG
        msg = lib.fmd_last_error()
        assert name.encode() in msg and word in msg, (fmts, msg)


def test_selection_of_no_batch_is_refused(pkg):
    lib = pkg.lib()
    ch = np.zeros(4, np.uint32)
    assert lib.fmd_batch_select_ciq(None, ch.ctypes.data, 1) == FMD_ERR_ARG
    assert b"fmd_batch_select_ciq" in lib.fmd_last_error() and b"null" in lib.fmd_last_error()
    assert lib.fmd_batch_get_ciq_selection(None, ch.ctypes.data, 4) == FMD_ERR_ARG
    assert b"fmd_batch_get_ciq_selection" in lib.fmd_last_error()


def test_python_layer_refuses_other_dtypes(pkg):
    assert pkg.ciq_format_of(np.complex64) == pkg.FMD_CIQ_F32
    assert pkg.ciq_format_of(np.int16) == pkg.FMD_CIQ_S16
    assert pkg.ciq_format_of(pkg.FMD_CIQ_S16) == pkg.FMD_CIQ_S16
    for dt in (None, np.float32, np.complex128, np.int8, 2, -1, True):
        with pytest.raises(pkg.FmdError, match="fmd error -1"):
            pkg.ciq_format_of(dt)


def test_host_build_of_the_conversion_equals_mpx16_of_both_parts(tmp_path):
    """every value of the sets as a real part beside every other as the imaginary part (the set against itself
    reversed): the packed word holds mpx16(re) below mpx16(im)"""
    exe = str(tmp_path / "ciq_convert_check")
    src = os.path.join(ROOT, "tests", "cpp", "ciq_convert_check.c")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-I", os.path.join(PKG_DIR, "csrc"), src, "-lm",
                           "-o", exe])
    for name, x in value_sets().items():
        z = np.stack([x, x[::-1]], axis=1).astype(np.float32)
        fin, fout = str(tmp_path / (name + ".c64")), str(tmp_path / (name + ".s16"))
        z.tofile(fin)
        subprocess.run([exe, fin, fout], check=True)
        got = np.fromfile(fout, dtype=np.int16).reshape(-1, 2)
        want = np.stack([mpx16(z[:, 0]), mpx16(z[:, 1])], axis=1)
        assert got.shape == want.shape, (name, got.shape)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (name, [(z[i].tolist(), got[i].tolist(), want[i].tolist()) for i in bad[:8]])
