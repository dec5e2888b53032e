"""CPU-only checks of the 16-bit PCM output of the C ABI (include/fmd.h, FMD_PCM_* and the _pcm entry points): the
four entry points are exported and bound, a null batch / decoder and a PCM or IQ format outside its enum are refused
with FMD_ERR_ARG and a sentence before the HIP runtime is touched, and the conversion of csrc/fmd_math.h (host build
of the source the GPU executes) equals the contract's numpy function pcm16() on every tie, every integer, the edge
values and a million random bit patterns."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from __graft_entry__ import PKG_DIR, ROOT, load_package

FMD_ERR_ARG = -1
SYMBOLS = ("fmd_batch_process_device_pcm", "fmd_batch_process_host_pcm", "fmd_process_stream_pcm",
           "fmd_batch_read_pcm_clipped")
PROCESS = SYMBOLS[:3]


def pcm16(x):
    y = np.asarray(x, np.float32) * np.float32(32768.0)
    with np.errstate(invalid="ignore"):
        r = np.clip(np.rint(y), -32768.0, 32767.0)
    return np.where(np.isnan(y), 0, r).astype(np.int16)


def clipped(x):
    """samples whose rounded value has to be clamped (NaN is not one)"""
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(np.asarray(x, np.float32) * np.float32(32768))
        return (r > 32767) | (r < -32768)


def value_sets():
    """every tie (k + 0.5) / 32768 and every integer k / 32768, k = -32769 ... 32768; the contract's edge list, +-0,
    the smallest denormal, 1e30, NaN; 10^6 random 32-bit patterns as floats"""
    k = np.arange(-32769, 32769, dtype=np.float64)
    ties = ((k + 0.5) / 32768.0).astype(np.float32)
    ints = (k / 32768.0).astype(np.float32)
    assert np.array_equal(ties.astype(np.float64) * 32768.0, k + 0.5)  # exact in float32
    edges = np.array([1.0, -1.0, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, 32767.5 / 32768, np.inf, -np.inf, 0.0, -0.0,
                      np.float32(1e-45), -np.float32(1e-45), 1e30, -1e30, np.nan, -np.nan, 32766.5 / 32768,
                      -32768.5 / 32768, -32767.5 / 32768, 3.4e38, -3.4e38], dtype=np.float32)
    rnd = np.random.default_rng(16).integers(0, 2 ** 32, 10 ** 6, dtype=np.uint64).astype(np.uint32).view(np.float32)
    return {"ties": ties, "integers": ints, "edges": edges, "random": rnd}


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def _calls(lib, handle, iq_fmt, pcm_fmt):
    """every _pcm entry point with `handle` as its object and the two formats; the other arguments are valid"""
    buf = np.zeros(4096, np.float32)
    out = np.zeros(4096, np.float32)
    cnt = np.zeros(4, np.uint64)
    nf = C.c_uint()
    p, o = buf.ctypes.data, out.ctypes.data
    return {
        "fmd_batch_process_device_pcm": lambda: lib.fmd_batch_process_device_pcm(handle, p, iq_fmt, 0, 1024, o, pcm_fmt,
                                                                                 0, C.byref(nf), None),
        "fmd_batch_process_host_pcm": lambda: lib.fmd_batch_process_host_pcm(handle, p, iq_fmt, 0, 1024, o, pcm_fmt, 0,
                                                                             C.byref(nf)),
        "fmd_process_stream_pcm": lambda: lib.fmd_process_stream_pcm(handle, p, iq_fmt, 1024, o, pcm_fmt),
        "fmd_batch_read_pcm_clipped": lambda: lib.fmd_batch_read_pcm_clipped(handle, 0, 1, cnt.ctypes.data),
    }


def test_pcm_symbols_are_exported_and_bound(pkg):
    lib = pkg.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in pkg.EXPORTS
        assert getattr(lib, name).argtypes is not None, name
    assert (pkg.FMD_PCM_F32, pkg.FMD_PCM_S16) == (0, 1)
    assert pkg.PCM_BYTES == {0: 4, 1: 2}
    for name in ("process_host_fmt", "process_device", "pcm_clipped"):
        assert hasattr(pkg.Batch, name)
    assert hasattr(pkg.FmDecoder, "ProcessStreamToPcm16")


@pytest.mark.parametrize("pcm", [0, 1])
@pytest.mark.parametrize("name", SYMBOLS)
def test_null_object_is_refused_for_every_format(pkg, name, pcm):
    lib = pkg.lib()
    assert _calls(lib, None, 0, pcm)[name]() == FMD_ERR_ARG
    msg = lib.fmd_last_error()
    assert b"null" in msg and len(msg.split()) >= 2, msg


@pytest.mark.parametrize("pcm", [-1, 2])
@pytest.mark.parametrize("name", PROCESS)
def test_pcm_format_outside_the_enum_is_refused_with_a_sentence(pkg, name, pcm):
    """The formats are the first things every entry point looks at: the sentence names the function and the word
    "format" even when the object is null, and the call returns before any HIP call (this test runs without a GPU)."""
    lib = pkg.lib()
    assert _calls(lib, None, 0, pcm)[name]() == FMD_ERR_ARG
    msg = lib.fmd_last_error()
    assert name.encode() in msg and b"format" in msg and b"FMD_PCM" in msg and len(msg.split()) >= 5, msg


@pytest.mark.parametrize("iq", [-1, 4])
@pytest.mark.parametrize("name", PROCESS)
def test_iq_format_outside_the_enum_is_refused_with_a_sentence(pkg, name, iq):
    lib = pkg.lib()
    assert _calls(lib, None, iq, 1)[name]() == FMD_ERR_ARG
    msg = lib.fmd_last_error()
    assert name.encode() in msg and b"format" in msg and b"FMD_IQ" in msg and len(msg.split()) >= 5, msg


def test_python_layer_refuses_other_output_dtypes(pkg):
    assert pkg.pcm_format_of(None) == pkg.FMD_PCM_F32
    assert pkg.pcm_format_of(np.float32) == pkg.FMD_PCM_F32
    assert pkg.pcm_format_of(np.int16) == pkg.FMD_PCM_S16
    assert pkg.pcm_format_of(pkg.FMD_PCM_S16) == pkg.FMD_PCM_S16
    for dt in (np.int8, np.int32, np.float64, 2, -1):
        with pytest.raises(pkg.FmdError, match="fmd error -1"):
            pkg.pcm_format_of(dt)


def test_the_specification_on_its_own_examples():
    x = np.array([1.0, -1.0, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, 32767.5 / 32768, np.inf, -np.inf, np.nan],
                 np.float32)
    assert pcm16(x).tolist() == [32767, -32768, 0, 2, 2, 32767, 32767, -32768, 0]
    assert clipped(x).tolist() == [True, False, False, False, False, True, True, True, False]


def test_host_build_of_the_conversion_equals_pcm16(tmp_path):
    exe = str(tmp_path / "pcm_convert_check")
    src = os.path.join(ROOT, "tests", "cpp", "pcm_convert_check.c")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-I", os.path.join(PKG_DIR, "csrc"), src, "-lm",
                           "-o", exe])
    for name, x in value_sets().items():
        fin, fout = str(tmp_path / (name + ".f32")), str(tmp_path / (name + ".s16"))
        x.tofile(fin)
        n_clip = int(subprocess.run([exe, fin, fout], capture_output=True, text=True, check=True).stdout)
        got = np.fromfile(fout, dtype=np.int16)
        want = pcm16(x)
        bad = np.flatnonzero(got != want) if got.size == want.size else None
        assert bad is not None and bad.size == 0, (name, [(float(x[i]), int(got[i]), int(want[i])) for i in bad[:8]])
        assert n_clip == int(clipped(x).sum()), name
    # the sets hold what they are meant to hold
    v = value_sets()
    assert np.isnan(v["random"]).any() and (np.abs(v["random"]) < np.float32(1.2e-38)).any()  # NaN, denormals
    assert (np.abs(v["random"]) > 1).any() and (np.abs(v["random"]) < 1).any()
    assert clipped(v["ties"]).sum() >= 2 and clipped(v["integers"]).sum() >= 2
