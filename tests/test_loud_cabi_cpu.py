"""CPU-only checks of the loudness meter's C ABI (include/fmd.h, "ITU-R BS.1770 loudness blocks"): the entry points
are declared and exported, the record has the layout the header states -- seen from a C program --, the header
compiles as C, what is refused without a batch is refused without a device call, and the host arithmetic over block
records (fmd_loudness_window, fmd_loudness_integrated) equals its numpy restatement in tests/loud_spec.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import loud_spec as ls
from __graft_entry__ import ROOT, load_package

NAMES = ["fmd_batch_set_loudness", "fmd_batch_get_loudness", "fmd_batch_loudness_block_frames",
         "fmd_batch_get_loudness_coeffs", "fmd_batch_collect_loudness", "fmd_loudness_window",
         "fmd_loudness_integrated", "fmd_batch_debug_loud_skip_carry"]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def test_the_entry_points_are_declared_and_exported(pkg):
    hdr = open(os.path.join(ROOT, "include", "fmd.h")).read()
    lib = pkg.lib()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, hdr) and hasattr(lib, n) and n in pkg.EXPORTS, n
    for name, value in (("FMD_LOUDNESS_OFF", 0), ("FMD_LOUDNESS_ON", 1)):
        assert re.search(r"#define %s %d\b" % (name, value), hdr)
    assert "Tech 3342" in hdr and "true peak" in hdr  # what is out of scope is said


def test_the_python_and_cpp_surfaces_are_there(pkg):
    for name in ("set_loudness", "loudness", "loudness_block_frames", "loudness_coeffs", "collect_loudness"):
        assert hasattr(pkg.Batch, name)
    import importlib
    loud = importlib.import_module(pkg.__name__ + ".loudness")
    for name in ("momentary", "short_term", "integrated", "window"):
        assert callable(getattr(loud, name))
    hpp = open(os.path.join(ROOT, "include", "fm_decoder.hpp")).read()
    for name, call in (("SetLoudness", "fmd_batch_set_loudness"), ("CollectLoudness", "fmd_batch_collect_loudness")):
        assert re.search(r"\b%s\s*\(" % name, hpp) and call in hpp, name


C_PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "fmd.h"
int main(void)
{
  fmd_loud_block b[2];
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(fmd_loud_block), offsetof(fmd_loud_block, z_l),
         offsetof(fmd_loud_block, z_r), offsetof(fmd_loud_block, peak_l), offsetof(fmd_loud_block, peak_r),
         (size_t)((char*)&b[1] - (char*)&b[0]));
  return FMD_LOUDNESS_ON - 1;
}
"""


def test_the_header_compiles_as_c_and_the_record_is_16_bytes(pkg, tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(C_PROGRAM)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split() == ["16", "0", "4", "8", "12", "16"]
    assert pkg.LOUD_BLOCK_DTYPE == ls.LOUD_BLOCK_DTYPE and pkg.LOUD_BLOCK_DTYPE.itemsize == 16
    assert [pkg.LOUD_BLOCK_DTYPE.fields[n][1] for n in ("z_l", "z_r", "peak_l", "peak_r")] == [0, 4, 8, 12]


CPP_CALLER = """
#define FMD_NO_CFMDECODER_ALIAS
#include "fm_decoder.hpp"
struct R {
  bool AddUECPDataFrame(unsigned char*, unsigned) { return true; }
  bool SetChannelName(std::string) { return true; }
  bool IsSettingActive() { return false; }
};
unsigned use(cFmDecoderT<R>& d) {
  fmd_loud_block b[8];
  uint64_t first = 0;
  unsigned lost = 0;
  return d.SetLoudness(true, 0, 64) + d.CollectLoudness(b, 8, &first, &lost) + d.SetLoudness(false);
}
"""


def test_a_cpp_caller_of_the_two_methods_compiles(tmp_path):
    src = tmp_path / "caller.cpp"
    src.write_text(CPP_CALLER)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_bad_arguments_are_refused_without_a_device(pkg):
    """the arguments' own ranges are checked in front of everything else, so no batch is needed to see them refused"""
    L = pkg.lib()
    for mode in (-1, 2, 7):
        assert L.fmd_batch_set_loudness(None, mode, 0, 0) == -1 and b"mode must be" in L.fmd_last_error()
    for bf in (1, 15, (1 << 20) + 1):
        assert L.fmd_batch_set_loudness(None, 1, bf, 0) == -1 and b"block_frames must be" in L.fmd_last_error()
    for ring in (1, 7, 4097):
        assert L.fmd_batch_set_loudness(None, 1, 0, ring) == -1 and b"ring_blocks must be" in L.fmd_last_error()
    for bf, ring in ((0, 0), (16, 8), (1 << 20, 4096)):  # in range: only the batch is missing
        assert L.fmd_batch_set_loudness(None, 1, bf, ring) == -1 and b"null batch" in L.fmd_last_error()
    rec, first, lost = np.zeros(4, pkg.LOUD_BLOCK_DTYPE), C.c_uint64(5), C.c_uint(7)
    assert L.fmd_batch_get_loudness(None) < 0
    assert L.fmd_batch_loudness_block_frames(None) == 0
    assert L.fmd_batch_get_loudness_coeffs(None, rec.ctypes.data) < 0
    assert L.fmd_batch_collect_loudness(None, rec.ctypes.data, 4, 0, 1, 0, None, C.byref(first), C.byref(lost)) < 0
    assert L.fmd_batch_debug_loud_skip_carry(None, 1) < 0
    assert not rec.view(np.uint8).any()


def test_the_debug_key_table_still_has_14_keys():
    """the mutation switch is an entry point of its own: fmd_batch_debug_set keeps its 14 keys"""
    src = open(os.path.join(ROOT, "pvr.rtl.radiofm_amd", "csrc", "fmd_batch.hip")).read()
    keys = re.findall(r'k == "(\w+)"', re.search(r"int fmd_batch_debug_set\(.*?\n}\n", src, re.S).group(0))
    assert len(keys) == len(set(keys)) == 14 and not [k for k in keys if "loud" in k], keys


def test_the_loudness_kernels_keep_float_denormals(tmp_path):
    """"Denormals are kept" is part of the definition.  No input reaches the meter of this decoder with a denormal
    (tests/test_gpu_loud.py, the silent capture), so it is pinned where it is decided: compiled with the library's
    flags, every loudness kernel's descriptor asks for float32 denormals in and out (float_denorm_mode_32 = 3)."""
    llvm = "/opt/rocm/lib/llvm/bin"
    csrc = os.path.join(ROOT, "pvr.rtl.radiofm_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^FLAGS = (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    co, elf = str(tmp_path / "loud.co"), str(tmp_path / "loud.elf")
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--offload-device-only", "-c",
                        os.path.join(csrc, "fmd_loud.hip"), "-o", co], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + co,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + elf])
    text = subprocess.check_output([os.path.join(llvm, "llvm-objdump"), "-D", "--no-show-raw-insn", elf], text=True)
    kernels = re.findall(r"\.amdhsa_kernel (\S*k_audio_tail\S*loud\S*)(.*?)\.end_amdhsa_kernel", text, re.S)
    assert len(kernels) == 8, [k for k, _ in kernels]
    for name, body in kernels:
        assert re.search(r"\.amdhsa_float_denorm_mode_32 3\b", body), name


# ---- the host arithmetic ----

def _blocks(powers, bf, split=0.5):
    """block records whose (z_l + z_r) / bf is `powers` (float32 sums: the restatement reads the same records)"""
    b = np.zeros(len(powers), ls.LOUD_BLOCK_DTYPE)
    p = np.asarray(powers, np.float64) * bf
    b["z_l"], b["z_r"] = (p * split).astype(np.float32), (p * (1.0 - split)).astype(np.float32)
    return b


def _lufs_power(l):
    return 10.0 ** ((l + 0.691) / 10.0)


def _c_window(pkg, b, bf):
    b = np.ascontiguousarray(b)
    return pkg.lib().fmd_loudness_window(b.ctypes.data, b.size, bf)


def _c_integrated(pkg, b, bf):
    b = np.ascontiguousarray(b)
    return pkg.lib().fmd_loudness_integrated(b.ctypes.data if b.size else None, b.size, bf)


CASES = {
    "all equal": [_lufs_power(-23.0)] * 40,
    "a quiet stretch 13 LU under a loud one": [_lufs_power(-20.0)] * 30 + [_lufs_power(-33.0)] * 30,
    "a stretch under -70": [_lufs_power(-23.0)] * 25 + [_lufs_power(-80.0)] * 25 + [_lufs_power(-18.0)] * 5,
    "everything under -70": [_lufs_power(-75.0)] * 12,
    "ramp": list(_lufs_power(np.linspace(-60.0, -10.0, 57))),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_integrated_and_window_equal_the_numpy_restatement(pkg, name):
    """Both sides are double arithmetic on the same float records, with the sums in the same order (a window: its
    blocks in order, z_l + z_r of each; the gates' means: the surviving windows in order), so 1e-9 LU is generous."""
    bf = 4800
    b = _blocks(CASES[name], bf, split=0.3)
    got, want = _c_integrated(pkg, b, bf), ls.integrated(b, bf)
    print(name, got, want)
    if np.isinf(want):
        assert got == want == -np.inf
    else:
        assert abs(got - want) <= 1e-9
    for n in (1, 4, 30):
        for at in (0, 3, len(b) - n):
            w = b[at:at + n]
            if len(w) == n:
                assert abs(_c_window(pkg, w, bf) - ls.window(w, bf)) <= 1e-9


def test_what_the_gates_drop(pkg):
    bf = 4800
    # equal blocks: the integrated loudness is every window's
    assert abs(_c_integrated(pkg, _blocks(CASES["all equal"], bf), bf) - (-23.0)) <= 1e-5
    # the quiet stretch lies 13 LU under the loud one: under the relative gate (10 LU under the mean of both, which is
    # itself under -20), so only windows with loud blocks in them count -- the answer is well above the plain mean
    b = _blocks(CASES["a quiet stretch 13 LU under a loud one"], bf)
    plain = ls.window(b, bf)
    got = _c_integrated(pkg, b, bf)
    assert plain < -22.7 and -20.6 < got <= -20.0
    # the stretch under -70 is dropped by the absolute gate: without it the relative gate would sit lower
    b = _blocks(CASES["a stretch under -70"], bf)
    assert abs(_c_integrated(pkg, b, bf) - ls.integrated(b, bf)) <= 1e-9
    assert _c_integrated(pkg, b, bf) > ls.window(b, bf) + 1.0
    assert _c_integrated(pkg, _blocks(CASES["everything under -70"], bf), bf) == -np.inf


def test_fewer_than_four_blocks_and_nan_blocks(pkg):
    bf = 1000
    b = _blocks([_lufs_power(-23.0)] * 12, bf)
    for n in range(4):
        assert _c_integrated(pkg, b[:n], bf) == -np.inf == ls.integrated(b[:n], bf)
    assert np.isfinite(_c_integrated(pkg, b[:4], bf))
    # a NaN block: the four windows that hold it pass no gate, the others give the answer
    c = b.copy()
    c["z_l"][5] = np.nan
    got, want = _c_integrated(pkg, c, bf), ls.integrated(c, bf)
    assert np.isfinite(got) and abs(got - want) <= 1e-9 and abs(got - (-23.0)) <= 1e-5
    assert np.isnan(_c_window(pkg, c[4:8], bf)) and np.isnan(ls.window(c[4:8], bf))
    c["z_r"][:] = np.nan
    assert _c_integrated(pkg, c, bf) == -np.inf == ls.integrated(c, bf)


def test_the_python_module_goes_through_the_c_functions(pkg):
    import importlib
    loud = importlib.import_module(pkg.__name__ + ".loudness")
    bf = 4800
    b = _blocks(CASES["ramp"], bf)
    m, s = loud.momentary(b, bf), loud.short_term(b, bf)
    assert m.shape == (len(b) - 3,) and s.shape == (len(b) - 29,)
    assert m[7] == _c_window(pkg, b[7:11], bf) and s[2] == _c_window(pkg, b[2:32], bf)
    assert loud.integrated(b, bf) == _c_integrated(pkg, b, bf)
    assert loud.integrated(b[:2], bf) == -np.inf
