"""CPU-only checks of the block observation's C ABI (include/fmd.h, "Every RDS block decision"): the four entry points
are exported and declared, the two records have the sizes and layouts the header states, and what is refused without
a batch is refused without a device call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import rds_sync_spec as spec
from __graft_entry__ import ROOT, load_package

NAMES = ["fmd_batch_set_rds_blocks", "fmd_batch_get_rds_blocks", "fmd_batch_collect_rds_blocks",
         "fmd_batch_read_rds_quality"]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def test_the_entry_points_are_declared_and_exported(pkg):
    hdr = open(os.path.join(ROOT, "include", "fmd.h")).read()
    lib = pkg.lib()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, hdr) and hasattr(lib, n) and n in pkg.EXPORTS
    for name, value in (("FMD_RDS_BLOCKS_OFF", 0), ("FMD_RDS_BLOCKS_COUNT", 1), ("FMD_RDS_BLOCKS_RECORD", 2)):
        assert re.search(r"#define %s %d\b" % (name, value), hdr) and getattr(pkg, name) == value


def test_the_python_and_cpp_surfaces_are_there(pkg):
    for name in ("set_rds_blocks", "rds_blocks", "collect_rds_blocks", "rds_quality"):
        assert hasattr(pkg.Batch, name)
    hpp = open(os.path.join(ROOT, "include", "fm_decoder.hpp")).read()
    for name, call in (("SetRdsBlocks", "fmd_batch_set_rds_blocks"), ("CollectRdsBlocks", "fmd_batch_collect_rds_blocks"),
                       ("GetRdsQuality", "fmd_batch_read_rds_quality")):
        assert re.search(r"\b%s\s*\(" % name, hpp) and call in hpp, name


CPP_CALLER = """
#define FMD_NO_CFMDECODER_ALIAS
#include "fm_decoder.hpp"
struct R {
  bool AddUECPDataFrame(unsigned char*, unsigned) { return true; }
  bool SetChannelName(std::string) { return true; }
  bool IsSettingActive() { return false; }
};
unsigned use(cFmDecoderT<R>& d) {
  fmd_rds_block b[4];
  fmd_rds_quality q;
  unsigned lost = 0;
  static_assert(sizeof(fmd_rds_block) == 24 && sizeof(fmd_rds_quality) == 32, "the records");
  return d.SetRdsBlocks(FMD_RDS_BLOCKS_RECORD) + d.CollectRdsBlocks(b, 4, &lost) + d.GetRdsQuality(&q);
}
"""


def test_a_cpp_caller_of_the_three_methods_compiles(tmp_path):
    """the members of a class template are only compiled where they are used: use them (host compiler, no GPU)"""
    src = tmp_path / "caller.cpp"
    src.write_text(CPP_CALLER)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_records_are_24_and_32_bytes(pkg):
    assert C.sizeof(pkg.FmdRdsBlock) == 24 and pkg.RDS_BLOCK_DTYPE.itemsize == 24
    assert C.sizeof(pkg.FmdRdsQuality) == 32 and pkg.RDS_QUALITY_DTYPE.itemsize == 32
    assert pkg.RDS_BLOCK_DTYPE == spec.BLOCK_DTYPE
    assert tuple(pkg.RDS_QUALITY_DTYPE.names) == spec.QUALITY_FIELDS
    for (name, _t), off in zip(pkg.FmdRdsBlock._fields_, (0, 4, 8, 12, 16, 18, 20, 21, 22, 23)):
        assert getattr(pkg.FmdRdsBlock, name).offset == off == pkg.RDS_BLOCK_DTYPE.fields[name][1]
    hdr = open(os.path.join(ROOT, "include", "fmd.h")).read()
    body = re.search(r"typedef struct fmd_rds_block \{(.*?)\} fmd_rds_block;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(\w+);", body) == [n for n, _t in pkg.FmdRdsBlock._fields_]
    body = re.search(r"typedef struct fmd_rds_quality \{(.*?)\} fmd_rds_quality;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b([a-z_]+)\b[,;]", body) == list(spec.QUALITY_FIELDS)


def test_a_null_batch_is_refused_without_a_device(pkg):
    L = pkg.lib()
    rec, q, lost = np.zeros(4, pkg.RDS_BLOCK_DTYPE), np.zeros(4, pkg.RDS_QUALITY_DTYPE), C.c_uint(7)
    assert L.fmd_batch_set_rds_blocks(None, 1, 0) < 0
    assert b"null" in L.fmd_last_error()
    assert L.fmd_batch_get_rds_blocks(None) < 0
    assert L.fmd_batch_collect_rds_blocks(None, rec.ctypes.data, 4, 0, None, C.byref(lost)) < 0
    assert L.fmd_batch_read_rds_quality(None, 0, 1, q.ctypes.data) < 0
    assert not rec.view(np.uint8).any() and not q.view(np.uint8).any()
