"""CPU-only checks of the output selections of the C ABI (fmd_batch_select_audio / _mpx and their getters,
include/fmd.h): the four entry points are exported, declared and bound; without a batch every one
of them fails loudly (FMD_ERR_ARG and a sentence) before the HIP runtime is touched; and the Python wrappers refuse a
list with a channel twice, a channel out of range or more rows than channels themselves, before any call into the
library -- this file runs without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package

FMD_ERR_ARG = -1
SYMBOLS = ("fmd_batch_select_audio", "fmd_batch_select_mpx", "fmd_batch_get_audio_selection",
           "fmd_batch_get_mpx_selection")


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def test_selection_symbols_are_exported_declared_and_bound(pkg):
    lib = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "fmd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in pkg.EXPORTS
        assert getattr(lib, name).argtypes is not None, name
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared in include/fmd.h"
    for name in ("select_audio", "select_mpx", "audio_selection", "mpx_selection"):
        assert hasattr(pkg.Batch, name), name
    # the header's list of what a state blob does not carry names the selections
    assert re.search(r"NOT carried:.*?output selections", hdr, flags=re.S)


@pytest.mark.parametrize("name", SYMBOLS)
@pytest.mark.parametrize("with_list", [True, False], ids=["list", "null-list"])
def test_null_batch_is_refused(pkg, name, with_list):
    """no batch: FMD_ERR_ARG and a sentence that names the function, whatever the list is"""
    lib = pkg.lib()
    ch = np.array([0, 1, 2], np.uint32)
    assert getattr(lib, name)(None, ch.ctypes.data if with_list else None, 3 if with_list else 0) == FMD_ERR_ARG
    msg = lib.fmd_last_error()
    assert name.encode() in msg and b"null" in msg and len(msg.split()) >= 3, msg


def _unborn_batch(pkg, n):
    """a Batch object without a library handle: any call into the library with it would fail on the null batch with
    another sentence, so a refusal worded by the Python layer was made in front of that call"""
    b = pkg.Batch.__new__(pkg.Batch)
    b._h = None
    b.sink = None
    b.n_channels = n
    return b


@pytest.mark.parametrize("which", ["select_audio", "select_mpx"])
def test_python_layer_refuses_bad_lists_itself(pkg, which):
    b = _unborn_batch(pkg, 8)
    with pytest.raises(pkg.FmdError, match="fmd error -1: %s: a channel is listed twice" % which):
        getattr(b, which)([1, 5, 1])
    with pytest.raises(pkg.FmdError, match="fmd error -1: %s: a channel is out of range" % which):
        getattr(b, which)([0, 8])
    with pytest.raises(pkg.FmdError, match="fmd error -1: %s: a channel is out of range" % which):
        getattr(b, which)([-1])
    with pytest.raises(pkg.FmdError, match="fmd error -1: %s: more rows than the batch has channels" % which):
        getattr(b, which)(list(range(8)) + [0])
    # a good list reaches the library, which refuses the null batch with its own sentence
    with pytest.raises(pkg.FmdError, match="fmd error -1: fmd_batch_%s: null batch" % which):
        getattr(b, which)([7, 0, 3])
    with pytest.raises(pkg.FmdError, match="fmd error -1: fmd_batch_%s: null batch" % which):
        getattr(b, which)(None)
    with pytest.raises(pkg.FmdError, match="fmd error -1: fmd_batch_%s: null batch" % which):
        getattr(b, which)([])
