"""Nothing a batch or a scan allocates outlives it.

One process creates, uses and destroys every kind of object the C ABI hands out, five rounds in a row: plain batches
of 64 and 8192 channels, a 16 448-channel shell over sub-batches, a batch with retuning enabled (its silent twin and
restart staging) and one retune, a band scan whose staging and scratch grow, host-buffer calls of growing sizes (the
staging buffers grow) and more than 16 call sizes on a large batch (the half-band plan cache evicts).  After the first
round has warmed the runtime up, the process's device memory must stay where it was: a leaked batch is hundreds of MB
per round.

The process's own VRAM comes from the kernel driver's per-process counters (read only; the entry whose count follows
a 256 MB allocation of the process), which other processes on the same GPU do not move; where there is none the
device-wide hipMemGetInfo stands in.  Either has to see such an allocation before it is trusted.  The child runs
without torch, so the only HIP runtime in it is the library's."""
import os
import subprocess
import sys

import pytest

from __graft_entry__ import ROOT

pytestmark = pytest.mark.gpu

ROUNDS = 5
BOUND_MB = 64

CHILD = r"""
import ctypes as C
import glob
import sys

import numpy as np

sys.path.insert(0, %r)
from __graft_entry__ import load_package

pkg = load_package()
L = C.CDLL(pkg.LIB_PATH)
hip = C.CDLL("libamdhip64.so.7")  # (the runtime the library is bound to)
vp, u = C.c_void_p, C.c_uint
L.fmd_last_error.restype = C.c_char_p
L.fmd_batch_create.argtypes = [C.POINTER(pkg.FmdParams), u, vp, C.c_int, vp, vp, C.POINTER(vp)]
L.fmd_batch_destroy.argtypes = [vp]
L.fmd_batch_max_audio_floats.restype = u
L.fmd_batch_max_audio_floats.argtypes = [vp, u]
L.fmd_batch_process_host.argtypes = [vp, vp, C.c_size_t, u, vp, C.c_size_t, C.POINTER(u)]
L.fmd_batch_collect_rds.argtypes = [vp, vp, u, C.c_int, vp]
L.fmd_batch_enable_retune.argtypes = [vp]
L.fmd_batch_retune_channels.argtypes = [vp, vp, vp, u]
L.fmd_scan_create.argtypes = [C.POINTER(pkg.FmdScanParams), u, C.c_int, C.POINTER(vp)]
L.fmd_scan_destroy.argtypes = [vp]
L.fmd_scan_destroy.restype = None
L.fmd_scan_accumulate_host.argtypes = [vp, vp, C.c_size_t, u]
L.fmd_scan_finish_host.argtypes = [vp, vp, vp, vp, vp, u, vp]


def ok(rc):
    if rc < 0:
        raise RuntimeError("fmd error %%d: %%s" %% (rc, L.fmd_last_error().decode()))
    return rc


rng = np.random.default_rng(7)
NOISE = (0.05 * rng.standard_normal(2 * 65536)).astype(np.float32)
RDS = np.zeros(1 << 16, dtype=pkg.RDS_GROUP_DTYPE)


def batch(n, shifts=None, table_size=0):
    p = pkg.make_params(2.4e6, -0.15 * 2.4e6 if shifts is None else 0.0, 48000.0, 15000.0, 11, table_size=table_size)
    h = vp()
    s = None if shifts is None else np.ascontiguousarray(shifts, np.int32)
    ok(L.fmd_batch_create(C.byref(p), n, None if s is None else s.ctypes.data, 0, None, None, C.byref(h)))
    return h


def call(h, n, samples, shared=True):
    iq = NOISE[:2 * samples] if shared else np.tile(NOISE[:2 * samples], n)
    a_stride = L.fmd_batch_max_audio_floats(h, samples)
    audio = np.empty((n, a_stride), np.float32)
    nf = u()
    ok(L.fmd_batch_process_host(h, iq.ctypes.data, 0 if shared else samples, samples, audio.ctypes.data, a_stride,
                                C.byref(nf)))
    ok(L.fmd_batch_collect_rds(h, RDS.ctypes.data, RDS.size, 0, None))
    assert nf.value > 0


def scan():
    G, T = 64, 64
    p = pkg.FmdScanParams(2.4e6, T, 1024, 100e3, 150e3, 10.0, 0.2)
    h = vp()
    ok(L.fmd_scan_create(C.byref(p), G, 0, C.byref(h)))
    for n in (8192, 32768):  # scratch and staging grow
        iq = np.tile(NOISE[:2 * n], G)
        ok(L.fmd_scan_accumulate_host(h, iq.ctypes.data, n, n))
    psd = np.empty((G, 1024), np.float32)
    slot_db = np.empty((G, T), np.float32)
    floor_db = np.empty(G, np.float32)
    cand = np.empty((G, T), pkg.SCAN_CANDIDATE_DTYPE)
    counts = np.empty(G, np.uint32)
    ok(L.fmd_scan_finish_host(h, psd.ctypes.data, slot_db.ctypes.data, floor_db.ctypes.data, cand.ctypes.data, T,
                              counts.ctypes.data))
    L.fmd_scan_destroy(h)


def one_round():
    h = batch(64)
    for n in (8192, 16384, 32768, 65536):  # host-buffer staging grows (one row per channel)
        call(h, 64, n, shared=False)
    L.fmd_batch_destroy(h)
    h = batch(8192)
    for k in range(18):  # more distinct call sizes than the half-band plan cache keeps (16)
        call(h, 8192, 8192 + 512 * k)
    L.fmd_batch_destroy(h)
    h = batch(16448)  # a shell over sub-batches
    for _ in range(3):
        call(h, 16448, 16384)
    L.fmd_batch_destroy(h)
    shifts = np.arange(1024, dtype=np.int32) %% 24 - 12
    h = batch(1024, shifts, table_size=24)
    ok(L.fmd_batch_enable_retune(h))
    call(h, 1024, 16384)
    ch, sh = np.array([5], np.uint32), np.array([3], np.int32)
    ok(L.fmd_batch_retune_channels(h, ch.ctypes.data, sh.ctypes.data, 1))
    call(h, 1024, 16384)
    call(h, 1024, 16384)
    L.fmd_batch_destroy(h)
    scan()


def kfd_vram(d):
    total = 0
    for f in glob.glob(d + "/vram_*"):
        with open(f) as fh:
            total += int(fh.read().split()[0])
    return total


def kfd_all():
    out = {}
    for d in glob.glob("/sys/class/kfd/kfd/proc/*"):
        try:
            out[d] = kfd_vram(d)
        except (OSError, ValueError):  # (a process that has just gone)
            pass
    return out


def device_used():
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return total.value - free.value


def with_probe(measure):  # measure() before and while this process holds 256 MB more
    p = vp()
    before = measure()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(256 << 20)) == 0
    during = measure()
    assert hip.hipFree(p) == 0
    return before, during


assert hip.hipSetDevice(0) == 0
# this process's KFD entry (its pid there can be another namespace's): the one that sees the probe come
before, during = with_probe(kfd_all)
mine = [d for d in during if during[d] - before.get(d, 0) >= 200 << 20]
source, measure = ("kfd", lambda: kfd_vram(mine[0])) if len(mine) == 1 else ("hipMemGetInfo", device_used)
before, during = with_probe(measure)
print("SOURCE", source, during - before, flush=True)
for r in range(%d):
    one_round()
    assert hip.hipDeviceSynchronize() == 0
    print("ROUND", r, measure(), flush=True)
assert "torch" not in sys.modules
"""


def test_create_use_destroy_leaks_no_device_memory():
    code = CHILD % (ROOT, ROUNDS)
    out = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", code], cwd=ROOT,
                         capture_output=True, text=True, timeout=270)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-3000:])
    lines = out.stdout.splitlines()
    source, probe = [l.split()[1:3] for l in lines if l.startswith("SOURCE")][0]
    used = [int(l.split()[2]) for l in lines if l.startswith("ROUND")]
    assert len(used) == ROUNDS, out.stdout
    assert int(probe) >= 200 << 20, "%s does not see a 256 MB allocation of the process (%s bytes)" % (source, probe)
    growth = max(used[1:]) - used[0]
    print("device memory (%s) after each round, MB:" % source, [round(m / 2 ** 20, 1) for m in used])
    assert growth <= BOUND_MB << 20, "device memory grew by %.1f MB after the first round (%s): %s" % (
        growth / 2 ** 20, source, [round(m / 2 ** 20, 1) for m in used])
