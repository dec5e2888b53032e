"""What selecting the channels that deliver rows saves (fmd_batch_select_audio / _mpx, include/fmd.h, DESIGN.md section
9.9): calls that deliver all rows against calls that deliver 64 and none, on one box, every variant visited twice in
alternation in one process.

  8192 channels x 65 536 samples, 2.4 MS/s, D = 11, a device-resident float input row per channel, overlapped calls
  (concurrency 2) consumed two calls late as bench.py runs them.  Device calls, ms per step per visit: float audio with
  all / 64 / 0 rows (no multiplex), and float multiplex with all / 64 / no rows beside all audio rows.  The host entry
  point fmd_batch_process_host_pcm (float audio, one shared input row, so that the copy in is small), ms per call: all
  rows against 64, with out[2] of fmd_batch_debug_host_ms (waiting for the kernels + copying the audio back) beside it.

One JSON line, also written to profiles/select_outputs.json.

    python tools/select_bench.py --steps 240 --warmup 8
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402
from tools import fmsig_py  # noqa: E402

N, LAG, RING, C = 65536, 2, 3, 8192
FS, D = 2.4e6, 11
# (audio rows, multiplex rows): None = one row per channel, "off" = the call does not ask for the multiplex
DEVICE_VARIANTS = {"audio_all": (None, "off"), "audio_64": (64, "off"), "audio_0": (0, "off"),
                   "mpx_all": (None, None), "mpx_64": (None, 64), "mpx_none": (None, 0)}
VISITS = list(DEVICE_VARIANTS) * 2


def pick(n):
    """n channels spread over the batch, in a shuffled order"""
    return np.random.default_rng(n).permutation(C)[:n].astype(np.uint32)


def run_device(pkg, iq, variant, steps, warmup):
    na, nm = DEVICE_VARIANTS[variant]
    b = pkg.Batch(pkg.make_params(FS, -0.15 * FS, 48000.0, 15000.0, D), C, record_callbacks=False)
    b.set_concurrency(2)
    if na is not None:
        b.select_audio(pick(na))
    if nm not in (None, "off"):
        b.select_mpx(pick(nm))
    a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
    m_stride = (b.max_mpx_samples(N) + 63) // 64 * 64
    audio = [torch.empty((max(1, C if na is None else na), a_stride), dtype=torch.float32, device="cuda")
             for _ in range(LAG + 3)]
    rows = None
    if nm != "off":
        rows = [torch.empty((max(1, C if nm is None else nm), m_stride), dtype=torch.float32, device="cuda")
                for _ in range(LAG + 3)]
    s = torch.cuda.current_stream().cuda_stream
    t0 = None
    for j in range(warmup + steps):
        if j == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        if rows is None:
            b.process_device(iq[j % RING].data_ptr(), N, N, audio[j % len(audio)].data_ptr(), a_stride, s)
        else:
            b.process_device(iq[j % RING].data_ptr(), N, N, audio[j % len(audio)].data_ptr(), a_stride, s,
                             d_mpx_ptr=rows[j % len(rows)].data_ptr(), mpx_stride=m_stride, mpx=np.float32)
        if j >= LAG:
            b.wait(stream=s, lag=LAG)
            b.collect_rds_array(cap=4 * C, stream=s, lag=LAG)
    b.wait(stream=s)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    b.close()
    return ms


def run_host(pkg, x, n_rows, calls, warmup):
    b = pkg.Batch(pkg.make_params(FS, -0.15 * FS, 48000.0, 15000.0, D), C, record_callbacks=False)
    if n_rows is not None:
        b.select_audio(pick(n_rows))
    t0 = None
    for j in range(warmup + calls):
        if j == warmup:
            b.debug_host_ms()  # (a query starts the sums again)
            t0 = time.perf_counter()
        b.process_host_fmt(x, shared=True, pcm=np.float32)
    ms = (time.perf_counter() - t0) * 1e3 / calls
    n, parts = b.debug_host_ms()
    b.close()
    return ms, parts["wait_copy_out"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--host-calls", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_outputs.json"))
    args = ap.parse_args()
    pkg = load_package()
    gen = fmsig_py.DeviceGenerator([fmsig_py.channel_params(FS, c) for c in range(C)], "cuda")
    iq = torch.empty((RING, C, N, 2), dtype=torch.float32, device="cuda")
    for r in range(RING):
        gen.generate(iq[r], r * N, N)
    torch.cuda.synchronize()
    res = {"tool": "select_bench", "channels": C, "samples": N, "sample_rate_if": FS, "downsample": D, "lag": LAG,
           "steps": args.steps, "warmup": args.warmup, "order_of_visits": VISITS}
    visits = {v: [] for v in DEVICE_VARIANTS}
    for v in VISITS:
        visits[v].append(round(run_device(pkg, iq, v, args.steps, args.warmup), 4))
    res["device_ms_per_step"] = visits
    x = iq[0, 0].cpu().numpy().reshape(-1)
    host = {}
    for name, n_rows in (("all", None), ("64", 64), ("all", None), ("64", 64)):
        ms, out2 = run_host(pkg, x, n_rows, args.host_calls, 2)
        host.setdefault(name, {"ms_per_call": [], "wait_copy_out_ms": []})
        host[name]["ms_per_call"].append(round(ms, 3))
        host[name]["wait_copy_out_ms"].append(round(out2, 3))
    res["host_pcm"] = host
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
