"""What delivering the mono feed costs (FMD_FEED_*, include/fmd.h): calls without it, calls with the int16 feed of every
channel beside the float audio, and calls with the feed alone (an empty audio selection: the stereo rows are not
written) on one box, every variant visited twice in alternation in one process.

  8192 channels x 65 536 samples, 2.4 MS/s, D = 11, feed divisor 3 (16 kHz), a device-resident float input row per
  channel, overlapped calls (concurrency 2) consumed two calls late as bench.py runs them.  Per visit: ms per step;
  per variant: MS/s of the better visit and the bytes a step delivers.
  The same three variants one kernel at a time (concurrency 0: every kernel of a call on one stream, nothing beside
  it): the difference to `none` is what the feed form of the tail, k_feed_out and the roll take by themselves.
  The host entry point (fmd_batch_process_host_feed) on one shared byte capture: the int16 feed alone against float
  audio alone, ms per call.

One JSON line, also written to profiles/feed.json.

    python tools/feed_bench.py --steps 240 --warmup 8
"""
import argparse
import ctypes as C_
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
FS, D, DIV = 2.4e6, 11, 3
VISITS = ["none", "feed", "feed_only", "none", "feed", "feed_only"]


def run(pkg, iq, variant, steps, warmup, mode=2):
    b = pkg.Batch(pkg.make_params(FS, -0.15 * FS, 48000.0, 15000.0, D), C, record_callbacks=False)
    b.set_concurrency(mode)
    a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
    audio = [torch.empty((C, a_stride), dtype=torch.float32, device="cuda") for _ in range(LAG + 3)]
    rows, f_stride, nfeed, nf = None, 0, 0, 0
    if variant != "none":
        b.set_feed(DIV)
        f_stride = (b.max_feed_samples(N) + 63) // 64 * 64
        rows = [torch.empty((C, f_stride), dtype=torch.int16, device="cuda") for _ in range(LAG + 3)]
    if variant == "feed_only":
        b.select_audio([])
    s = torch.cuda.current_stream().cuda_stream
    t0 = None
    for j in range(warmup + steps):
        if j == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        if rows is None:
            nf = b.process_device(iq[j % RING].data_ptr(), N, N, audio[j % len(audio)].data_ptr(), a_stride, s)
        else:
            nf, nfeed = b.process_device(iq[j % RING].data_ptr(), N, N, audio[j % len(audio)].data_ptr(), a_stride, s,
                                         d_feed_ptr=rows[j % len(rows)].data_ptr(), feed_stride=f_stride,
                                         feed=np.int16)
        if mode == 2 and j >= LAG:
            b.wait(stream=s, lag=LAG)
            b.collect_rds_array(cap=4 * C, stream=s, lag=LAG)
        elif mode != 2:
            b.wait(stream=s)
            b.collect_rds_array(cap=4 * C, stream=s)
    b.wait(stream=s)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    b.close()
    delivered = (0 if variant == "feed_only" else C * nf * 4) + C * nfeed * 2
    return ms, delivered


def run_host(pkg, capture, feed_only, calls):
    """ms per fmd_batch_process_host_feed call on a shared byte capture: the int16 feed alone, or float audio alone"""
    lib = pkg.lib()
    b = pkg.Batch(pkg.make_params(FS, -0.15 * FS, 48000.0, 15000.0, D), C, record_callbacks=False)
    a_stride = b.max_audio_floats(N)
    nf, nm, nfeed = C_.c_uint(), C_.c_uint(), C_.c_uint()
    audio = feed = None
    f_stride = 0
    if feed_only:
        b.set_feed(DIV)
        b.select_audio([])
        f_stride = b.max_feed_samples(N)
        feed = np.zeros((C, f_stride), np.int16)
    else:
        audio = np.zeros((C, a_stride), np.float32)
    ms = []
    for j in range(calls + 2):
        x = capture[j % len(capture)]
        t0 = time.perf_counter()
        rc = lib.fmd_batch_process_host_feed(b._h, x.ctypes.data, pkg.FMD_IQ_U8, 0, N,
                                             None if audio is None else audio.ctypes.data, pkg.FMD_PCM_F32, a_stride,
                                             C_.byref(nf), None, 0, 0, C_.byref(nm),
                                             None if feed is None else feed.ctypes.data, pkg.FMD_FEED_S16, f_stride,
                                             C_.byref(nfeed))
        assert rc >= 0, lib.fmd_last_error()
        if j >= 2:
            ms.append((time.perf_counter() - t0) * 1e3)
    b.close()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--host-calls", type=int, default=12)
    ap.add_argument("--serial-steps", type=int, default=48)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feed.json"))
    args = ap.parse_args()
    pkg = load_package()
    gen = fmsig_py.DeviceGenerator([fmsig_py.channel_params(FS, c) for c in range(C)], "cuda")
    iq = torch.empty((RING, C, N, 2), dtype=torch.float32, device="cuda")
    for r in range(RING):
        gen.generate(iq[r], r * N, N)
    torch.cuda.synchronize()
    res = {"tool": "feed_bench", "channels": C, "samples": N, "sample_rate_if": FS, "downsample": D,
           "feed_divisor": DIV, "lag": LAG, "steps": args.steps, "warmup": args.warmup, "order_of_visits": VISITS}
    visits = {v: [] for v in set(VISITS)}
    delivered = {}
    for v in VISITS:
        ms, delivered[v] = run(pkg, iq, v, args.steps, args.warmup)
        visits[v].append(round(ms, 4))
    for v in ("none", "feed", "feed_only"):
        res[v] = {"ms_per_step": visits[v], "ms_samples_per_s": round(C * N / (min(visits[v]) * 1e-3) / 1e6, 1),
                  "bytes_delivered_per_step": delivered[v]}
    for v in ("feed", "feed_only"):
        res[v]["ms_per_step_vs_none"] = round(min(visits[v]) - min(visits["none"]), 4)
    serial = {v: round(run(pkg, iq, v, args.serial_steps, 4, mode=0)[0], 4) for v in ("none", "feed", "feed_only")}
    res["one_kernel_at_a_time"] = {"steps": args.serial_steps, "ms_per_step": serial,
                                   "feed_vs_none": round(serial["feed"] - serial["none"], 4),
                                   "feed_only_vs_none": round(serial["feed_only"] - serial["none"], 4)}
    del iq
    torch.cuda.empty_cache()
    p = fmsig_py.default_params(FS)
    capture = [np.clip(np.round(fmsig_py.generate_f32(p, r * N, N) * 127.5 + 127.5), 0, 255).astype(np.uint8)
               for r in range(RING)]
    host_feed = run_host(pkg, capture, True, args.host_calls)
    host_audio = run_host(pkg, capture, False, args.host_calls)
    res["host_entry_point"] = {"input": "one shared byte capture", "calls": args.host_calls,
                               "s16_feed_alone_ms": round(float(np.median(host_feed)), 3),
                               "float_audio_alone_ms": round(float(np.median(host_audio)), 3)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
