"""What the loudness meter costs (fmd_batch_set_loudness, include/fmd.h): calls with the meter off, calls with it on
beside the float audio of every channel, and calls with it on and an empty audio selection (the logging site's case:
no audio row is written) on one box, every variant visited twice in alternation in one process.

  8192 channels x 65 536 samples, 2.4 MS/s, D = 11, the default 100 ms block and ring of 64, a device-resident float
  input row per channel, overlapped calls (concurrency 2) consumed two calls late as bench.py runs them, the blocks
  collected with the groups.  Per visit: ms per step; per variant: MS/s of the better visit.
  The audio tail's own time of each variant from the batch's stage times (profiling level 2: every kernel of a call on
  one stream, events between the stages).
  The host entry point on one shared byte capture: the meter and no audio rows (the blocks collected behind every call)
  against float audio for all channels, ms per call.

One JSON line, also written to profiles/loud.json.

    python tools/loud_bench.py --steps 240 --warmup 8
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
FS, D = 2.4e6, 11
VISITS = ["off", "on", "on_only", "off", "on", "on_only"]


def make(pkg, variant):
    b = pkg.Batch(pkg.make_params(FS, -0.15 * FS, 48000.0, 15000.0, D), C, record_callbacks=False)
    if variant != "off":
        b.set_loudness(True)
    if variant == "on_only":
        b.select_audio([])
    return b


def run(pkg, iq, variant, steps, warmup, profile=False):
    b = make(pkg, variant)
    if profile:
        b.set_profiling(2)
    else:
        b.set_concurrency(2)
    a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
    audio = [torch.empty((C, a_stride), dtype=torch.float32, device="cuda") for _ in range(LAG + 3)]
    s = torch.cuda.current_stream().cuda_stream
    lag = 0 if profile else LAG
    t0, blocks = None, 0
    for j in range(warmup + steps):
        if j == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        b.process_device(iq[j % RING].data_ptr(), N, N, audio[j % len(audio)].data_ptr(), a_stride, s)
        if j >= lag:
            b.wait(stream=s, lag=lag)
            b.collect_rds_array(cap=4 * C, stream=s, lag=lag)
            if variant != "off":
                blocks += len(b.collect_loudness(lag=lag, cap=64, stream=s)[0])
    b.wait(stream=s)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    tail = b.stage_ms()[0].get("audio_tail", -1.0) if profile else None
    b.close()
    return ms, blocks, tail


def run_host(pkg, capture, variant, calls):
    """ms per host-buffer call on a shared byte capture: the meter with no audio rows, or float audio of all channels"""
    lib = pkg.lib()
    b = make(pkg, variant)
    a_stride = b.max_audio_floats(N)
    nf, nm, nfeed = C_.c_uint(), C_.c_uint(), C_.c_uint()
    audio = None if variant == "on_only" else np.zeros((C, a_stride), np.float32)
    ms = []
    for j in range(calls + 2):
        x = capture[j % len(capture)]
        t0 = time.perf_counter()
        rc = lib.fmd_batch_process_host_feed(b._h, x.ctypes.data, pkg.FMD_IQ_U8, 0, N,
                                             None if audio is None else audio.ctypes.data, pkg.FMD_PCM_F32, a_stride,
                                             C_.byref(nf), None, 0, 0, C_.byref(nm), None, pkg.FMD_FEED_S16, 0,
                                             C_.byref(nfeed))
        assert rc >= 0, lib.fmd_last_error()
        if variant != "off":
            b.collect_loudness(cap=64)
        if j >= 2:
            ms.append((time.perf_counter() - t0) * 1e3)
    b.close()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--host-calls", type=int, default=12)
    ap.add_argument("--serial-steps", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loud.json"))
    args = ap.parse_args()
    pkg = load_package()
    gen = fmsig_py.DeviceGenerator([fmsig_py.channel_params(FS, c) for c in range(C)], "cuda")
    iq = torch.empty((RING, C, N, 2), dtype=torch.float32, device="cuda")
    for r in range(RING):
        gen.generate(iq[r], r * N, N)
    torch.cuda.synchronize()
    res = {"tool": "loud_bench", "channels": C, "samples": N, "sample_rate_if": FS, "downsample": D,
           "block_frames": 4800, "ring_blocks": 64, "lag": LAG, "steps": args.steps, "warmup": args.warmup,
           "order_of_visits": VISITS}
    visits = {v: [] for v in set(VISITS)}
    blocks = {}
    for v in VISITS:
        ms, blocks[v], _ = run(pkg, iq, v, args.steps, args.warmup)
        visits[v].append(round(ms, 4))
    for v in ("off", "on", "on_only"):
        res[v] = {"ms_per_step": visits[v], "ms_samples_per_s": round(C * N / (min(visits[v]) * 1e-3) / 1e6, 1),
                  "blocks_collected": blocks[v]}
    for v in ("on", "on_only"):
        res[v]["ms_per_step_vs_off"] = round(min(visits[v]) - min(visits["off"]), 4)
        res[v]["ratio_to_off"] = round(min(visits[v]) / min(visits["off"]), 4)
    tails = {v: round(run(pkg, iq, v, args.serial_steps, 4, profile=True)[2], 4) for v in ("off", "on", "on_only")}
    res["audio_tail_ms"] = dict(tails, steps=args.serial_steps, how="stage times at profiling level 2")
    del iq
    torch.cuda.empty_cache()
    p = fmsig_py.default_params(FS)
    capture = [np.clip(np.round(fmsig_py.generate_f32(p, r * N, N) * 127.5 + 127.5), 0, 255).astype(np.uint8)
               for r in range(RING)]
    host_meter = run_host(pkg, capture, "on_only", args.host_calls)
    host_audio = run_host(pkg, capture, "off", args.host_calls)
    res["host_entry_point"] = {"input": "one shared byte capture", "calls": args.host_calls,
                               "meter_and_no_audio_rows_ms": round(float(np.median(host_meter)), 3),
                               "float_audio_of_all_channels_ms": round(float(np.median(host_audio)), 3)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
