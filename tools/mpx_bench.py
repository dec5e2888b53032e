"""What delivering the demodulated multiplex costs (FMD_MPX_*, include/fmd.h): calls without it against calls with
float and with int16 rows on one box, every variant visited twice in alternation (none, f32, s16, none, f32, s16) in
one process.

  8192 channels x 65 536 samples, 2.4 MS/s, D = 11, a device-resident float input row per channel, overlapped calls
  (concurrency 2) consumed two calls late as bench.py runs them, float audio.  Per visit: ms per step; per variant:
  MS/s of the better visit.  The writer kernel's own ms (events at its start and stop,
  fmd_batch_debug_mpx_ms): inside that pipeline (the last 8 calls of a short extra run), and alone (concurrency 0:
  nothing of another call beside it).  Against the floor by bytes: the kernel reads channels x M x 8 bytes (the
  rows are float2, the other half rides along) and writes channels x M x 4 or 2, at 0.79 of 8 TB/s.

One JSON line, also written to profiles/mpx_out.json.

    python tools/mpx_bench.py --steps 240 --warmup 8
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
VISITS = ["none", "f32", "s16", "none", "f32", "s16"]
COPY_RATE = 0.79 * 8e12  # bytes per second: the chip's measured copy rate (README)
FMT = {"f32": np.float32, "s16": np.int16}


def run(pkg, iq, variant, steps, warmup, mode=2, timing=False):
    b = pkg.Batch(pkg.make_params(FS, -0.15 * FS, 48000.0, 15000.0, D), C, record_callbacks=False)
    b.set_concurrency(mode)
    if timing:
        b.debug_mpx_ms()  # (the first query switches the writer's events on)
    a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
    m_stride = (b.max_mpx_samples(N) + 63) // 64 * 64
    audio = [torch.empty((C, a_stride), dtype=torch.float32, device="cuda") for _ in range(LAG + 3)]
    rows = None
    if variant != "none":
        rows = [torch.empty((C, m_stride), dtype=torch.int16 if variant == "s16" else torch.float32, device="cuda")
                for _ in range(LAG + 3)]
    s = torch.cuda.current_stream().cuda_stream
    t0, m = None, 0
    for j in range(warmup + steps):
        if j == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        if rows is None:
            b.process_device(iq[j % RING].data_ptr(), N, N, audio[j % len(audio)].data_ptr(), a_stride, s)
        else:
            _, m = b.process_device(iq[j % RING].data_ptr(), N, N, audio[j % len(audio)].data_ptr(), a_stride, s,
                                    d_mpx_ptr=rows[j % len(rows)].data_ptr(), mpx_stride=m_stride, mpx=FMT[variant])
        if mode == 2 and j >= LAG:
            b.wait(stream=s, lag=LAG)
            b.collect_rds_array(cap=4 * C, stream=s, lag=LAG)
        elif mode != 2:
            b.wait(stream=s)
            b.collect_rds_array(cap=4 * C, stream=s)
    b.wait(stream=s)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    writer = b.debug_mpx_ms() if timing else None
    b.close()
    return ms, writer, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--timing-steps", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpx_out.json"))
    args = ap.parse_args()
    pkg = load_package()
    gen = fmsig_py.DeviceGenerator([fmsig_py.channel_params(FS, c) for c in range(C)], "cuda")
    iq = torch.empty((RING, C, N, 2), dtype=torch.float32, device="cuda")
    for r in range(RING):
        gen.generate(iq[r], r * N, N)
    torch.cuda.synchronize()
    res = {"tool": "mpx_bench", "channels": C, "samples": N, "sample_rate_if": FS, "downsample": D, "lag": LAG,
           "steps": args.steps, "warmup": args.warmup, "order_of_visits": VISITS}
    visits = {"none": [], "f32": [], "s16": []}
    for v in VISITS:
        visits[v].append(round(run(pkg, iq, v, args.steps, args.warmup)[0], 4))
    for v in ("none", "f32", "s16"):
        res[v] = {"ms_per_step": visits[v], "ms_samples_per_s": round(C * N / (min(visits[v]) * 1e-3) / 1e6, 1)}
    for v in ("f32", "s16"):
        _, inside, m = run(pkg, iq, v, args.timing_steps, args.warmup, timing=True)
        _, alone, _ = run(pkg, iq, v, 8, 2, mode=0, timing=True)
        esz = 2 if v == "s16" else 4
        floor_ms = (C * m * 8 + C * m * esz) / COPY_RATE * 1e3
        res[v].update({
            "baseband_length": m, "bytes_read": C * m * 8, "bytes_written": C * m * esz,
            "floor_ms_by_bytes": round(floor_ms, 4),
            "writer_ms_in_pipeline": [round(float(x), 4) for x in inside],
            "writer_ms_alone": [round(float(x), 4) for x in alone],
            "writer_alone_over_floor": round(float(np.median(alone)) / floor_ms, 2) if len(alone) else None,
            "whole_path_cost_vs_none": round(min(visits[v]) / min(visits["none"]) - 1.0, 4)})
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
