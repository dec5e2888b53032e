"""What delivering every channel's IF-filtered IQ costs (FMD_CIQ_*, include/fmd.h): calls without the rows against
calls with all complex64 rows, all int16 rows and 64 selected complex64 rows on one box, every variant visited twice in
alternation (none, f32, s16, sel64, none, f32, s16, sel64) in one process.

  8192 channels x 65 536 samples, 2.4 MS/s, D = 11, a device-resident float input row per channel, overlapped calls
  (concurrency 2) consumed two calls late as bench.py runs them, float audio.  Per visit: ms per step; per variant:
  MS/s of the better visit and the cost against the better visit without rows.  Against the floor by bytes: the writer
  reads rows x M x 8 bytes and writes rows x M x 8 or 4, at 0.79 of 8 TB/s.

One JSON line, also written to profiles/ciq.json.

    python tools/ciq_bench.py --steps 240 --warmup 8
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
VARIANTS = ["none", "f32", "s16", "sel64"]
COPY_RATE = 0.79 * 8e12  # bytes per second: the chip's measured copy rate (README)
FMT = {"f32": np.complex64, "s16": np.int16, "sel64": np.complex64}
SELECTED = [(127 * i + 5) % C for i in range(64)]  # 64 channels spread over the batch, in no order


def run(pkg, iq, variant, steps, warmup):
    b = pkg.Batch(pkg.make_params(FS, -0.15 * FS, 48000.0, 15000.0, D), C, record_callbacks=False)
    b.set_concurrency(2)
    a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
    q_stride = (b.max_mpx_samples(N) + 63) // 64 * 64
    audio = [torch.empty((C, a_stride), dtype=torch.float32, device="cuda") for _ in range(LAG + 3)]
    rows, n_rows = None, 0
    if variant != "none":
        n_rows = 64 if variant == "sel64" else C
        if variant == "sel64":
            b.select_ciq(SELECTED)
        rows = [torch.empty((n_rows, 2 * q_stride), dtype=torch.int16 if variant == "s16" else torch.float32,
                            device="cuda") for _ in range(LAG + 3)]
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
                                    d_ciq_ptr=rows[j % len(rows)].data_ptr(), ciq_stride=q_stride, ciq=FMT[variant])
        if j >= LAG:
            b.wait(stream=s, lag=LAG)
            b.collect_rds_array(cap=4 * C, stream=s, lag=LAG)
    b.wait(stream=s)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    b.close()
    return ms, m, n_rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--visits", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ciq.json"))
    args = ap.parse_args()
    pkg = load_package()
    gen = fmsig_py.DeviceGenerator([fmsig_py.channel_params(FS, c) for c in range(C)], "cuda")
    iq = torch.empty((RING, C, N, 2), dtype=torch.float32, device="cuda")
    for r in range(RING):
        gen.generate(iq[r], r * N, N)
    torch.cuda.synchronize()
    order = VARIANTS * args.visits
    res = {"tool": "ciq_bench", "channels": C, "samples": N, "sample_rate_if": FS, "downsample": D, "lag": LAG,
           "steps": args.steps, "warmup": args.warmup, "order_of_visits": order}
    visits, shape = {v: [] for v in VARIANTS}, {}
    for v in order:
        ms, m, n_rows = run(pkg, iq, v, args.steps, args.warmup)
        visits[v].append(round(ms, 4))
        shape[v] = (m, n_rows)
    for v in VARIANTS:
        res[v] = {"ms_per_step": visits[v], "ms_samples_per_s": round(C * N / (min(visits[v]) * 1e-3) / 1e6, 1)}
    for v in VARIANTS[1:]:
        m, n_rows = shape[v]
        esz = 4 if v == "s16" else 8
        res[v].update({
            "rows": n_rows, "baseband_length": m, "bytes_read": n_rows * m * 8, "bytes_written": n_rows * m * esz,
            "floor_ms_by_bytes": round(n_rows * m * (8 + esz) / COPY_RATE * 1e3, 4),
            "ms_over_none": round(min(visits[v]) - min(visits["none"]), 4),
            "whole_path_cost_vs_none": round(min(visits[v]) / min(visits["none"]) - 1.0, 4)})
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
