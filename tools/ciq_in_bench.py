"""What a call costs that brings its baseband itself (FMD_IN_CIQ_*, include/fmd.h): calls fed channel IQ rows, as float
pairs and as pairs of 16-bit integers, against the IQ call that produces the same baseband length, on one box, every
variant visited twice in alternation (iq, f32, s16, iq, f32, s16) in one process.

  8192 channels, 2.4 MS/s, D = 11: the IQ call takes 65 536 samples of a device-resident float row per channel, the
  channel IQ calls M = 5958 complex samples per channel -- the rows an IQ call of the same batch delivered (FMD_CIQ_*).
  Overlapped calls (concurrency 2) consumed two calls late as bench.py runs them, float audio.  Per visit: ms per step.
  The copying kernel alone: its own start and stop in a profiled visit of 16 calls (level 1, the IF stage's slot of
  fmd_batch_get_stage_ms), against the floor by bytes -- it reads C x M x 8 or 4 bytes and writes C x M x 8 -- at 0.79
  of 8 TB/s.

One JSON line, also written to profiles/ciq_in.json.

    python tools/ciq_in_bench.py --steps 240 --warmup 8
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
VARIANTS = ["iq", "f32", "s16"]
COPY_RATE = 0.79 * 8e12  # bytes per second: the chip's measured copy rate (README)


def make_rows(pkg, iq):
    """the channel IQ rows of one IQ call per ring slot, in both formats: [C, q_stride] complex64, [C, q_stride, 2] int16"""
    b = pkg.Batch(pkg.make_params(FS, -0.15 * FS, 48000.0, 15000.0, D), C, record_callbacks=False)
    a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
    q_stride = (b.max_mpx_samples(N) + 63) // 64 * 64
    audio = torch.empty((C, a_stride), dtype=torch.float32, device="cuda")
    f32 = torch.zeros((RING, C, q_stride), dtype=torch.complex64, device="cuda")
    s16 = torch.zeros((RING, C, q_stride, 2), dtype=torch.int16, device="cuda")
    m = 0
    for r in range(RING):  # (a fresh batch per format would do as well: the rows only have to be plausible baseband)
        _, m = b.process_device(iq[r].data_ptr(), N, N, audio.data_ptr(), a_stride, d_ciq_ptr=f32[r].data_ptr(),
                                ciq_stride=q_stride, ciq=np.complex64)
    b.reset()
    for r in range(RING):
        _, m = b.process_device(iq[r].data_ptr(), N, N, audio.data_ptr(), a_stride, d_ciq_ptr=s16[r].data_ptr(),
                                ciq_stride=q_stride, ciq=np.int16)
    b.wait()
    torch.cuda.synchronize()
    m = b.max_mpx_samples(N)  # 5958: the call at decimator phase 0 (a later phase gives 5957 and leaves a zero behind)
    b.close()
    return f32, s16, m


def run(pkg, iq, rows, m, variant, steps, warmup, profiling=0):
    b = pkg.Batch(pkg.make_params(FS, -0.15 * FS, 48000.0, 15000.0, D), C, record_callbacks=False)
    b.set_concurrency(2)
    if profiling:
        b.set_profiling(profiling)
    a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
    audio = [torch.empty((C, a_stride), dtype=torch.float32, device="cuda") for _ in range(LAG + 3)]
    s = torch.cuda.current_stream().cuda_stream
    t0 = None
    for j in range(warmup + steps):
        if j == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        out = pkg.make_rows(audio[j % len(audio)].data_ptr(), pkg.FMD_PCM_F32, a_stride)
        if variant == "iq":
            b.process_call(pkg.make_call(iq[j % RING].data_ptr(), pkg.FMD_IQ_F32, N, N, audio=out, stream=s))
        else:
            b.process_call(ciq_in=rows[variant][j % RING][:, :m], audio=out, stream=s)
        if j >= LAG:
            b.wait(stream=s, lag=LAG)
            b.collect_rds_array(cap=4 * C, stream=s, lag=LAG)
    b.wait(stream=s)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    stage = b.stage_ms()[0] if profiling else None
    b.close()
    return ms, stage


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--visits", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ciq_in.json"))
    args = ap.parse_args()
    pkg = load_package()
    gen = fmsig_py.DeviceGenerator([fmsig_py.channel_params(FS, c) for c in range(C)], "cuda")
    iq = torch.empty((RING, C, N, 2), dtype=torch.float32, device="cuda")
    for r in range(RING):
        gen.generate(iq[r], r * N, N)
    torch.cuda.synchronize()
    f32, s16, m = make_rows(pkg, iq)
    rows = {"f32": f32, "s16": s16}
    order = VARIANTS * args.visits
    res = {"tool": "ciq_in_bench", "channels": C, "samples": N, "baseband_length": m, "sample_rate_if": FS,
           "downsample": D, "lag": LAG, "steps": args.steps, "warmup": args.warmup, "order_of_visits": order}
    visits = {v: [] for v in VARIANTS}
    for v in order:
        ms, _ = run(pkg, iq, rows, m, v, args.steps, args.warmup)
        visits[v].append(round(ms, 4))
    for v in VARIANTS:
        res[v] = {"ms_per_step": visits[v]}
    res["iq"]["ms_samples_per_s"] = round(C * N / (min(visits["iq"]) * 1e-3) / 1e6, 1)
    for v in VARIANTS[1:]:
        esz = 4 if v == "s16" else 8
        _, stage = run(pkg, iq, rows, m, v, 16, 4, profiling=1)  # the copying kernel's own time, 16 profiled calls
        first = next(iter(stage.items()))
        res[v].update({
            "baseband_ms_samples_per_s": round(C * m / (min(visits[v]) * 1e-3) / 1e6, 1),
            "step_vs_iq_call": round(min(visits[v]) / min(visits["iq"]), 4),
            "bytes_read": C * m * esz, "bytes_written": C * m * 8,
            "floor_ms_by_bytes": round(C * m * (8 + esz) / COPY_RATE * 1e3, 4),
            "copy_kernel_ms": round(first[1], 4), "copy_kernel_slot": first[0]})
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
